// Kernels that only STAGE-0 U-Net training needs (reference trainer/train_0.py, model/blocks/unet.py:50-95):
//   * dice_score (trainer/loss.py:20-31): per-pixel arg-max over the class logits, three INTEGER counts per class
//     (intersection, predicted, target), then 2 (inter + eps) / (pred + target + eps) in f32
//   * Dropout2d (unet.py:31,53-65): one keep-or-drop decision per (sample, channel) -- a [N][C] scale table -- and the
//     in-place product of an NHWC channel window with it (forward on the activation, backward on the gradient)
// Counts are integers (LDS and global integer adds: the result does not depend on their order), no float atomics anywhere.
#include "common.h"

constexpr int DICE_MAX_C = 64;

// logits f32 [B][C][HW], target int64 [B][HW].  counts [3][C] (q: 0 arg-max == target == c, 1 arg-max == c, 2 target == c),
// zeroed by the caller.  Ties take the lowest class index (torch.argmax).
__global__ void __launch_bounds__(256) dice_count_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                        int B, int C, long long HW, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int cnt[3][DICE_MAX_C];
    for (int i = threadIdx.x; i < 3 * DICE_MAX_C; i += 256) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / HW, p = i - b * HW;
        const float* px = logits + (size_t)b * C * HW + p;
        float m = px[0];
        int am = 0;
        for (int c = 1; c < C; ++c) {
            const float v = px[(size_t)c * HW];
            if (v > m) { m = v; am = c; }
        }
        const long long t = target[i];
        atomicAdd(&cnt[1][am], 1u);
        if (t >= 0 && t < C) atomicAdd(&cnt[2][(int)t], 1u);
        if (t == am) atomicAdd(&cnt[0][am], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C; i += 256) {
        const int q = i / C, c = i - q * C;
        const unsigned int v = cnt[q][c];
        if (v) atomicAdd(&counts[q * C + c], (unsigned long long)v);
    }
}

__global__ void dice_finalize_kernel(const unsigned long long* __restrict__ counts, int C, float eps, float* __restrict__ dice) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    // loss.py:27-29: inter = (p * t).sum().float() + eps; union = p.sum() + t.sum() + eps (an integer sum, then f32)
    const float inter = (float)counts[c] + eps;
    const float uni = (float)(counts[C + c] + counts[2 * C + c]) + eps;
    dice[c] = 2.f * inter / uni;
}

// table[n][c] = keep ? 1 / (1 - p) : 0, keep with probability 1 - p from the counter-based hash of (seed, n * C + c)
__global__ void __launch_bounds__(256) dropout2d_table_kernel(float* __restrict__ table, long long total, float p, float keep_scale,
                                                             unsigned long long seed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) table[i] = hash_uniform(seed, (unsigned long long)i) >= p ? keep_scale : 0.f;
}

// x[n][pix][coff + c] *= table[n][c]   (in place; C, ld, coff multiples of the 16-byte vector)
template <typename T>
__global__ void __launch_bounds__(256) channel_scale_kernel(T* __restrict__ x, int ld, int coff, const float* __restrict__ table,
                                                           int N, long long HW, int C) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int CV = C / VE;
    const long long total = (long long)N * HW * CV;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        const long long row = i / CV;
        const long long n = row / HW;
        T* px = x + (size_t)row * ld + coff + cv * VE;
        const float* s = table + (size_t)n * C + cv * VE;
        float v[VE];
        unpack16<T>(ldg16(px), v);
#pragma unroll
        for (int k = 0; k < VE; ++k) v[k] *= s[k];
        stg16(px, pack16<T>(v));
    }
}

extern "C" {

int pmoe_dice_score(const float* logits, const int64_t* target, int32_t B, int32_t C, int64_t HW, float epsilon,
                    uint64_t* counts, float* dice, void* stream) {
    if (!logits || !target || !counts || !dice || B < 1 || C < 1 || C > DICE_MAX_C || HW < 1) return PMOE_ERR_ARG;
    HIP_RET(hipMemsetAsync(counts, 0, sizeof(uint64_t) * 3 * (size_t)C, (hipStream_t)stream));
    HIP_RET((launch<dice_count_kernel, 0>(dim3(grid_for((long long)B * HW, 2048)), dim3(256), 0, (hipStream_t)stream, logits,
                                          (const long long*)target, B, C, (long long)HW, (unsigned long long*)counts)));
    return launch<dice_finalize_kernel, 0>(dim3(1), dim3(DICE_MAX_C), 0, (hipStream_t)stream, (const unsigned long long*)counts, C,
                                           epsilon, dice);
}

int pmoe_dropout2d_table(float* table, int32_t N, int32_t C, float p, uint64_t seed, void* stream) {
    if (!table || N < 1 || C < 1 || !(p >= 0.f) || p > 1.f) return PMOE_ERR_ARG;
    const long long total = (long long)N * C;
    const float keep_scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
    return launch<dropout2d_table_kernel, 0>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, total,
                                             p, keep_scale, (unsigned long long)seed);
}

int pmoe_channel_scale(void* x, int32_t ld, int32_t coff, const float* table, int32_t N, int64_t HW, int32_t C, int32_t dtype,
                       void* stream) {
    if (!x || !table || N < 1 || HW < 1 || C < 1 || coff < 0 || coff + C > ld) return PMOE_ERR_ARG;
    DISPATCH_DT(dtype, {
        constexpr int VE = VecOf<T>::N;
        if (C % VE || !window_ok<T>(C, ld, coff)) return PMOE_ERR_ARG;
        return launch<channel_scale_kernel<T>, 0>(dim3(grid_for((long long)N * HW * (C / VE), 8192)), dim3(256), 0,
                                                  (hipStream_t)stream, (T*)x, ld, coff, table, N, (long long)HW, C);
    });
}

}  // extern "C"
