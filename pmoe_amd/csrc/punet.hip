// Kernels that only the PU-Net / PMoE model types need:
//   * MaxPool2d(2,2)                                   (blocks/unet.py:29, forward only: the U-Nets are frozen on this path)
//   * ConvTranspose2d(k=2,s=2) scatter                 (unet.py:34-44): the 4 taps are one 1x1 GEMM with 4*Cout rows, this
//                                                       kernel interleaves them into the 2H x 2W output (a channel window of
//                                                       the skip-concat buffer, unet.py:71-84)
//   * channel-window copy                              (torch.cat along C, punet.py:104,113; view(B,-1,H,W), moe.py:311-313)
//   * tanh action head, L1/MSE losses, PMoE blend      (moe.py:317,353-356; loss.py:135-151)
// All of them are HBM-bound streaming kernels: 16-byte vectors, grid-stride, no LDS.
#include "common.h"

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) maxpool2_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W,
                                                      int C, int Ho, int Wo, int x_ld, int x_coff) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int CV = C / VE;
    const long long total = (long long)N * Ho * Wo * CV;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        long long t = i / CV;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const T* p = x + (((size_t)n * H + 2 * oy) * W + 2 * ox) * x_ld + x_coff + cv * VE;
        float a[VE], b[VE], c[VE], d[VE];
        unpack16<T>(ldg16(p), a);
        unpack16<T>(ldg16(p + x_ld), b);
        unpack16<T>(ldg16(p + (size_t)W * x_ld), c);
        unpack16<T>(ldg16(p + (size_t)W * x_ld + x_ld), d);
#pragma unroll
        for (int k = 0; k < VE; ++k) {      // a NaN in the window wins, as in torch and in maxpool2_bwd_kernel (fmaxf drops it)
            const float m = fmaxf(fmaxf(a[k], b[k]), fmaxf(c[k], d[k]));
            a[k] = (a[k] != a[k] || b[k] != b[k] || c[k] != c[k] || d[k] != d[k]) ? __builtin_nanf("") : m;
        }
        stg16(y + (size_t)i * VE, pack16<T>(a));
    }
}

// src [N,H,W,4*C] with channel (dy*2+dx)*C + c  ->  dst[n, 2y+dy, 2x+dx, dst_coff + c]
template <typename T>
__global__ void __launch_bounds__(256) pixel_shuffle2_kernel(const T* __restrict__ src, T* __restrict__ dst, int N, int H,
                                                            int W, int C, int src_ld, int dst_ld, int dst_coff) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int CV = C / VE;
    const long long total = (long long)N * H * W * 4 * CV;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        long long t = i / CV;
        const int q = (int)(t & 3); t >>= 2;
        const int x = (int)(t % W); t /= W;
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        const v4i v = ldg16(src + (((size_t)n * H + y) * W + x) * src_ld + q * C + cv * VE);
        stg16(dst + (((size_t)n * 2 * H + 2 * y + (q >> 1)) * 2 * W + 2 * x + (q & 1)) * dst_ld + dst_coff + cv * VE, v);
    }
}

// rows x C elements between two channel windows; VEC = elements per access (1 when an offset is unaligned)
template <typename T, int VEC>
__global__ void __launch_bounds__(256) copy_window_kernel(const T* __restrict__ src, int src_ld, int src_coff,
                                                         T* __restrict__ dst, int dst_ld, int dst_coff, long long rows,
                                                         int C) {
    const int CV = C / VEC;
    const long long total = rows * CV;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        const long long r = i / CV;
        const T* s = src + (size_t)r * src_ld + src_coff + cv * VEC;
        T* d = dst + (size_t)r * dst_ld + dst_coff + cv * VEC;
        if (VEC == 1) *d = *s;
        else stg16(d, ldg16(s));
    }
}

// ------------------------------------------------------------------------------------------------
// PUNetExpert tail (moe.py:317): actions = tanh(head[:, 0:2]), pred_speed = spd[:, 0]
template <typename T>
__global__ void __launch_bounds__(256) action_head_fwd_kernel(const T* __restrict__ head, int head_ld,
                                                             const T* __restrict__ spd, int spd_ld,
                                                             float* __restrict__ actions, float* __restrict__ speeds, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    actions[b * 2 + 0] = tanhf(to_f32(head[(size_t)b * head_ld + 0]));
    actions[b * 2 + 1] = tanhf(to_f32(head[(size_t)b * head_ld + 1]));
    speeds[b] = to_f32(spd[(size_t)b * spd_ld]);
}

template <typename T>
__global__ void __launch_bounds__(256) action_head_bwd_kernel(const float* __restrict__ actions,
                                                             const float* __restrict__ dact,
                                                             const float* __restrict__ dspeeds, T* __restrict__ dhead,
                                                             int head_ld, T* __restrict__ dspd, int spd_ld, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    T* hr = dhead + (size_t)b * head_ld;
    T* sr = dspd + (size_t)b * spd_ld;
    for (int i = 0; i < head_ld; ++i) {
        float g = 0.f;
        if (i < 2 && dact) {
            const float a = actions[b * 2 + i];
            g = dact[b * 2 + i] * (1.f - a * a);
        }
        hr[i] = from_f32<T>(g);
    }
    sr[0] = from_f32<T>(dspeeds ? dspeeds[b] : 0.f);
    for (int i = 1; i < spd_ld; ++i) sr[i] = from_f32<T>(0.f);
}

// punet_loss / pmoe_loss (loss.py:135-151): c0 * mean|a - a_gt| (+ c1 * mean (s - s_gt)^2), gradients in the same pass
__global__ void __launch_bounds__(256) action_loss_kernel(const float* __restrict__ actions, const float* __restrict__ speeds,
                                                         const float* __restrict__ act_gt, const float* __restrict__ spd_gt,
                                                         float c0, float c1, float* __restrict__ loss,
                                                         float* __restrict__ dact, float* __restrict__ dspeeds, int B) {
    float l1 = 0.f, l2 = 0.f;
    for (int i = threadIdx.x; i < 2 * B; i += 256) {
        const float d = actions[i] - act_gt[i];
        l1 += fabsf(d);
        dact[i] = c0 * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / (2.f * (float)B);
    }
    if (speeds)
        for (int b = threadIdx.x; b < B; b += 256) {
            const float d = speeds[b] - spd_gt[b];
            l2 += d * d;
            dspeeds[b] = c1 * 2.f * d / (float)B;
        }
    __shared__ float r1[256], r2[256];
    r1[threadIdx.x] = l1;
    r2[threadIdx.x] = l2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            r1[threadIdx.x] += r1[threadIdx.x + s];
            r2[threadIdx.x] += r2[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = c0 * r1[0] / (2.f * (float)B) + (speeds ? c1 * r2[0] / (float)B : 0.f);
}

// PMoE blend (moe.py:353-356): out[b][j] = tanh(w_j[0]*moe[b][j] + w_j[1]*punet[b][j] + bias_j), j=0 lateral, j=1 longitudinal
// (one expression for blend_fwd_kernel and mixture_draw_kernel: the closed-loop tick's blend equals pmoe_blend_fwd bit for bit)
__device__ __forceinline__ float blend_value(const float* __restrict__ w, float bias, float moe, float pu) {
    return tanhf(w[0] * moe + w[1] * pu + bias);
}
__global__ void __launch_bounds__(256) blend_fwd_kernel(const float* __restrict__ moe_act, const float* __restrict__ pu_act,
                                                       const float* __restrict__ lat_w, const float* __restrict__ lat_b,
                                                       const float* __restrict__ long_w, const float* __restrict__ long_b,
                                                       float* __restrict__ out, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * B) return;
    const int j = i & 1;
    const float* w = j ? long_w : lat_w;
    const float bias = j ? long_b[0] : lat_b[0];
    out[i] = blend_value(w, bias, moe_act[i], pu_act[i]);
}

// one workgroup: dW_j = sum_b g*[moe, punet], db_j = sum_b g, dpunet = g * w_j[1];  g = dout * (1 - out^2)
__global__ void __launch_bounds__(256) blend_bwd_kernel(const float* __restrict__ moe_act, const float* __restrict__ pu_act,
                                                       const float* __restrict__ lat_w, const float* __restrict__ long_w,
                                                       const float* __restrict__ out, const float* __restrict__ dout,
                                                       float* __restrict__ dlat_w, float* __restrict__ dlat_b,
                                                       float* __restrict__ dlong_w, float* __restrict__ dlong_b,
                                                       float* __restrict__ dpu, int B) {
    float acc[6] = {0, 0, 0, 0, 0, 0};       // lat: w0 w1 b ; long: w0 w1 b
    for (int b = threadIdx.x; b < B; b += 256) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = b * 2 + j;
            const float g = dout[i] * (1.f - out[i] * out[i]);
            acc[j * 3 + 0] += g * moe_act[i];
            acc[j * 3 + 1] += g * pu_act[i];
            acc[j * 3 + 2] += g;
            if (dpu) dpu[i] = g * (j ? long_w[1] : lat_w[1]);
        }
    }
    __shared__ float red[6][256];
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
#pragma unroll
            for (int k = 0; k < 6; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        dlat_w[0] = red[0][0]; dlat_w[1] = red[1][0]; dlat_b[0] = red[2][0];
        dlong_w[0] = red[3][0]; dlong_w[1] = red[4][0]; dlong_b[0] = red[5][0];
    }
}

// ------------------------------------------------------------------------------------------------
// Closed-loop history (pmoe_amd/infer.py:PolicyTick; the agent's deque, autoagents/image_agent.py:63-64,136,158) as a ring that
// stays in place: ring [B][T][L], slot t + 1 moves to slot t (t = 0..T-2), `item` [B][L] becomes slot T-1.  One thread owns one
// element offset (a 16-byte vector, or one element where L is not a multiple of it) in ALL T slots of its row and walks them
// oldest first, so no thread reads what another one writes: in place, no second buffer, no ordering between threads.  The row
// b is blockIdx.y (wave-uniform geometry, no per-element division).  `nhwc` (f32 rings of C channel planes, L = C * HW): the
// same launch also writes the new item as ET [B][HW][Cp], zero padded -- the tensor pmoe_nchw_to_nhwc makes of it (a conversion
// of the same f32 values: bit-identical); that half reads `item` only.
template <typename RT, typename ET, int VEC>
__global__ void __launch_bounds__(256) history_push_kernel(RT* ring, const RT* __restrict__ item, int T, long long L,
                                                          ET* __restrict__ nhwc, int C, long long HW, int Cp) {
    const int b = blockIdx.y;
    RT* row = ring + (size_t)b * T * L;
    const RT* src = item + (size_t)b * L;
    const long long nv = L / VEC;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        RT* p = row + (size_t)i * VEC;
        for (int t = 0; t + 1 < T; ++t, p += L) {
            if (VEC == 1) *p = p[L];
            else stg16(p, ldg16(p + L));
        }
        if (VEC == 1) *p = src[i];
        else stg16(p, ldg16(src + (size_t)i * VEC));
    }
    if (nhwc == nullptr) return;
    constexpr int VE = 16 / (int)sizeof(ET);
    const float* planes = reinterpret_cast<const float*>(src);            // (RT is float on this half: checked by the entry point)
    ET* dst = nhwc + (size_t)b * HW * Cp;
    for (long long px = (long long)blockIdx.x * 256 + threadIdx.x; px < HW; px += (long long)gridDim.x * 256)
        for (int c0 = 0; c0 < Cp; c0 += VE) {
            float v[VE];
#pragma unroll
            for (int k = 0; k < VE; ++k) v[k] = c0 + k < C ? planes[(size_t)(c0 + k) * HW + px] : 0.f;
            stg16(dst + (size_t)px * Cp + c0, pack16<ET>(v));
        }
}

// One draw per batch row from the Gaussian mixture (moe.py:154-156 + dists.sample(), moe.py:337) with the counter-based
// hash_uniform of common.h, and optionally the PMoE blend of the draw.  `state` = {seed, draws_done} lives in device memory:
// every row reads it, then -- behind the barrier -- one lane stores draws_done + 1, so a launch re-issued with the same frozen
// arguments (a recorded plan) draws fresh numbers.  ONE workgroup loops over the rows (B is a handful in the closed loop).
//   u_i = hash_uniform(seed, (draws_done * B + b) * 4 + i);  component = first k with sum(probs[b, 0..k]) > u0 * sum(probs[b, :])
//   (f32 running sums in index order; the last component when none does);  r = sqrt(-2 log(1 - u1));
//   raw[b] = mean[b, k] + std[b, k] * (r cos(2 pi u2), r sin(2 pi u2))
__global__ void __launch_bounds__(256) mixture_draw_kernel(const float* __restrict__ probs, const float* __restrict__ mean,
                                                          const float* __restrict__ sd, unsigned long long* state,
                                                          float* __restrict__ raw, const float* __restrict__ pu_act,
                                                          const float* __restrict__ lat_w, const float* __restrict__ lat_b,
                                                          const float* __restrict__ long_w, const float* __restrict__ long_b,
                                                          float* __restrict__ out, int B, int E) {
    const unsigned long long seed = state[0], done = state[1];
    for (int b = threadIdx.x; b < B; b += 256) {
        const unsigned long long ctr = (done * (unsigned long long)B + (unsigned long long)b) * 4ull;
        const float u0 = hash_uniform(seed, ctr), u1 = hash_uniform(seed, ctr + 1), u2 = hash_uniform(seed, ctr + 2);
        const float* p = probs + (size_t)b * E;
        float total = 0.f;
        for (int e = 0; e < E; ++e) total += p[e];
        const float thr = u0 * total;
        int k = E - 1;
        float run = 0.f;
        for (int e = 0; e < E; ++e) {
            run += p[e];
            if (run > thr) { k = e; break; }
        }
        const float r = sqrtf(-2.f * logf(1.f - u1)), ang = 6.28318530717958647692f * u2;
        const size_t o = ((size_t)b * E + k) * 2;
        const float a0 = mean[o] + sd[o] * (r * cosf(ang)), a1 = mean[o + 1] + sd[o + 1] * (r * sinf(ang));
        raw[b * 2 + 0] = a0;
        raw[b * 2 + 1] = a1;
        if (pu_act) {
            out[b * 2 + 0] = blend_value(lat_w, lat_b[0], a0, pu_act[b * 2 + 0]);
            out[b * 2 + 1] = blend_value(long_w, long_b[0], a1, pu_act[b * 2 + 1]);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) state[1] = done + 1ull;
}

template <typename RT, typename ET>
static int history_push_launch(void* ring, const void* item, int B, int T, long long L, void* nhwc, int C, long long HW, int Cp,
                               hipStream_t stream) {
    constexpr int VR = 16 / (int)sizeof(RT);
    const bool vec = !(L % VR) && !((uintptr_t)ring % 16) && !((uintptr_t)item % 16);
    const long long work = vec ? L / VR : L;
    const dim3 grid(grid_for(work > HW ? work : HW, 8192), B);
    if (vec)
        return launch<history_push_kernel<RT, ET, VR>, 0>(grid, dim3(256), 0, stream, (RT*)ring, (const RT*)item, T, L, (ET*)nhwc,
                                                          C, HW, Cp);
    return launch<history_push_kernel<RT, ET, 1>, 0>(grid, dim3(256), 0, stream, (RT*)ring, (const RT*)item, T, L, (ET*)nhwc, C,
                                                     HW, Cp);
}

// ------------------------------------------------------------------------------------------------
extern "C" {

int pmoe_maxpool2s2_fwd(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t x_ld, int32_t x_coff,
                        int32_t dtype, void* stream) {
    if (H < 2 || W < 2 || N < 1) return PMOE_ERR_ARG;
    const int Ho = H / 2, Wo = W / 2;
    DISPATCH_DT(dtype, {
        constexpr int VE = VecOf<T>::N;
        if (C % VE || !window_ok<T>(C, x_ld, x_coff)) return PMOE_ERR_ARG;
        return launch<maxpool2_kernel<T>, 0>(dim3(grid_for((long long)N * Ho * Wo * (C / VE), 8192)), dim3(256), 0,
                                             (hipStream_t)stream, (const T*)x, (T*)y, N, H, W, C, Ho, Wo, x_ld, x_coff);
    });
}

int pmoe_pixel_shuffle2(const void* src, void* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t src_ld,
                        int32_t dst_ld, int32_t dst_coff, int32_t dtype, void* stream) {
    DISPATCH_DT(dtype, {
        constexpr int VE = VecOf<T>::N;
        if (C % VE || src_ld % VE || src_ld < 4 * C || !window_ok<T>(C, dst_ld, dst_coff)) return PMOE_ERR_ARG;
        return launch<pixel_shuffle2_kernel<T>, 0>(dim3(grid_for((long long)N * H * W * 4 * (C / VE), 8192)), dim3(256), 0,
                                                   (hipStream_t)stream, (const T*)src, (T*)dst, N, H, W, C, src_ld, dst_ld,
                                                   dst_coff);
    });
}

int pmoe_copy_window(const void* src, int32_t src_ld, int32_t src_coff, void* dst, int32_t dst_ld, int32_t dst_coff,
                     int64_t rows, int32_t C, int32_t dtype, void* stream) {
    if (rows < 0 || C < 1 || src_coff + C > src_ld || dst_coff + C > dst_ld) return PMOE_ERR_ARG;
    if (rows == 0) return 0;
    DISPATCH_DT(dtype, {
        constexpr int VE = VecOf<T>::N;
        // whole 16-byte vectors on both sides, or the scalar kernel
        if (!(C % VE) && window_ok<T>(C, src_ld, src_coff) && window_ok<T>(C, dst_ld, dst_coff))
            return launch<copy_window_kernel<T, VE>, 0>(dim3(grid_for(rows * (C / VE), 8192)), dim3(256), 0, (hipStream_t)stream,
                                                        (const T*)src, src_ld, src_coff, (T*)dst, dst_ld, dst_coff,
                                                        (long long)rows, C);
        return launch<copy_window_kernel<T, 1>, 0>(dim3(grid_for(rows * C, 8192)), dim3(256), 0, (hipStream_t)stream, (const T*)src,
                                                   src_ld, src_coff, (T*)dst, dst_ld, dst_coff, (long long)rows, C);
    });
}

int pmoe_action_head_fwd(const void* head, int32_t head_ld, const void* spd, int32_t spd_ld, float* actions,
                         float* speeds, int32_t B, int32_t dtype, void* stream) {
    if (B < 1 || head_ld < 2 || spd_ld < 1) return PMOE_ERR_ARG;
    DISPATCH_DT(dtype, return launch<action_head_fwd_kernel<T>, 0>(dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream,
            (const T*)head, head_ld, (const T*)spd, spd_ld, actions, speeds, B));
}

int pmoe_action_head_bwd(const float* actions, const float* dactions, const float* dspeeds, void* dhead, int32_t head_ld,
                         void* dspd, int32_t spd_ld, int32_t B, int32_t dtype, void* stream) {
    if (B < 1 || head_ld < 2 || spd_ld < 1) return PMOE_ERR_ARG;
    DISPATCH_DT(dtype, return launch<action_head_bwd_kernel<T>, 0>(dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream,
            actions, dactions, dspeeds, (T*)dhead, head_ld, (T*)dspd, spd_ld, B));
}

int pmoe_action_loss(const float* actions, const float* speeds, const float* actions_gt, const float* speed_gt, float c0,
                     float c1, float* loss, float* dactions, float* dspeeds, int32_t B, void* stream) {
    if (B < 1 || (speeds && (!speed_gt || !dspeeds))) return PMOE_ERR_ARG;
    return launch<action_loss_kernel, 0>(dim3(1), dim3(256), 0, (hipStream_t)stream, actions, speeds, actions_gt, speed_gt, c0, c1,
                                         loss, dactions, dspeeds, B);
}

int pmoe_blend_fwd(const float* moe_actions, const float* punet_actions, const float* lat_w, const float* lat_b,
                   const float* long_w, const float* long_b, float* out, int32_t B, void* stream) {
    if (B < 1) return PMOE_ERR_ARG;
    return launch<blend_fwd_kernel, 0>(dim3((2 * B + 255) / 256), dim3(256), 0, (hipStream_t)stream, moe_actions, punet_actions,
                                       lat_w, lat_b, long_w, long_b, out, B);
}

int pmoe_blend_bwd(const float* moe_actions, const float* punet_actions, const float* lat_w, const float* long_w,
                   const float* out, const float* dout, float* dlat_w, float* dlat_b, float* dlong_w, float* dlong_b,
                   float* dpunet, int32_t B, void* stream) {
    if (B < 1) return PMOE_ERR_ARG;
    return launch<blend_bwd_kernel, 0>(dim3(1), dim3(256), 0, (hipStream_t)stream, moe_actions, punet_actions, lat_w, long_w, out,
                                       dout, dlat_w, dlat_b, dlong_w, dlong_b, dpunet, B);
}

int pmoe_history_push(void* ring, const void* item, int32_t B, int32_t T, int64_t L, int32_t dtype, void* nhwc, int32_t C,
                      int32_t Cp, int32_t nhwc_dtype, void* stream) {
    if (!ring || !item || B < 1 || B > 65535 || T < 1 || L < 1) return PMOE_ERR_ARG;
    if (dtype != PMOE_DT_BF16 && dtype != PMOE_DT_F32) return PMOE_ERR_ARG;
    if (!nhwc) {
        if (dtype == PMOE_DT_F32) return history_push_launch<float, float>(ring, item, B, T, L, nullptr, 0, 0, 0, (hipStream_t)stream);
        return history_push_launch<bf16, bf16>(ring, item, B, T, L, nullptr, 0, 0, 0, (hipStream_t)stream);
    }
    // the NHWC copy of the new item: f32 channel planes in, whole 16-byte vectors out
    if (dtype != PMOE_DT_F32 || C < 1 || Cp < C || L % C || (uintptr_t)nhwc % 16) return PMOE_ERR_ARG;
    const long long HW = L / C;
    if (nhwc_dtype == PMOE_DT_F32) {
        if (Cp % 4) return PMOE_ERR_ARG;
        return history_push_launch<float, float>(ring, item, B, T, L, nhwc, C, HW, Cp, (hipStream_t)stream);
    }
    if (nhwc_dtype != PMOE_DT_BF16 || Cp % 8) return PMOE_ERR_ARG;
    return history_push_launch<float, bf16>(ring, item, B, T, L, nhwc, C, HW, Cp, (hipStream_t)stream);
}

int pmoe_mixture_draw(const float* probs, const float* mean, const float* std_, void* state, float* raw,
                      const float* punet_actions, const float* lat_w, const float* lat_b, const float* long_w,
                      const float* long_b, float* out, int32_t B, int32_t E, void* stream) {
    if (!probs || !mean || !std_ || !state || !raw || B < 1 || E < 1 || (uintptr_t)state % 8) return PMOE_ERR_ARG;
    if (punet_actions && (!lat_w || !lat_b || !long_w || !long_b || !out)) return PMOE_ERR_ARG;
    return launch<mixture_draw_kernel, 0>(dim3(1), dim3(256), 0, (hipStream_t)stream, probs, mean, std_, (unsigned long long*)state,
                                          raw, punet_actions, lat_w, lat_b, long_w, long_b, out, B, E);
}

}  // extern "C"
