// Train-time image augmenter (model/augmenter.py: the imgaug Sequential between Resize and ToTensor of
// model/data_loader.py:255-271) on resized uint8 NHWC frames.  The operator SET, schedules and ranges are the reference's; the
// per-operator ARITHMETIC is this project's own (include/pmoe_hip.h, pmoe_amd/augment.py) and is restated in numpy by
// tests/augment_ref.py -- no parity with imgaug's random stream or cv2's arithmetic is claimed.  The output is a pure function
// of (pixels, plan): counter-hash randomness, integer blur, single f32 operations without contraction, no atomics.
//
// Launches per batch: point phase 0 [-> blur H -> blur V -> point phase 1]; the blur pair and phase 1 only when some frame of
// the batch drew a blur (the host knows the plan).  Frames without a blur are copied through by the two blur passes.
#include "common.h"

static constexpr int AUG_PLAN_WORDS = (int)(sizeof(pmoe_aug_plan) / 4);
static_assert(sizeof(pmoe_aug_plan) % 4 == 0, "plan rows are staged as dwords");

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int round255(float x) {          // clamp(rint(x)), rint = round-half-even
    x = rintf(x);
    return (int)fminf(fmaxf(x, 0.f), 255.f);
}

// one frame's plan row -> LDS (every thread of the block calls it; ends with a barrier)
__device__ __forceinline__ void stage_plan(const pmoe_aug_plan* __restrict__ plan, int n, pmoe_aug_plan* s_plan) {
    const int32_t* g = reinterpret_cast<const int32_t*>(plan + n);
    int32_t* s = reinterpret_cast<int32_t*>(s_plan);
    for (int i = threadIdx.x; i < AUG_PLAN_WORDS; i += blockDim.x) s[i] = g[i];
    __syncthreads();
}

// the slots [s0, s1) of one pixel (y, x = pix / w, pix % w), channels v[0..2], in plan order
__device__ __forceinline__ void apply_slots(const pmoe_aug_plan* sp, int s0, int s1, int pix, int h, int w, int* v) {
    for (int s = s0; s < s1; ++s) {
        const pmoe_aug_slot& sl = sp->slot[s];
        const int op = sl.op;
        if (op == PMOE_AUG_ADD) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] + (int)sl.p[c]);
        } else if (op == PMOE_AUG_MULTIPLY) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = round255(__fmul_rn((float)v[c], sl.p[c]));
        } else if (op == PMOE_AUG_CONTRAST) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = round255(__fadd_rn(__fmul_rn(sl.p[c], (float)(v[c] - 128)), 128.f));
        } else if (op == PMOE_AUG_GRAYSCALE) {
            const int g = (4899 * v[0] + 9617 * v[1] + 1868 * v[2] + 8192) >> 14;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = round255(__fadd_rn((float)v[c], __fmul_rn(sl.p[c], (float)(g - v[c]))));
        } else if (op == PMOE_AUG_DROPOUT || op == PMOE_AUG_COARSE_DROPOUT || op == PMOE_AUG_NOISE) {
            unsigned long long cell = (unsigned long long)pix;
            if (op == PMOE_AUG_COARSE_DROPOUT) {
                const int hl = sl.hl < 1 ? 1 : sl.hl, wl = sl.wl < 1 ? 1 : sl.wl;
                const int y = pix / w, x = pix - y * w;
                const int yl = (int)((long long)y * hl / h), xl = (int)((long long)x * wl / w);
                cell = (unsigned long long)yl * wl + xl;
            }
            const unsigned long long seed = sl.seed;
            const float p = sl.p[0];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned long long idx = sl.per_channel ? cell * 3 + c : cell;
                if (op == PMOE_AUG_NOISE) {
                    const float u1 = hash_uniform(seed, 2 * idx), u2 = hash_uniform(seed, 2 * idx + 1);
                    const float z = sqrtf(-2.f * logf(1.f - u1)) * cosf(6.28318530717958647692f * u2);
                    v[c] = round255((float)v[c] + p * z);
                } else if (!(hash_uniform(seed, idx) >= p)) {
                    v[c] = 0;
                }
            }
        }                                                   // PMOE_AUG_BLUR (the phase boundary) and unknown codes: nothing
    }
}

template <typename OUT> __device__ __forceinline__ OUT aug_out(int v);
template <> __device__ __forceinline__ uint8_t aug_out<uint8_t>(int v) { return (uint8_t)v; }
template <> __device__ __forceinline__ float aug_out<float>(int v) { return (float)(uint8_t)v / 255.0f; }   // = preprocess.hip px_out<float>

// src [n][h][w][3] uint8 -> OUT = uint8: dst [n][h][w][3];  OUT = float: dst [n][3][h][w] = value / 255 (ToTensor).
// grid (x, n): a block works on one frame; a thread takes 4 consecutive pixels (12 bytes = one dwordx3 load) while the frame's
// first byte is 4-byte aligned, the h*w % 4 tail pixels -- or the whole of a frame that is not aligned -- one at a time.
template <typename OUT>
__global__ void __launch_bounds__(256) augment_point_kernel(const uint8_t* __restrict__ src, OUT* __restrict__ dst,
                                                           const pmoe_aug_plan* __restrict__ plan, int h, int w, int phase) {
    __shared__ pmoe_aug_plan s_plan;
    const int n = blockIdx.y;
    stage_plan(plan, n, &s_plan);
    int ns = s_plan.n_slots;
    ns = ns < 0 ? 0 : (ns > PMOE_AUG_MAX_SLOTS ? PMOE_AUG_MAX_SLOTS : ns);
    const int bs = s_plan.blur_slot;
    const bool has_blur = bs >= 0 && bs < ns;
    const int s0 = phase == 0 ? 0 : (has_blur ? bs + 1 : ns);
    const int s1 = phase == 0 ? (has_blur ? bs : ns) : ns;
    const int hw = h * w;
    const uint8_t* fsrc = src + (size_t)n * hw * 3;
    OUT* fdst = dst + (size_t)n * hw * 3;
    const bool vec_in = ((uintptr_t)fsrc & 3) == 0;
    const int groups = vec_in ? hw / 4 : 0;
    constexpr bool F32 = sizeof(OUT) == 4;
    // vector store: u8 -> 12 bytes at fdst + 12 g (needs 4-byte alignment); f32 -> 4 floats per plane at c*hw + 4 g (16-byte)
    const bool vec_out = F32 ? (((uintptr_t)fdst & 15) == 0 && (hw & 3) == 0) : (((uintptr_t)fdst & 3) == 0);
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const unsigned* pi = reinterpret_cast<const unsigned*>(fsrc + (size_t)g * 12);   // three dwords (a 3-vector type would
        const unsigned raw[3] = {pi[0], pi[1], pi[2]};                                   // be loaded and aligned as 16 bytes)
        int v[4][3];
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b / 3][b % 3] = (int)((raw[b >> 2] >> ((b & 3) * 8)) & 0xffu);
#pragma unroll
        for (int k = 0; k < 4; ++k) apply_slots(&s_plan, s0, s1, 4 * g + k, h, w, v[k]);
        if constexpr (F32) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* pl = reinterpret_cast<float*>(fdst) + (size_t)c * hw + (size_t)g * 4;
                if (vec_out) {
                    f32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = aug_out<float>(v[k][c]);
                    *reinterpret_cast<f32x4*>(pl) = o;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) pl[k] = aug_out<float>(v[k][c]);
                }
            }
        } else {
            uint8_t* po = reinterpret_cast<uint8_t*>(fdst) + (size_t)g * 12;
            if (vec_out) {
                unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
                for (int b = 0; b < 12; ++b) o[b >> 2] |= (unsigned)v[b / 3][b % 3] << ((b & 3) * 8);
                unsigned* pw = reinterpret_cast<unsigned*>(po);
                pw[0] = o[0]; pw[1] = o[1]; pw[2] = o[2];
            } else {
#pragma unroll
                for (int b = 0; b < 12; ++b) po[b] = (uint8_t)v[b / 3][b % 3];
            }
        }
    }
    for (int pix = groups * 4 + blockIdx.x * 256 + threadIdx.x; pix < hw; pix += gridDim.x * 256) {   // scalar tail
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = fsrc[(size_t)pix * 3 + c];
        apply_slots(&s_plan, s0, s1, pix, h, w, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (F32) fdst[(size_t)c * hw + pix] = aug_out<float>(v[c]);
            else fdst[(size_t)pix * 3 + c] = aug_out<uint8_t>(v[c]);
        }
    }
}

// ---- Gaussian blur: two separable integer passes, (sum q_i v + 32768) >> 16 with sum q = 65536, reflect-101 borders, 8-bit
// intermediate.  Taps and K come from the frame's plan row; a frame without a blur (blur_k == 0) is copied through.
static constexpr int BLUR_MAXR = PMOE_AUG_MAX_TAPS / 2;   // 16

__device__ __forceinline__ int reflect101(int i, int n) {  // -1 -> 1, n -> n - 2; clamped (a well-formed plan has K/2 < n)
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// K of a plan row as the kernels use it: 0 (copy) unless odd, 3..PMOE_AUG_MAX_TAPS
__device__ __forceinline__ int blur_taps_of(const pmoe_aug_plan* sp) {
    const int K = sp->blur_k;
    return (K < 3 || K > PMOE_AUG_MAX_TAPS || !(K & 1)) ? 0 : K;
}

// horizontal: a block takes BH_ROWS rows x BH_COLS pixels of one frame; each row segment with its halo of K/2 pixels sits in LDS
static constexpr int BH_ROWS = 4, BH_COLS = 128;
__global__ void __launch_bounds__(256) augment_blur_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const pmoe_aug_plan* __restrict__ plan, int h, int w) {
    __shared__ pmoe_aug_plan s_plan;
    __shared__ uint8_t s_px[BH_ROWS][(BH_COLS + 2 * BLUR_MAXR) * 3];
    const int n = blockIdx.z, y0 = blockIdx.y * BH_ROWS, x0 = blockIdx.x * BH_COLS;
    stage_plan(plan, n, &s_plan);
    const int K = blur_taps_of(&s_plan), r = K >> 1;
    const int rows = min(BH_ROWS, h - y0), cols = min(BH_COLS, w - x0);
    const uint8_t* fsrc = src + (size_t)n * h * w * 3;
    uint8_t* fdst = dst + (size_t)n * h * w * 3;
    const int span = (cols + 2 * r) * 3;                    // staged bytes per row
    for (int e = threadIdx.x; e < rows * span; e += 256) {
        const int rr = e / span, b = e - rr * span;
        const int px = b / 3, c = b - px * 3;
        s_px[rr][b] = fsrc[((size_t)(y0 + rr) * w + reflect101(x0 - r + px, w)) * 3 + c];
    }
    __syncthreads();
    const int obytes = cols * 3;
    for (int e = threadIdx.x; e < rows * obytes; e += 256) {
        const int rr = e / obytes, b = e - rr * obytes;
        int out;
        if (K == 0) {
            out = s_px[rr][b];
        } else {
            int acc = 32768;
            for (int i = 0; i < K; ++i) acc += s_plan.taps[i] * (int)s_px[rr][b + 3 * i];
            out = clamp255(acc >> 16);
        }
        fdst[((size_t)(y0 + rr) * w + x0) * 3 + b] = (uint8_t)out;
    }
}

// vertical: a block takes BV_ROWS rows x BV_COLS pixels; the column strip with K/2 halo rows above and below sits in LDS
static constexpr int BV_ROWS = 32, BV_COLS = 64;
__global__ void __launch_bounds__(256) augment_blur_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const pmoe_aug_plan* __restrict__ plan, int h, int w) {
    __shared__ pmoe_aug_plan s_plan;
    __shared__ uint8_t s_px[BV_ROWS + 2 * BLUR_MAXR][BV_COLS * 3];
    const int n = blockIdx.z, y0 = blockIdx.y * BV_ROWS, x0 = blockIdx.x * BV_COLS;
    stage_plan(plan, n, &s_plan);
    const int K = blur_taps_of(&s_plan), r = K >> 1;
    const int rows = min(BV_ROWS, h - y0), cols = min(BV_COLS, w - x0);
    const uint8_t* fsrc = src + (size_t)n * h * w * 3;
    uint8_t* fdst = dst + (size_t)n * h * w * 3;
    const int rbytes = cols * 3;
    for (int e = threadIdx.x; e < (rows + 2 * r) * rbytes; e += 256) {
        const int rr = e / rbytes, b = e - rr * rbytes;
        s_px[rr][b] = fsrc[((size_t)reflect101(y0 - r + rr, h) * w + x0) * 3 + b];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * rbytes; e += 256) {
        const int rr = e / rbytes, b = e - rr * rbytes;
        int out;
        if (K == 0) {
            out = s_px[rr][b];
        } else {
            int acc = 32768;
            for (int i = 0; i < K; ++i) acc += s_plan.taps[i] * (int)s_px[rr + i][b];
            out = clamp255(acc >> 16);
        }
        fdst[((size_t)(y0 + rr) * w + x0) * 3 + b] = (uint8_t)out;
    }
}

static inline bool aug_args_ok(const void* src, const void* dst, const void* plan, int32_t n_img, int32_t h, int32_t w) {
    // grid.y / grid.z carry the frame index (<= 65535); a frame's pixels are indexed with 32-bit integers
    return src && dst && plan && n_img >= 1 && n_img <= 65535 && h >= 1 && w >= 1 && (long long)h * w <= (1ll << 28);
}

template <typename OUT>
static int launch_point(const uint8_t* src, OUT* dst, const pmoe_aug_plan* plan, int32_t n_img, int32_t h, int32_t w,
                        int32_t phase, void* stream) {
    if (!aug_args_ok(src, dst, plan, n_img, h, w) || (phase != 0 && phase != 1)) return PMOE_ERR_ARG;
    const long long work = ((long long)h * w + 3) / 4;      // one thread per 4 pixels
    return launch<augment_point_kernel<OUT>, 0>(dim3(grid_for(work, 1024), (unsigned)n_img), dim3(256), 0, (hipStream_t)stream, src,
                                                dst, plan, h, w, phase);
}

extern "C" {

int pmoe_augment_point_to_u8(const uint8_t* src, uint8_t* dst, const pmoe_aug_plan* plan, int32_t n_img, int32_t h, int32_t w,
                             int32_t phase, void* stream) {
    if (src == dst) return PMOE_ERR_ARG;
    return launch_point<uint8_t>(src, dst, plan, n_img, h, w, phase, stream);
}

int pmoe_augment_point_to_f32(const uint8_t* src, float* dst_nchw, const pmoe_aug_plan* plan, int32_t n_img, int32_t h, int32_t w,
                              int32_t phase, void* stream) {
    return launch_point<float>(src, dst_nchw, plan, n_img, h, w, phase, stream);
}

int pmoe_augment_blur_h(const uint8_t* src, uint8_t* dst, const pmoe_aug_plan* plan, int32_t n_img, int32_t h, int32_t w,
                        void* stream) {
    if (!aug_args_ok(src, dst, plan, n_img, h, w) || src == dst || (h + BH_ROWS - 1) / BH_ROWS > 65535) return PMOE_ERR_ARG;
    return launch<augment_blur_h_kernel, 0>(dim3((w + BH_COLS - 1) / BH_COLS, (h + BH_ROWS - 1) / BH_ROWS, n_img), dim3(256), 0,
                                            (hipStream_t)stream, src, dst, plan, h, w);
}

int pmoe_augment_blur_v(const uint8_t* src, uint8_t* dst, const pmoe_aug_plan* plan, int32_t n_img, int32_t h, int32_t w,
                        void* stream) {
    if (!aug_args_ok(src, dst, plan, n_img, h, w) || src == dst || (h + BV_ROWS - 1) / BV_ROWS > 65535) return PMOE_ERR_ARG;
    return launch<augment_blur_v_kernel, 0>(dim3((w + BV_COLS - 1) / BV_COLS, (h + BV_ROWS - 1) / BV_ROWS, n_img), dim3(256), 0,
                                            (hipStream_t)stream, src, dst, plan, h, w);
}

}  // extern "C"
