// Device-resident dataset (pmoe_amd/data.py): the resized uint8 frames of a whole training set stay in HBM (FrameStore), a
// batch is an int64 index table plus one gather.  Three memory-bound streams, one workgroup column per gathered row:
//   gather_rows      dst[i] = src[idx[i]] for rows of row_bytes bytes (uint8 NHWC frames for the augmenter, f32 measurement rows)
//   gather_frames    uint8 [n_src][h][w][C] -> f32 [n][C][h][w] = value / 255 (ToTensor, the bits of preprocess.hip px_out<float>)
//   gather_labels    uint8 [n_src][hw] -> int64 [n][hw] (MaskPILToTensor)
// Every byte offset is 64-bit (a store passes 4 GiB at about 28,000 frames of 224 x 224 x 3).  An index outside [0, n_src) reads
// nothing and writes zeros.  No atomics, no host synchronisation.
#include "common.h"

static constexpr int GATHER_MAX_ROWS_Y = 65535;   // grid.y; rows beyond it are walked with a stride

__device__ __forceinline__ bool row_ok(long long r, long long n_src) { return r >= 0 && r < n_src; }

// LANE = v4i (16 bytes), unsigned (4 bytes) or uint8_t; `lanes` = row_bytes / sizeof(LANE)
template <typename LANE>
__global__ void __launch_bounds__(256) gather_rows_kernel(const LANE* __restrict__ src, const long long* __restrict__ idx,
                                                         LANE* __restrict__ dst, long long n_src, long long n, long long lanes) {
    for (long long i = blockIdx.y; i < n; i += gridDim.y) {
        const long long r = idx[i];
        const bool ok = row_ok(r, n_src);
        const LANE* s = src + (ok ? r : 0) * lanes;
        LANE* d = dst + i * lanes;
        for (long long l = (long long)blockIdx.x * 256 + threadIdx.x; l < lanes; l += (long long)gridDim.x * 256) {
            LANE v = {};
            if (ok) v = s[l];
            d[l] = v;
        }
    }
}

// The access shape of augment_point_kernel: a thread takes 4 consecutive pixels (4 C bytes = C dwords) while the frame's first
// byte is 4-byte aligned and writes 4 floats per plane (one 16-byte store where the plane's address allows); the hw % 4 tail
// pixels -- or the whole of a frame that is not aligned, or of a channel count other than CT -- go one at a time.
// CT = 3 or 1: the compiled channel count of the 4-pixel path; CT = 0: single pixels only, C channels.
template <int CT>
__global__ void __launch_bounds__(256) gather_frames_f32_kernel(const uint8_t* __restrict__ store, const long long* __restrict__ idx,
                                                               float* __restrict__ dst, long long n_src, int n, int hw, int C) {
    const int Cc = CT ? CT : C;
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const long long r = idx[i];
        const bool ok = row_ok(r, n_src);
        const uint8_t* fsrc = store + (size_t)(ok ? r : 0) * hw * Cc;
        float* fdst = dst + (size_t)i * hw * Cc;
        int groups = 0;
        if constexpr (CT > 0) {
            groups = ((uintptr_t)fsrc & 3) == 0 ? hw / 4 : 0;
            const bool vec_out = ((uintptr_t)fdst & 15) == 0 && (hw & 3) == 0;
            for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
                unsigned raw[CT];
#pragma unroll
                for (int k = 0; k < CT; ++k) raw[k] = 0u;
                if (ok) {
                    const unsigned* pi = reinterpret_cast<const unsigned*>(fsrc + (size_t)g * (4 * CT));
#pragma unroll
                    for (int k = 0; k < CT; ++k) raw[k] = pi[k];
                }
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    f32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int b = k * CT + c;               // byte of pixel k, channel c
                        o[k] = (float)(uint8_t)((raw[b >> 2] >> ((b & 3) * 8)) & 0xffu) / 255.0f;
                    }
                    float* pl = fdst + (size_t)c * hw + (size_t)g * 4;
                    if (vec_out) {
                        *reinterpret_cast<f32x4*>(pl) = o;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) pl[k] = o[k];
                    }
                }
            }
        }
        for (int pix = groups * 4 + blockIdx.x * 256 + threadIdx.x; pix < hw; pix += gridDim.x * 256) {
            for (int c = 0; c < Cc; ++c) {
                const uint8_t v = ok ? fsrc[(size_t)pix * Cc + c] : (uint8_t)0;
                fdst[(size_t)c * hw + pix] = (float)v / 255.0f;
            }
        }
    }
}

// a thread takes 4 labels (one dword) of an aligned row and writes them as two 16-byte stores where dst allows
__global__ void __launch_bounds__(256) gather_labels_i64_kernel(const uint8_t* __restrict__ store, const long long* __restrict__ idx,
                                                               long long* __restrict__ dst, long long n_src, int n, long long hw) {
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const long long r = idx[i];
        const bool ok = row_ok(r, n_src);
        const uint8_t* fsrc = store + (size_t)(ok ? r : 0) * hw;
        long long* fdst = dst + (size_t)i * hw;
        const long long groups = ((uintptr_t)fsrc & 3) == 0 ? hw / 4 : 0;
        const bool vec_out = ((uintptr_t)fdst & 15) == 0;
        for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
            const unsigned raw = ok ? *reinterpret_cast<const unsigned*>(fsrc + g * 4) : 0u;
            long long* po = fdst + g * 4;
            if (vec_out) {
                v4i lo, hi;
                lo[0] = (int)(raw & 0xffu); lo[1] = 0; lo[2] = (int)((raw >> 8) & 0xffu); lo[3] = 0;
                hi[0] = (int)((raw >> 16) & 0xffu); hi[1] = 0; hi[2] = (int)(raw >> 24); hi[3] = 0;
                stg16(po, lo);
                stg16(po + 2, hi);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) po[k] = (long long)((raw >> (8 * k)) & 0xffu);
            }
        }
        for (long long pix = groups * 4 + (long long)blockIdx.x * 256 + threadIdx.x; pix < hw; pix += (long long)gridDim.x * 256)
            fdst[pix] = ok ? (long long)fsrc[pix] : 0ll;
    }
}

// every address of a gather is a multiple of `a` bytes: both bases and the row pitch
static inline bool aligned_rows(const void* src, const void* dst, long long row_bytes, int a) {
    return !((uintptr_t)src % a) && !((uintptr_t)dst % a) && !(row_bytes % a);
}

static inline dim3 gather_grid(long long work_per_row, long long n) {
    return dim3(grid_for(work_per_row, 1024), (unsigned)(n < GATHER_MAX_ROWS_Y ? n : GATHER_MAX_ROWS_Y));
}

template <typename LANE>
static int launch_rows(const void* src, const int64_t* idx, void* dst, int64_t n_src, int64_t n, int64_t row_bytes, void* stream) {
    const long long lanes = row_bytes / (long long)sizeof(LANE);
    return launch<gather_rows_kernel<LANE>, 0>(gather_grid(lanes, n), dim3(256), 0, (hipStream_t)stream, (const LANE*)src,
                                               (const long long*)idx, (LANE*)dst, (long long)n_src, (long long)n, lanes);
}

extern "C" {

int pmoe_gather_rows(const void* src, const int64_t* idx, void* dst, int64_t n_src, int64_t n, int64_t row_bytes, void* stream) {
    if (!src || !idx || !dst || n_src < 1 || n < 1 || row_bytes < 1 || src == dst) return PMOE_ERR_ARG;
    if (aligned_rows(src, dst, row_bytes, 16)) return launch_rows<v4i>(src, idx, dst, n_src, n, row_bytes, stream);
    if (aligned_rows(src, dst, row_bytes, 4)) return launch_rows<unsigned>(src, idx, dst, n_src, n, row_bytes, stream);
    return launch_rows<uint8_t>(src, idx, dst, n_src, n, row_bytes, stream);
}

int pmoe_gather_frames_to_f32(const uint8_t* store, const int64_t* idx, float* dst_nchw, int64_t n_src, int32_t n, int32_t h,
                              int32_t w, int32_t C, void* stream) {
    // a frame's pixels are indexed with 32-bit integers (like the augmenter's); frames and planes with 64-bit ones
    if (!store || !idx || !dst_nchw || n_src < 1 || n < 1 || h < 1 || w < 1 || C < 1 || (long long)h * w > (1ll << 28))
        return PMOE_ERR_ARG;
    const int hw = h * w;
    const dim3 grid = gather_grid(((long long)hw + 3) / 4, n);
    const long long* tbl = (const long long*)idx;
    const hipStream_t st = (hipStream_t)stream;
    if (C == 3) return launch<gather_frames_f32_kernel<3>, 0>(grid, dim3(256), 0, st, store, tbl, dst_nchw, (long long)n_src, n, hw, C);
    if (C == 1) return launch<gather_frames_f32_kernel<1>, 0>(grid, dim3(256), 0, st, store, tbl, dst_nchw, (long long)n_src, n, hw, C);
    return launch<gather_frames_f32_kernel<0>, 0>(grid, dim3(256), 0, st, store, tbl, dst_nchw, (long long)n_src, n, hw, C);
}

int pmoe_gather_labels_to_i64(const uint8_t* store, const int64_t* idx, int64_t* dst, int64_t n_src, int32_t n, int64_t hw,
                              void* stream) {
    if (!store || !idx || !dst || n_src < 1 || n < 1 || hw < 1) return PMOE_ERR_ARG;
    return launch<gather_labels_i64_kernel, 0>(gather_grid((hw + 3) / 4, n), dim3(256), 0, (hipStream_t)stream, store,
                                               (const long long*)idx, (long long*)dst, (long long)n_src, n, (long long)hw);
}

}  // extern "C"
