// Vision utilities on the device (pmoe_amd/vision.py; the reference's utils/vision.py): class ids -> palette colours, and the
// annotated video frame of draw_on_image -- normalise to uint8, print the measurements with a bitmap font.  The rules are stated in
// include/pmoe_hip.h; tests/vision_ref.py restates them in numpy and the device result equals it bit for bit.
#include "common.h"

// numpy's argmax over n values `stride` apart: the lowest index wins a tie, a NaN is the maximum and the first NaN wins
__device__ __forceinline__ int argmax_np(const float* __restrict__ p, int n, size_t stride) {
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < n; ++c) {
        const float v = p[(size_t)c * stride];
        if (best == best && (v > best || v != v)) {
            best = v;
            bi = c;
        }
    }
    return bi;
}

// One thread per pixel, neighbouring lanes on neighbouring pixels of a row: every class plane is read in whole lines.  The
// palette is device data nobody has checked: an id outside [0, nc) is black and never indexes it.
template <typename OT>
__global__ void __launch_bounds__(256)
decode_mask_kernel(const void* __restrict__ mask, int kind, OT* __restrict__ out, const uint8_t* __restrict__ palette, int nc,
                   int C, int HW) {
    const size_t b = blockIdx.y;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        long long id;
        if (kind == PMOE_MASK_LOGITS_F32)
            id = argmax_np(reinterpret_cast<const float*>(mask) + b * C * HW + p, C, (size_t)HW);
        else if (kind == PMOE_MASK_IDS_I64)
            id = reinterpret_cast<const int64_t*>(mask)[b * HW + p];
        else
            id = reinterpret_cast<const uint8_t*>(mask)[b * HW + p];
        const bool in = id >= 0 && id < nc;
        const uint8_t* col = palette + 3 * (in ? (int)id : 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t v = in ? col[c] : (uint8_t)0;
            if constexpr (sizeof(OT) == 1)
                out[(b * HW + p) * 3 + c] = v;
            else
                out[(b * 3 + c) * HW + p] = (OT)v / (OT)255;
        }
    }
}

// ---- the annotated frame
static constexpr int ANNOT_THREADS = 1024;          // one workgroup walks a whole frame twice: as wide as it can be
static constexpr int ROWS = PMOE_TEXT_ROWS, COLS = PMOE_TEXT_COLS;

__device__ __forceinline__ int put(uint8_t* row, int n, int ch) {
    if (n < COLS) row[n] = (uint8_t)ch;
    return n + 1;
}
__device__ __forceinline__ int put_str(uint8_t* row, int n, const char* s) {
    for (; *s; ++s) n = put(row, n, *s);
    return n;
}
__device__ __forceinline__ int put_uint(uint8_t* row, int n, unsigned v) {
    bool on = false;
    for (unsigned div = 1000000000u; div >= 1; div /= 10) {
        const unsigned d = v / div;
        v -= d * div;
        if (d || on || div == 1) {
            n = put(row, n, '0' + (int)d);
            on = true;
        }
    }
    return n;
}
// "%.3f" of the f32 with these bits, in integers (include/pmoe_hip.h)
__device__ __forceinline__ int put_f3(uint8_t* row, int n, uint32_t bits) {
    const uint32_t ex = (bits >> 23) & 0xffu, mant = bits & 0x7fffffu;
    if (ex == 0xffu && mant) return put_str(row, n, "nan");
    if (bits >> 31) n = put(row, n, '-');
    if (ex == 0xffu) return put_str(row, n, "inf");
    if (ex >= 127u + 20u) return put_str(row, n, "big");
    const unsigned long long m = (unsigned long long)(ex ? (mant | 0x800000u) : mant) * 1000ull;   // < 2^34
    const int s = ex ? 150 - (int)ex : 149;                                                      // 4 .. 149: |x| = m / 1000 / 2^s
    unsigned long long q = 0;
    if (s < 64) {
        const unsigned long long rem = m & ((1ull << s) - 1ull), half = 1ull << (s - 1);
        q = m >> s;
        q += (rem > half || (rem == half && (q & 1ull))) ? 1ull : 0ull;
    }
    const unsigned ip = (unsigned)(q / 1000ull), fr = (unsigned)(q % 1000ull);
    n = put_uint(row, n, ip);
    n = put(row, n, '.');
    n = put(row, n, '0' + (int)(fr / 100u));
    n = put(row, n, '0' + (int)(fr / 10u % 10u));
    return put(row, n, '0' + (int)(fr % 10u));
}

// string r of the frame: position and colour
__device__ __forceinline__ int row_x(int r, int W2) { return (r < 3 || r == 4) ? 5 : W2; }
__device__ __forceinline__ int row_y(int r) { return r < 3 ? 30 + 20 * r : (r < 5 ? 10 : 30 + 20 * (r - 5)); }

// the last string with ink on pixel (x, y): -1 none, 0 red, 1 green
__device__ __forceinline__ int ink(const uint8_t* text, const uint8_t* __restrict__ font, int x, int y, int W2, int rows) {
    for (int r = rows - 1; r >= 0; --r) {
        const int dy = y - row_y(r), dx = x - row_x(r, W2);
        if ((unsigned)dy >= 7u || dx < 0) continue;
        const int ci = dx / 6, gx = dx - ci * 6;
        if (ci >= COLS || gx >= 5) continue;
        const int ch = text[r * COLS + ci] & 127;
        if ((font[ch * 7 + dy] >> (4 - gx)) & 1) return r < 3 ? 0 : 1;
    }
    return -1;
}

__device__ __forceinline__ uint32_t norm_u8(float x, float lo, float d) {
    const float v = __fmul_rn(__fdiv_rn(__fsub_rn(x, lo), d), 255.0f);
    return (v >= 0.0f && v <= 255.0f) ? (uint32_t)(int)v : 0u;
}

// four neighbouring pixels g * 4 .. g * 4 + 3 (they may straddle a row end) -> 12 bytes NHWC as three dwords
__device__ __forceinline__ void store_group(uint32_t* __restrict__ o, int g, const f32x4& r, const f32x4& gr, const f32x4& bl, float lo,
                                            float d, int W, int W2, int rows, const uint8_t* text, const uint8_t* __restrict__ font) {
    uint32_t px[4][3];
    int y = 4 * g / W, x = 4 * g - y * W;
#pragma unroll
    for (int j = 0; j < 4; ++j, ++x) {
        for (; x >= W; x -= W) ++y;
        const int k = (y >= 10 && y < 77) ? ink(text, font, x, y, W2, rows) : -1;
        px[j][0] = k < 0 ? norm_u8(r[j], lo, d) : (k == 0 ? 255u : 0u);
        px[j][1] = k < 0 ? norm_u8(gr[j], lo, d) : (k == 1 ? 255u : 0u);
        px[j][2] = k < 0 ? norm_u8(bl[j], lo, d) : 0u;
    }
    o[3 * g] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
    o[3 * g + 1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
    o[3 * g + 2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
}

// Workgroup b owns frame b.  Phase 1: minimum and maximum (wave reduction, one pair per wave in LDS).  Phase 2: wave 0 formats
// the strings into LDS, one lane per string.  Phase 3: every pixel gets the colour of the last string with ink on it, or its
// normalised value.  `vec`: the frame and its slot are 16- / 4-byte aligned and H W is a multiple of 4 -- a thread then owns four
// neighbouring pixels: three 16-byte reads, three dword writes.
__global__ void __launch_bounds__(ANNOT_THREADS)
frame_annotate_kernel(const float* __restrict__ frames, long long frame_stride, uint8_t* __restrict__ out, int H, int W, int slot0,
                      int capacity, const float* __restrict__ action, const float* __restrict__ speed,
                      const float* __restrict__ command, int n_cmd, const float* __restrict__ control_gt, int gt,
                      const uint8_t* __restrict__ font, uint8_t* __restrict__ text_out, int vec) {
    __shared__ float s_lo[ANNOT_THREADS / 64], s_hi[ANNOT_THREADS / 64];
    __shared__ uint8_t s_text[ROWS * COLS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int HW = H * W;
    const float* img = frames + (size_t)b * (size_t)frame_stride;
    uint8_t* dst = out + (size_t)((slot0 + b) % capacity) * HW * 3;

    float lo = INFINITY, hi = -INFINITY;
    if (vec) {
        // one workgroup reads the whole frame: four independent 16-byte loads per lane in flight (the extrema do not depend on
        // the order)
        const f32x4* v4 = reinterpret_cast<const f32x4*>(img);
        const int n4 = 3 * (HW / 4);
        int i = tid;
        for (; i + 3 * ANNOT_THREADS < n4; i += 4 * ANNOT_THREADS) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = v4[i + u * ANNOT_THREADS];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lo = fminf(lo, v[u][j]);
                    hi = fmaxf(hi, v[u][j]);
                }
        }
        for (; i < n4; i += ANNOT_THREADS) {
            const f32x4 v = v4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo = fminf(lo, v[j]);
                hi = fmaxf(hi, v[j]);
            }
        }
    } else {
        for (size_t i = tid; i < (size_t)3 * HW; i += ANNOT_THREADS) {
            lo = fminf(lo, img[i]);
            hi = fmaxf(hi, img[i]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((tid & 63) == 0) {
        s_lo[tid >> 6] = lo;
        s_hi[tid >> 6] = hi;
    }
    __syncthreads();

    if (tid < ROWS) {
        uint8_t* row = s_text + tid * COLS;
        int n = 0;
        if (tid < 4 || gt) {
            const float* src = tid < 3 ? action : control_gt;                 // (rows 3 and 4 read neither)
            const int what = tid < 3 ? tid : tid - 5;                         // 0 steer, 1 throttle, 2 brake
            if (tid == 3) {
                n = put_str(row, n, "Command: ");
                n = put_uint(row, n, (unsigned)argmax_np(command + (size_t)b * n_cmd, n_cmd, 1));
            } else if (tid == 4) {
                n = put_str(row, n, "Speed: ");
                n = put_f3(row, n, __float_as_uint(speed[b]));
            } else if (what == 0) {
                n = put_str(row, n, "Steer: ");
                n = put_f3(row, n, __float_as_uint(src[2 * b]));
            } else {
                const float pedal = src[2 * b + 1];
                n = put_str(row, n, what == 1 ? "Throttle: " : "Brake: ");
                if ((pedal > 0.0f) == (what == 1))                            // throttle of a positive pedal, brake of any other
                    n = put_f3(row, n, __float_as_uint(pedal) ^ (what == 2 ? 0x80000000u : 0u));
                else
                    n = put_str(row, n, "0.000");
            }
        }
        for (; n < COLS;) n = put(row, n, ' ');
    }
    __syncthreads();

    lo = s_lo[0];
    hi = s_hi[0];
#pragma unroll
    for (int w = 1; w < ANNOT_THREADS / 64; ++w) {
        lo = fminf(lo, s_lo[w]);
        hi = fmaxf(hi, s_hi[w]);
    }
    const float d = __fadd_rn(-lo, hi);
    const int W2 = W / 2, rows = gt ? ROWS : 4;
    if (text_out != nullptr && tid < ROWS * COLS) text_out[(size_t)b * ROWS * COLS + tid] = s_text[tid];

    if (vec) {
        const f32x4* p0 = reinterpret_cast<const f32x4*>(img);
        const f32x4* p1 = reinterpret_cast<const f32x4*>(img + HW);
        const f32x4* p2 = reinterpret_cast<const f32x4*>(img + 2 * (size_t)HW);
        uint32_t* o = reinterpret_cast<uint32_t*>(dst);
        const int n4 = HW / 4;
        int g = tid;
        for (; g + ANNOT_THREADS < n4; g += 2 * ANNOT_THREADS) {            // two groups: six loads in flight
            const int g1 = g + ANNOT_THREADS;
            const f32x4 a0 = p0[g], a1 = p1[g], a2 = p2[g], b0 = p0[g1], b1 = p1[g1], b2 = p2[g1];
            store_group(o, g, a0, a1, a2, lo, d, W, W2, rows, s_text, font);
            store_group(o, g1, b0, b1, b2, lo, d, W, W2, rows, s_text, font);
        }
        for (; g < n4; g += ANNOT_THREADS) store_group(o, g, p0[g], p1[g], p2[g], lo, d, W, W2, rows, s_text, font);
    } else {
        for (int p = tid; p < HW; p += ANNOT_THREADS) {
            const int y = p / W, x = p - y * W;
            const int k = (y >= 10 && y < 77) ? ink(s_text, font, x, y, W2, rows) : -1;
            uint8_t* q = dst + (size_t)p * 3;
            q[0] = (uint8_t)(k < 0 ? norm_u8(img[p], lo, d) : (k == 0 ? 255u : 0u));
            q[1] = (uint8_t)(k < 0 ? norm_u8(img[(size_t)HW + p], lo, d) : (k == 1 ? 255u : 0u));
            q[2] = (uint8_t)(k < 0 ? norm_u8(img[2 * (size_t)HW + p], lo, d) : 0u);
        }
    }
}

extern "C" {

int pmoe_decode_mask(const void* mask, int32_t kind, void* out, int32_t out_dtype, const uint8_t* palette, int32_t nc, int32_t B,
                     int32_t C, int32_t H, int32_t W, void* stream) {
    if (!mask || !out || !palette || nc < 1 || B < 1 || B > 65535 || H < 1 || W < 1) return PMOE_ERR_ARG;
    if (kind != PMOE_MASK_LOGITS_F32 && kind != PMOE_MASK_IDS_I64 && kind != PMOE_MASK_IDS_U8) return PMOE_ERR_ARG;
    if (out_dtype != PMOE_VIS_U8 && out_dtype != PMOE_VIS_F32 && out_dtype != PMOE_VIS_F64) return PMOE_ERR_ARG;
    if (kind == PMOE_MASK_LOGITS_F32 && C < 1) return PMOE_ERR_ARG;
    if ((uintptr_t)mask % (kind == PMOE_MASK_LOGITS_F32 ? 4 : kind == PMOE_MASK_IDS_I64 ? 8 : 1)) return PMOE_ERR_ARG;
    if ((uintptr_t)out % (out_dtype == PMOE_VIS_F32 ? 4 : out_dtype == PMOE_VIS_F64 ? 8 : 1)) return PMOE_ERR_ARG;
    if ((long long)H * W > (1ll << 28)) return PMOE_ERR_ARG;
    const int HW = H * W;
    const dim3 grid(grid_for(HW, 4096), B), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (out_dtype == PMOE_VIS_U8)
        return launch<decode_mask_kernel<uint8_t>, 0>(grid, block, 0, st, mask, kind, (uint8_t*)out, palette, nc, C, HW);
    if (out_dtype == PMOE_VIS_F32)
        return launch<decode_mask_kernel<float>, 0>(grid, block, 0, st, mask, kind, (float*)out, palette, nc, C, HW);
    return launch<decode_mask_kernel<double>, 0>(grid, block, 0, st, mask, kind, (double*)out, palette, nc, C, HW);
}

int pmoe_frame_annotate(const float* frames, int64_t frame_stride, uint8_t* out, int32_t B, int32_t H, int32_t W, int32_t slot0,
                        int32_t capacity, const float* action, const float* speed, const float* command, int32_t n_cmd,
                        const float* control_gt, int32_t gt, const uint8_t* font, uint8_t* text_out, void* stream) {
    if (!frames || !out || !action || !command || !font || (gt && (!speed || !control_gt))) return PMOE_ERR_ARG;
    if ((uintptr_t)frames % 4 || (uintptr_t)action % 4 || (uintptr_t)command % 4 || (uintptr_t)speed % 4 || (uintptr_t)control_gt % 4)
        return PMOE_ERR_ARG;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || n_cmd < 1 || capacity < 1 || B > capacity || slot0 < 0 || slot0 >= capacity)
        return PMOE_ERR_ARG;
    if ((long long)H * W > (1ll << 28) || frame_stride < 3ll * H * W) return PMOE_ERR_ARG;
    const int HW = H * W;
    const int vec = !(HW % 4) && !((uintptr_t)frames % 16) && !(frame_stride % 4) && !((uintptr_t)out % 4);
    return launch<frame_annotate_kernel, 0>(dim3(B), dim3(ANNOT_THREADS), 0, (hipStream_t)stream, frames, (long long)frame_stride, out, H,
                                            W, slot0, capacity, action, speed, command, n_cmd, control_gt, gt ? 1 : 0, font, text_out,
                                            vec);
}

}  // extern "C"
