// Gradients with respect to the network's INPUTS: d loss / d images through the stem's first convolution, and
// d loss / d speed, d loss / d command through the first Linear of the measurement encoders.  All three inputs are SHARED by
// the E experts of a mixture while every gradient upstream of them is per expert, so the expert sum is part of the reduction
// of each kernel: one launch, f32 accumulation in a fixed order, no atomics, no per-expert intermediate.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// Stem input gradient (basics.py:61-76,86-106 backward, summed over the experts of moe.py:141-149):
//
//   dx[b][c][h][w] = sum_e ( sum_{r,s,co} dz[e*B + b][h - 1 + r][w - 1 + s][co] * wd[e*B + b][c][r*3 + s][co]  +  dgap[e*B + b][c] )
//
// dz: T [E*B][H][W][64] (the gradient of conv1's output).  wd: the data-gradient half of pmoe_pack_conv_weights_gated,
// T [E*B][cinp2][9][coutp2] = W_e[co][c][8 - tap] * gate[e*B + b][c] (flipped taps, gate folded in).  dgap: f32 [E*B][16], the
// gradient that reaches every pixel through the gate's pooled input, already divided by H*W (pmoe_eca_bwd_small, dgap_scale), or
// NULL.  dx: f32 [B][creal][H][W] planes, the caller's own image layout; channels creal..15 are computed and dropped.
//
// bf16: the mirror image of conv3x3_c16_kernel.  v_mfma_f32_16x16x32_bf16 with M = 16 consecutive pixels of a row, N = the 16
// (padded) input channels, K = 32 output channels of one tap: a lane's A fragment is 8 consecutive channels of one pixel -- one
// 16-byte load straight from the NHWC row, no LDS -- and its B fragment 8 consecutive co of one (c, tap) row of the pack.  A wave
// owns 16 columns x ROWS rows of dx and walks the ROWS + 2 rows of dz it needs once per expert.  A row is loaded once (plus one
// halo pixel on either side); its three column taps are DPP lane shifts of the loaded fragment, and each fragment feeds the three
// output rows it is a tap of.  (Loading the row at its three column shifts instead, the second and third from the vector cache,
// ran at 2.1 TB/s of dz: the cache's request rate was the limit.  DESIGN.md section 2.)  The four waves of a workgroup sit side
// by side in the row; workgroups whose bands share halo rows run on one XCD and meet in its L2.  The 18 B fragments of an
// (expert, image) stay in registers for the whole walk.  Accumulation order per output element: expert, dz row, column tap, K chunk.
constexpr int IG_ROWS = 8;

__global__ void __launch_bounds__(256, 3) stem_input_grad_mfma_kernel(const bf16* __restrict__ dz, const bf16* __restrict__ wd,
                                                                   const float* __restrict__ dgap, float* __restrict__ dx, int E,
                                                                   int B, int H, int W, int creal, int cinp2, int coutp2, int gx,
                                                                   int gy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    // logical tile order: the 64-column tiles of a row band, the bands of an image, the images -- a contiguous run of it per XCD
    // (xcd_remap), so that the bands which share halo rows meet in one L2
    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int w0 = ((int)(bid % (unsigned)gx) * 4 + wave) * 16, h0 = (int)(bid / (unsigned)gx % (unsigned)gy) * IG_ROWS;
    const int b = (int)(bid / ((unsigned)gx * (unsigned)gy));
    if (w0 >= W) return;                                   // (no barrier in this kernel: a wave past the right edge just leaves)
    f32x4 acc[IG_ROWS];
#pragma unroll
    for (int j = 0; j < IG_ROWS; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A dz row is loaded ONCE: the wave's own 16 pixels by all lanes (fragment `c`), the pixel left of them by lane m = 0 and the
    // pixel right of them by lane m = 15 of every 16-lane row (fragment `h`).  The column taps are lane shifts of that: the DPP
    // row shifts move a fragment by one pixel inside the 16 lanes that share a K group and leave `h` in the lane that has no
    // source.  Loads come from clamped addresses and are ANDed with a mask that is zero where the pixel lies outside the map (a
    // select would be turned back into a branch around the load).  Per dz row: the loads of the NEXT row, the MFMAs of this one,
    // then masks and shifts on what has arrived -- the scheduling barriers keep that order.
    const bool edge = m == 0 || m == 15;
    const int wc = w0 + m, wh = m == 0 ? w0 - 1 : w0 + 16;
    const unsigned ofs_c = (unsigned)((wc >= W ? W - 1 : wc) * 64 + q * 8) * 2u;       // byte offsets in a dz row: a uniform row
    const unsigned ofs_h = (unsigned)((wh < 0 ? 0 : wh >= W ? W - 1 : wh) * 64 + q * 8) * 2u;      // base + these two, no more
    const int ok_c = wc < W ? -1 : 0, ok_h = edge && wh >= 0 && wh < W ? -1 : 0;
    float bias = 0.f;
    for (int e = 0; e < E; ++e) {
        const size_t n = (size_t)e * B + b;
        const bf16* wn = wd + (n * cinp2 + m) * 9 * (size_t)coutp2 + q * 8;        // row (c = m) of this (expert, image) pack
        v4i bw[9][2];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) bw[t][kc] = ldg16(wn + t * coutp2 + kc * 32);
        if (dgap) bias += dgap[n * 16 + m];
        const char* dn = (const char*)(dz + n * H * W * 64);
        v4i cur[3][2], c[2], h[2];
        auto load_row = [&](int hi) {
            int hp = h0 + hi;                              // the dz row; tap row r reaches output row hp + 1 - r
            // (opaque to the optimiser: the row offsets and masks of all ROWS + 2 rows would otherwise be hoisted out of the
            //  expert loop and held in ~100 registers)
            asm volatile("" : "+s"(hp));
            const int rowok = hp >= 0 && hp < H ? -1 : 0;  // (wave-uniform)
            const char* p = dn + (unsigned)(hp < 0 ? 0 : hp >= H ? H - 1 : hp) * (unsigned)W * 128u;
            c[0] = ldg16(p + ofs_c);
            c[1] = ldg16(p + ofs_c + 64);
            h[0] = h[1] = v4i{0, 0, 0, 0};
            if (edge) {
                h[0] = ldg16(p + ofs_h);
                h[1] = ldg16(p + ofs_h + 64);
            }
            return rowok;
        };
        auto shift_row = [&](int rowok) {                  // c, h -> cur[s]: the pixels w0 + m - 1 + s
            const int mc = rowok & ok_c, mh = rowok & ok_h;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                const v4i cc = c[kc] & v4i{mc, mc, mc, mc}, hh = h[kc] & v4i{mh, mh, mh, mh};
                cur[1][kc] = cc;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    cur[0][kc][i] = __builtin_amdgcn_update_dpp(hh[i], cc[i], 0x111, 0xf, 0xf, false);      // row_shr:1
                    cur[2][kc][i] = __builtin_amdgcn_update_dpp(hh[i], cc[i], 0x101, 0xf, 0xf, false);      // row_shl:1
                }
            }
        };
        shift_row(load_row(-1));
#pragma unroll
        for (int hi = -1; hi <= IG_ROWS; ++hi) {
            int nxt_ok = 0;
            if (hi < IG_ROWS) nxt_ok = load_row(hi + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int j = hi + 1 - r;
                    if (j < 0 || j >= IG_ROWS) continue;   // (compile time)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cur[s][0]),
                                                                     __builtin_bit_cast(bf16x8, bw[r * 3 + s][0]), acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cur[s][1]),
                                                                     __builtin_bit_cast(bf16x8, bw[r * 3 + s][1]), acc[j], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (hi < IG_ROWS) shift_row(nxt_ok);
        }
    }
    // D[row = 4q + i][col = m]: pixels w0 + 4q + 0..3 of channel m
    if (m >= creal) return;
    const int wq = w0 + q * 4;
    if (wq >= W) return;
    float* plane = dx + ((size_t)b * creal + m) * H * W;
    const bool vec = !(W & 3) && !((uintptr_t)dx & 15);    // then every (plane, row, wq) offset is a whole 16-byte vector
#pragma unroll
    for (int j = 0; j < IG_ROWS; ++j) {
        const int h = h0 + j;
        if (h >= H) break;
        float* o = plane + (size_t)h * W + wq;
        if (vec) {
            *reinterpret_cast<f32x4*>(o) = f32x4{acc[j][0] + bias, acc[j][1] + bias, acc[j][2] + bias, acc[j][3] + bias};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (wq + i < W) o[i] = acc[j][i] + bias;
        }
    }
}

// The parity form (f32 operands; also what defines the result for any T): one thread per pixel, the 16 channel sums in registers,
// the pack read through wave-uniform addresses.  Accumulation order per output element: expert, tap row, tap column, co.
template <typename T>
__global__ void __launch_bounds__(64) stem_input_grad_direct_kernel(const T* __restrict__ dz, const T* __restrict__ wd,
                                                                    const float* __restrict__ dgap, float* __restrict__ dx, int E,
                                                                    int B, int H, int W, int creal, int cinp2, int coutp2) {
    const int w = blockIdx.x * 64 + threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    if (w >= W) return;
    float acc[16], bias[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = bias[c] = 0.f;
    for (int e = 0; e < E; ++e) {
        const size_t n = (size_t)e * B + b;
        const T* wn = wd + n * cinp2 * 9 * (size_t)coutp2;
        if (dgap)
#pragma unroll
            for (int c = 0; c < 16; ++c) bias[c] += dgap[n * 16 + c];
        for (int r = 0; r < 3; ++r) {
            const int hp = h - 1 + r;
            if (hp < 0 || hp >= H) continue;
            for (int s = 0; s < 3; ++s) {
                const int wp = w - 1 + s;
                if (wp < 0 || wp >= W) continue;
                const T* p = dz + ((n * H + hp) * W + wp) * 64;
                const T* wt = wn + (r * 3 + s) * coutp2;
                for (int co = 0; co < 64; ++co) {
                    const float v = to_f32(p[co]);
#pragma unroll
                    for (int c = 0; c < 16; ++c) acc[c] = fmaf(v, to_f32(wt[(size_t)c * 9 * coutp2 + co]), acc[c]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < creal) dx[(((size_t)b * creal + c) * H + h) * W + w] = acc[c] + bias[c];
}

// ------------------------------------------------------------------------------------------------
// First Linear of speed_encoder / command_encoder (moe.py:55-56,88-89): its input [B][cin] is shared by the experts,
//   dx[b][j] = sum_e sum_o dh[e*B + b][dh_coff + o] * w[e][o][j]
// dh: T [E*B][dh_ld], the gradient of the layer's pre-activation output; w: the layer's forward pack T [E][coutp][cinp];
// dx: f32 [B][cin].  One thread per output element, experts then output features in order.
template <typename T>
__global__ void __launch_bounds__(256) shared_linear_input_grad_kernel(const T* __restrict__ dh, int dh_ld, int dh_coff,
                                                                       const T* __restrict__ w, float* __restrict__ dx, int E,
                                                                       int B, int cout, int coutp, int cinp, int cin) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * cin) return;
    const int b = i / cin, j = i % cin;
    float acc = 0.f;
    for (int e = 0; e < E; ++e) {
        const T* d = dh + ((size_t)e * B + b) * dh_ld + dh_coff;
        const T* we = w + (size_t)e * coutp * cinp + j;
        for (int o = 0; o < cout; ++o) acc = fmaf(to_f32(d[o]), to_f32(we[(size_t)o * cinp]), acc);
    }
    dx[i] = acc;
}

extern "C" {

int pmoe_stem_input_grad(const void* dz1, const void* wd, const float* dgap, float* dx, int32_t E, int32_t B, int32_t H,
                         int32_t W, int32_t creal, int32_t cinp2, int32_t coutp2, int32_t dtype, void* stream) {
    if (!dz1 || !wd || !dx || E < 1 || B < 1 || H < 1 || W < 1 || creal < 1 || creal > 16 || cinp2 < 16 || coutp2 < 64 || coutp2 % 8)
        return PMOE_ERR_ARG;
    if (((uintptr_t)dz1 | (uintptr_t)wd) & 15 || (uintptr_t)dx & 3 || B > 65535 || (long long)E * B > 0x7fffffffLL ||
        (long long)H * W * 256 > 0x7fffffffLL)                 // (byte offsets inside one image of dz1: 32 bits)
        return PMOE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PMOE_DT_BF16) {
        const int gx = (W + 63) / 64, gy = (H + IG_ROWS - 1) / IG_ROWS;
        if ((long long)gx * gy * B > 0x7fffffffLL) return PMOE_ERR_ARG;
        return launch<stem_input_grad_mfma_kernel, 0>(dim3((unsigned)(gx * gy * B)), dim3(256), 0, st, (const bf16*)dz1,
                                                      (const bf16*)wd, dgap, dx, E, B, H, W, creal, cinp2, coutp2, gx, gy);
    }
    if (dtype != PMOE_DT_F32 || H > 65535) return PMOE_ERR_ARG;
    return launch<stem_input_grad_direct_kernel<float>, 0>(dim3((W + 63) / 64, H, B), dim3(64), 0, st, (const float*)dz1,
                                                           (const float*)wd, dgap, dx, E, B, H, W, creal, cinp2, coutp2);
}

int pmoe_shared_linear_input_grad(const void* dh, int32_t dh_ld, int32_t dh_coff, const void* w, float* dx, int32_t E, int32_t B,
                                  int32_t cout, int32_t coutp, int32_t cinp, int32_t cin, int32_t dtype, void* stream) {
    if (!dh || !w || !dx || E < 1 || B < 1 || cout < 1 || cin < 1 || cin > cinp || cout > coutp || dh_coff < 0 ||
        dh_coff + cout > dh_ld || (long long)B * cin > 0x7fffffffLL)
        return PMOE_ERR_ARG;
    DISPATCH_DT(dtype, return launch<shared_linear_input_grad_kernel<T>, 0>(dim3(grid_for((long long)B * cin, 0x7fffffff)), dim3(256), 0,
                                                                            (hipStream_t)stream, (const T*)dh, dh_ld, dh_coff,
                                                                            (const T*)w, dx, E, B, cout, coutp, cinp, cin));
}

}  // extern "C"
