// Internal launcher interfaces shared by the .hip translation units and the C-ABI layer (api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pmoe_hip.h"

struct ConvArgs {
    const void* in;        // [Nin][H][W][in_ld] T ; channels [in_coff, in_coff+Cin) are reduced over
    const void* w;         // [E][CoutP][ks*ks][Cin] T
    void* out;             // [N][Ho][Wo][out_ld] T ; channels [out_coff, out_coff+Cout) are written
    const void* res;       // residual / saved activation, geometry of `out` with its own ld/coff
    const float* bias;     // [E][CoutP] f32 or null
    float* stats;          // [mblocks][2][CoutP] f32 partial (sum, sum of squares) or null
    const float* oscale;   // w_fp8: [E][CoutP] f32, accumulator scale = weight scale / in_scale
    float in_scale;        // w_fp8: activations are stored in LDS as e4m3(x * in_scale)
    int w_fp8;             // 1: `w` holds e4m3 bytes [E][CoutP][ks*ks][Cin]
    int in_fp8;            // 1: `in` holds e4m3 bytes too (e4m3(x * in_scale), written by pmoe_bn_apply's fp8 side output)
    int N, H, W, Cin;
    int Ho, Wo, Cout, CoutP;
    int in_ld, in_coff, out_ld, out_coff, res_ld, res_coff;
    int ipe;               // images per expert (N = E * ipe)
    int in_shared;         // 1: the input holds ipe images shared by all experts
    int ks, stride, pad, dilate;
    int act, res_mode;
    float drop_p;
    unsigned long long seed;
    // filled by the planner (conv_select)
    int lTW, lTH, TN, n_groups, tiles_y, tiles_x;
    // tap window + output lattice (defaults: kh = kw = ks, identity tap order, dense output).  A stride-2 data gradient
    // is issued as 4 launches, one per output parity class (py,px): a kh x kw = (1+py) x (1+px) stride-1 correlation over
    // dy whose taps are `tapmap` entries of the 3x3 filter, written to dx[2a+py][2b+px] (out_step 2).
    int kh, kw, use_tapmap, tapmap[4];
    int out_step, out_offy, out_offx, OH, OW;
    const float* bn;       // PMOE_RES_DBN: [4][N / bn_ipe][Cout] f32 (mean, invstd, scale, beta)
    int bn_ipe;
    int stagger;           // planner: waves 4-7 of the 8-wave tile run one k-substep behind their SIMD partners
    int prefetch;          // planner: 2 patch buffers, the next channel chunk's halo patch is fetched under the MFMAs
    int shuf_c;            // > 0 (1x1 direct kernel, round 4): ConvTranspose2d(k2,s2) scatter fused -- out is [N][2Ho][2Wo][out_ld], output
                           // channel q*shuf_c + c (q = 2 dy + dx) goes to pixel (2 oy + dy, 2 ox + dx), channel out_coff + c
};

struct WgradArgs {
    const void* x;         // conv input  [Nin][H][W][x_ld] T
    const void* dy;        // output grad [N][Ho][Wo][dy_ld] T
    float* dw;             // [E][taps][CoutP][CinP] f32, overwritten (every element is stored once; no atomics)
    float* part;           // K-split partial slabs [nsplit][E][taps][CoutP][CinP] f32 (conv_wgrad_ws_floats; may be null if 0)
    long long part_floats;
    int N, H, W, Cin, CinP;      // Cin: multiple of the channel chunk; CinP: row length of dw
    int Ho, Wo, Cout, CoutP;     // Cout: multiple of the channel chunk actually reduced
    int x_ld, x_coff, dy_ld, dy_coff;
    int ipe, x_shared;
    int ks, stride, pad;
    int per_image;         // 1: dw is [N][taps][CoutP][CinP] -- one slab per IMAGE (no sum over the expert's images)
    float* grads;          // optional: the parameter's own gradient [E][cout_real][cin_real][ks][ks] f32, written INSTEAD of dw
    int cout_real, cin_real;
    int defer_fold;        // 1: conv_wgrad_launch stops after the MFMA kernel (conv_wgrad_fold runs the tail)
    int lTW, lTH, TN, n_groups, tiles_y, tiles_x, mb_per_wg;
    int slice_fastest;     // grid order of round 1: always 0 (its switch is retired; the kernels still read the field)
};

// The piece decode of the LDS-DMA kernels divides by multiply-and-shift: patch pixel pp of PH rows x PW pixels per image lies in
// row (pp * mpw) >> 16, that row in image (row * mph) >> 16.  Sets mpw / mph; true if both are exact for every pp < n.
inline bool magic_div_exact(int n, int PW, int PH, int* mpw, int* mph) {
    *mpw = 65536 / PW + 1; *mph = 65536 / PH + 1;
    for (int pp = 0; pp < n; ++pp)
        if (((pp * *mpw) >> 16) != pp / PW || (((pp / PW) * *mph) >> 16) != (pp / PW) / PH) return false;
    return true;
}

// ceil(log2(v)): the smallest l with 2^l >= v
inline int ceil_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// The pixel tile of the conv and weight-gradient kernels: a block of 2^lBM output pixels cut as TN images x 2^lTH rows x 2^lTW
// pixels -- rows as wide as the map needs (at most 2^ltw_max), then as many rows as it needs, the rest of the block over images --
// and how many of them cover one expert's ipe maps of Ho x Wo pixels.
struct PixelTile {
    int lTW, lTH, TN, n_groups, tiles_y, tiles_x;
    int per_expert() const { return n_groups * tiles_y * tiles_x; }
};
inline PixelTile pixel_tile(int Ho, int Wo, int ipe, int lBM, int ltw_max) {
    PixelTile t;
    t.lTW = ceil_log2(Wo) > ltw_max ? ltw_max : ceil_log2(Wo);
    t.lTH = ceil_log2(Ho) > lBM - t.lTW ? lBM - t.lTW : ceil_log2(Ho);
    t.TN = (1 << lBM) >> (t.lTW + t.lTH);
    t.n_groups = (ipe + t.TN - 1) / t.TN;
    t.tiles_y = (Ho + (1 << t.lTH) - 1) >> t.lTH;
    t.tiles_x = (Wo + (1 << t.lTW) - 1) >> t.lTW;
    return t;
}
// input pixels under 2^l output pixels along one axis (the halo patch is patch_extent(lTW, ..) x patch_extent(lTH, ..) per image)
inline int patch_extent(int l, int k, int stride) { return ((1 << l) - 1) * stride + k; }
template <typename Args> inline void set_tile(Args& a, const PixelTile& t) {      // ConvArgs | WgradArgs
    a.lTW = t.lTW; a.lTH = t.lTH; a.TN = t.TN; a.n_groups = t.n_groups; a.tiles_y = t.tiles_y; a.tiles_x = t.tiles_x;
}

// resident-weight ping-pong kernel and its LDS-DMA successors for the <=64-channel 3x3 stride-1 layers (conv_res.hip): what the
// tile fields of ConvLaunch.a do not say
struct ResPlan {
    int tiles_per_expert, wgs_per_expert, log_rb;
    size_t smem;
};

// the kernel families a conv launch can run on
enum ConvKind { CONV_SKINNY = 1, CONV_C16, CONV_C1X1, CONV_RES, CONV_DMA, CONV_DMA_S2, CONV_DMA_S2CLS, CONV_DMA_F8, CONV_TILE };

// One kernel launch as conv_select decided it: the family, the descriptor the kernel receives (tile fields filled in) and what
// that family's launcher needs to pick the instantiation and its grid.  Filled by the family's planner, read by its launcher.
struct ConvLaunch {
    int kind;              // ConvKind
    int code;              // pmoe_conv2d_plan code of this launch (include/pmoe_hip.h)
    int mblocks;           // m-blocks = statistics rows this launch writes
    ConvArgs a;
    size_t smem;           // dynamic LDS bytes of the launch (RES: of the LDS-DMA variants; the ping-pong kernel's are res.smem)
    int pbuf, mpw, mph;    // LDS-DMA (+ RES with res_dma): patch buffer bytes, magic numbers of the piece decode
    int mf16, stream, producer, narrow;        // DMA: conv3x3_dma_kernel<MF16, PROD> | conv3x3_dma_stream_kernel<MF16, NARROW>
    ResPlan res;           // RES
    int res_dma, res_pipe;                     // RES: conv3x3_resdma_kernel, conv3x3_respipe_kernel<BIAS, MODE>
    int wpe, tpe, tiles_x, slabs, mt;           // C16 / C1X1: workgroups and tiles per expert, (C16) tiles per row, (C1X1) slabs, MT
    int log_rb, wm, wn, lite;                   // TILE: conv_igemm_kernel<T, LOG_RB, WM, WN> | conv_igemm_lite_kernel<T, LOG_RB>
};

// what conv_select decided for a descriptor: up to four launches (a stride-2 data gradient: one per output parity class)
struct ConvPlan {
    int code;              // pmoe_conv2d_plan code, or a PMOE_ERR_* (< 0): nothing runs
    int mblocks;           // statistics rows (pmoe_conv2d_stat_rows)
    int n;
    ConvLaunch l[4];
};
int conv_select(const ConvArgs& a, int dtype, ConvPlan* p);

// the family planners (false / no launch: the family does not serve this descriptor) and launchers
bool gemm_skinny_plan(const ConvArgs& a, int dtype, ConvLaunch* l);          // gemm_skinny.hip: the expert MLP layers
int gemm_skinny_launch(const ConvLaunch& l, hipStream_t st);
bool conv_c16_plan(const ConvArgs& a, int dtype, ConvLaunch* l);             // conv_c16.hip: the 16-channel stem conv
int conv_c16_launch(const ConvLaunch& l, hipStream_t st);
bool conv_c1x1_plan(const ConvArgs& a, int dtype, ConvLaunch* l);            // conv_c1x1.hip: 1x1 direct kernel
int conv_c1x1_launch(const ConvLaunch& l, hipStream_t st);
bool conv_res_plan(const ConvArgs& a, int dtype, ConvLaunch* l);             // conv_res.hip (l->res_dma / res_pipe: which kernel)
int conv_res_launch(const ConvLaunch& l, hipStream_t st);
// LDS-DMA 3x3 kernels (conv_dma.hip): stride 1 (>= 128 output channels, or the 64-channel streaming tile), the block-scaled fp8
// one (e4m3 weights and activations), the stride-2 forward one, and one parity class of a stride-2 data gradient on the same
// kernel (ConvArgs with the class fields set).  One launcher serves all four.
bool conv_dma_plan(const ConvArgs& a, int dtype, ConvLaunch* l);
bool conv_dma_f8_plan(const ConvArgs& a, int dtype, ConvLaunch* l);
bool conv_dma_s2_plan(const ConvArgs& a, int dtype, ConvLaunch* l);
bool conv_dma_s2cls_plan(const ConvArgs& a, int dtype, ConvLaunch* l);
int conv_dma_launch(const ConvLaunch& l, hipStream_t st);

int conv_igemm_launch(const ConvArgs& a, int dtype, hipStream_t st);
int conv_igemm_mblocks(const ConvArgs& a, int dtype);
int conv_igemm_plan(const ConvArgs& a, int dtype);

// the kernel families a weight-gradient launch can run on
enum WgradKind { WGRAD_TILE = 1, WGRAD_DMA, WGRAD_DMA2, WGRAD_BNBWD };

// pmoe_wgrad_desc.bn_fused: the per-image filter gradient with the BatchNorm backward applied on load (conv_wgrad_bnbwd_kernel,
// round 4).  `fused` and `z_ld` take part in the selection; the pointers are read by the launch only.
struct WgradBn {
    int fused, z_ld;
    const void* z;
    const float *coef, *c1, *c2;
};

// What wgrad_select decided for a descriptor: the family, the descriptor the kernel receives (tile fields, mb_per_wg and
// slice_fastest filled in) and what that family's launcher needs to pick the instantiation.  The launch, the deferred fold, the plan
// code and the workspace size all read this one plan.
struct WgradPlan {
    int kind;              // WgradKind
    int code;              // pmoe_conv2d_wgrad_plan code, or a PMOE_ERR_* (< 0): nothing runs
    WgradArgs a;
    int esz, maxv;         // TILE: conv_wgrad_kernel<T, taps, MAXV> (esz = sizeof(T))
    int pin, wci, pairs, req;      // DMA: conv_wgrad_dma_kernel<PIN, WCI, PAIRS, REQ> (DMA2: conv_wgrad_dma2_kernel<a.lTW>)
    dim3 grid, block;
    size_t smem;           // dynamic LDS bytes of the launch
    int mpw, mph;          // DMA / DMA2: magic numbers of the piece decode
    int E, taps, nsplit;   // experts, filter taps, K-split slabs the launch writes (the fold sums them)
    long long ws_floats;   // pmoe_conv2d_wgrad_ws_floats: nsplit slabs, 0 if the launch writes dw itself
};
int wgrad_select(const WgradArgs& a, int dtype, const WgradBn& bn, WgradPlan* p);      // -> p->code

int conv_wgrad_launch(const WgradArgs& a, int dtype, const WgradBn& bn, hipStream_t st);
int conv_wgrad_fold(const WgradArgs& a, int dtype, const WgradBn& bn, hipStream_t st);
long long conv_wgrad_ws_floats(const WgradArgs& a, int dtype, const WgradBn& bn);
int conv_wgrad_plan(const WgradArgs& a, int dtype, const WgradBn& bn);
