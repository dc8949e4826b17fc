// Prints what conv_select and wgrad_select decide over a sweep of descriptors: every non-pointer field of each ConvLaunch and
// WgradPlan by name (zero fields are left out; the tile fields come from the descriptor the kernel receives, `.a`).  A plain host
// program: build it against the library,
//   hipcc --offload-arch=gfx950 -std=c++17 tools/dump_plans.cpp -Lpmoe_amd -lpmoe_hip -Wl,-rpath,$PWD/pmoe_amd -o build/dump_plans
// and compare its output with tests/golden/conv_plans.txt (tests/test_abi.py does).  Per switch setting only the rows whose
// answer differs from the default one are printed.  No launch, no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../pmoe_amd/csrc/kernels.h"

static float dummy[4];
static std::string out;
static void kv(const char* name, long long v) { if (v) out += std::string(" ") + name + "=" + std::to_string(v); }
#define F(s, f) kv(#f, (long long)(s).f)

struct ConvRow { std::string name; ConvArgs a; int dtype; };
struct WgradRow { std::string name; WgradArgs a; int dtype; WgradBn bn; };

static bool keep(unsigned i, unsigned every) { return ((i * 2654435761u) >> 16) % every == 0; }

// a forward conv (or, dilate: the data gradient of a stride-2 one, output map twice the input) as api.hip's to_plan_args builds it
static ConvArgs conv(int E, int ipe, int cin, int cout, int H, int W, int ks, int stride, bool dilate = false) {
    ConvArgs a{};
    const int pad = ks / 2;
    a.in = a.w = dummy; a.out = dummy + 1;
    a.N = E * ipe; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.CoutP = (cout + 63) / 64 * 64;
    a.Ho = dilate ? 2 * H : (H + 2 * pad - ks) / stride + 1; a.Wo = dilate ? 2 * W : (W + 2 * pad - ks) / stride + 1;
    a.in_ld = cin; a.out_ld = cout; a.ipe = a.bn_ipe = ipe; a.ks = a.kh = a.kw = ks; a.stride = dilate ? 1 : stride; a.pad = pad; a.dilate = dilate;
    a.out_step = 1; a.OH = a.Ho; a.OW = a.Wo;
    return a;
}

static std::string conv_name(const ConvArgs& a, int dtype) {
    char b[256];
    snprintf(b, sizeof b, "dt%d N%d ipe%d %dx%d c%d>%d(%d) k%d s%d d%d ld%d,%d sh%d b%d st%d a%d r%d p%d bn%d f8%d%d sc%d", dtype, a.N, a.ipe, a.H, a.W, a.Cin,
             a.Cout, a.CoutP, a.ks, a.stride, a.dilate, a.in_ld, a.out_ld, a.in_shared, !!a.bias, !!a.stats, a.act, a.res_mode,
             a.drop_p > 0.f, !!a.bn, a.w_fp8, a.in_fp8, a.shuf_c);
    return b;
}

static std::vector<ConvRow> conv_rows() {
    std::vector<ConvRow> rows;
    auto add = [&rows](const ConvArgs& a, int dtype) { rows.push_back({conv_name(a, dtype), a, dtype}); };
    // 1. the general cross, sampled: dtypes x forms (3x3 / 1x1, both strides, the two stride-2 data gradients) x maps x channels
    //    x images per expert x experts x epilogues
    const int maps[][2] = {{1, 1}, {4, 4}, {8, 8}, {16, 16}, {32, 32}, {64, 64}, {128, 128}, {256, 256}, {40, 24}, {71, 55}, {13, 9}};
    const int cins[] = {16, 64, 128, 256, 512}, couts[] = {64, 128, 256}, ipes[] = {1, 2, 5, 64}, Es[] = {1, 4};
    unsigned i = 0;
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int form = 0; form < 6; ++form)
            for (auto& m : maps)
                for (int cin : cins)
                    for (int cout : couts)
                        for (int ipe : ipes)
                            for (int E : Es)
                                for (int epi = 0; epi < 4; ++epi) {
                                    if (!keep(i++, 500)) continue;
                                    const int ks = form == 2 || form == 3 || form == 5 ? 1 : 3, stride = form == 1 || form == 3 ? 2 : 1;
                                    ConvArgs a = conv(E, ipe, cin, cout, m[0], m[1], ks, stride, form >= 4);
                                    if (epi == 1) { a.bias = dummy; a.act = PMOE_ACT_RELU; }
                                    if (epi == 2) { a.res = dummy + 2; a.res_ld = cout; a.res_mode = PMOE_RES_ADD; a.stats = dummy; }
                                    if (epi == 3) a.stats = dummy;
                                    if (form == 5) { a.res = a.out; a.res_ld = a.out_ld; a.res_mode = PMOE_RES_ADD; a.bias = nullptr; a.act = 0; }
                                    add(a, dtype);
                                }
    // 2. the fused requests (tests/test_fused_contract_cpu.py's grid), sampled
    i = 0;
    for (int req = 0; req < 6; ++req)
        for (int c : {16, 64, 128, 256, 512})
            for (int side : {8, 16, 32, 64, 128})
                for (int ipe : {1, 2, 64})
                    for (int bs = 0; bs < 4; ++bs) {
                        if (!keep(i++, 24)) continue;
                        const bool shuf = req == 3 || req == 4, inbn = req == 0 || req == 1 || req == 4;
                        ConvArgs a = conv(2, ipe, c, c, side, side, req == 0 || req == 2 || req == 5 ? 3 : 1, 1);
                        if (shuf) { a.shuf_c = c / 4; a.out_ld = 2 * a.shuf_c; a.out_coff = a.shuf_c; }
                        if (bs & 1) a.bias = dummy;
                        if (bs & 2) a.stats = dummy;
                        if (inbn) { a.res_mode = PMOE_RES_INBN; a.bn = dummy; }
                        if (req == 2) { a.res_mode = PMOE_RES_DBN; a.res = dummy + 2; a.res_ld = c; a.bn = dummy; }
                        if (req == 5) { a.w_fp8 = a.in_fp8 = 1; a.in_scale = 1.f; a.oscale = dummy; }
                        add(a, 0);
                    }
    // 3. the instantiations tests/test_abi.py names, the expert MLP layers, the stem on a shared input, e4m3 weights
    const int named[][8] = {{4, 64, 64, 64, 128, 3, 1, 0},  {4, 64, 16, 64, 256, 3, 1, 0}, {4, 64, 256, 256, 32, 3, 1, 0}, {4, 64, 128, 128, 64, 3, 1, 0},
                            {4, 64, 128, 256, 64, 1, 2, 0}, {4, 64, 256, 512, 32, 1, 2, 0}, {4, 64, 1536, 512, 1, 1, 1, 0}, {4, 256, 512, 1536, 1, 1, 1, 0},
                            {3, 1, 512, 512, 14, 3, 1, 0},  {3, 1, 128, 128, 56, 3, 1, 0}, {3, 1, 128, 128, 64, 3, 1, 0}, {4, 64, 128, 64, 64, 3, 1, 1},
                            {4, 64, 256, 128, 32, 3, 1, 1}, {4, 64, 64, 128, 128, 3, 2, 0}, {1, 1, 64, 64, 64, 3, 1, 0}, {4, 64, 512, 512, 16, 3, 1, 0},
                            {4, 64, 128, 64, 64, 3, 1, 0}};
    for (auto& n : named)
        for (int dtype = 0; dtype < 2; ++dtype) {
            ConvArgs a = conv(n[0], n[1], n[2], n[3], n[4], n[4], n[5], n[6], n[7]);
            add(a, dtype);
            if (!dtype && !n[7] && n[5] == 3 && n[6] == 1) {
                ConvArgs b = a; b.bias = dummy; b.res = dummy + 2; b.res_ld = b.Cout; b.res_mode = PMOE_RES_ADD; add(b, 0);
                ConvArgs f = a; f.w_fp8 = 1; f.in_scale = 1.f; f.oscale = dummy; add(f, 0);
            }
        }
    for (int E : {1, 4, 8}) {
        ConvArgs a = conv(E, E == 1 ? 1 : 64, 16, 64, 256, 256, 3, 1);
        a.in_shared = 1; add(a, 0);
        a.out_ld = 1024; add(a, 0);                     // a window of a wide buffer: past 32-bit offsets at E = 8
    }
    { ConvArgs a = conv(4, 64, 64, 64, 32, 32, 5, 1); add(a, 0); }      // PMOE_ERR_ARG: no 5x5 kernel
    return rows;
}

static WgradRow wgrad(int dtype, int E, int ipe, int cin, int cout, int H, int W, int ks, int stride, int per_image, int fused) {
    const int pad = ks / 2, ckw = dtype ? 32 : 64;
    WgradArgs a{};
    a.x = a.dy = dummy; a.dw = dummy + 1;
    a.N = E * ipe; a.H = H; a.W = W; a.Cin = cin; a.CinP = (cin + ckw - 1) / ckw * ckw;
    a.Ho = (H + 2 * pad - ks) / stride + 1; a.Wo = (W + 2 * pad - ks) / stride + 1;
    a.Cout = cout; a.CoutP = (cout + ckw - 1) / ckw * ckw;
    a.x_ld = cin; a.dy_ld = cout; a.ipe = ipe; a.ks = ks; a.stride = stride; a.pad = pad; a.per_image = per_image;
    char b[160];
    snprintf(b, sizeof b, "dt%d N%d ipe%d %dx%d c%d>%d k%d s%d pi%d bn%d", dtype, a.N, ipe, H, W, cin, cout, ks, stride, per_image, fused);
    return {b, a, dtype, WgradBn{fused, cout, dummy, dummy, dummy, dummy}};
}

static std::vector<WgradRow> wgrad_rows() {
    std::vector<WgradRow> rows;
    // 1. tests/test_abi.py's _wgrad_sweep_descriptors cross, sampled more thinly
    const int forms[][2] = {{1, 1}, {1, 2}, {3, 1}, {3, 2}};
    const int maps[][2] = {{4, 4}, {8, 8}, {16, 16}, {32, 32}, {64, 64}, {128, 128}, {256, 256}, {40, 24}, {71, 55}, {13, 9}, {7, 10}, {256, 8}, {200, 6}, {32, 8}};
    unsigned i = 0;
    for (int dtype = 0; dtype < 2; ++dtype)
        for (auto& f : forms)
            for (auto& m : maps)
                for (int cin : {16, 32, 64, 128, 256, 512})
                    for (int ipe : {1, 2, 5, 64, 512})
                        for (int E : {1, 4})
                            for (int per_image = 0; per_image < 2; ++per_image)
                                for (int fused = 0; fused < 2; ++fused)
                                    if (keep(i++, 160)) rows.push_back(wgrad(dtype, E, ipe, cin, cin > 64 ? cin : 64, m[0], m[1], f[0], f[1], per_image, fused));
    // 2. the smallest shape of each launcher branch (tests/test_ops_gpu.py's WGRAD_BRANCH_CASES), the request-mode shapes, the
    //    layers tests/test_abi.py names, the BatchNorm-fused stem (tests/test_fused_contract_cpu.py's grid, sampled)
    const int named[][8] = {{0, 1, 2, 64, 64, 32, 32, 3},   {0, 1, 2, 64, 64, 16, 16, 3},   {0, 1, 2, 64, 64, 32, 8, 3},  {0, 1, 2, 16, 64, 32, 32, 3},
                            {0, 1, 2, 32, 64, 32, 32, 3},   {0, 1, 2, 64, 128, 32, 32, 1},  {1, 1, 2, 64, 64, 32, 32, 3}, {0, 2, 2, 64, 64, 128, 128, 3},
                            {0, 1, 5, 128, 256, 40, 24, 3}, {0, 2, 3, 256, 128, 16, 16, 3}, {0, 4, 64, 64, 64, 128, 128, 3}, {0, 4, 64, 256, 256, 32, 32, 3},
                            {0, 4, 64, 16, 64, 256, 256, 3}, {0, 1, 600, 64, 64, 16, 16, 3}};
    for (auto& n : named) rows.push_back(wgrad(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], 1, 0, 0));
    rows.push_back(wgrad(0, 1, 2, 64, 128, 32, 32, 3, 2, 0, 0));
    rows.push_back(wgrad(0, 4, 64, 64, 128, 128, 128, 3, 2, 0, 0));
    rows.push_back(wgrad(0, 2, 2, 64, 64, 32, 32, 3, 1, 1, 0));
    rows.back().a.CinP = 128; rows.back().name += " cinp128";           // PMOE_ERR_ARG: the tiles would not cover dw exactly
    i = 0;
    for (int c : {16, 64, 128, 256, 512})
        for (int side : {8, 16, 32, 64, 128})
            for (int ipe : {1, 2, 64})
                for (int which = 0; which < 2; ++which)
                    if (keep(i++, 6)) rows.push_back(wgrad(0, 2, ipe, which ? c : 16, which ? 64 : c, side, side, 3, 1, 1, 1));
    return rows;
}

static std::string conv_answer(const ConvRow& r) {
    ConvPlan p;
    conv_select(r.a, r.dtype, &p);
    out.clear();
    F(p, code); F(p, mblocks); F(p, n);
    for (int k = 0; k < p.n; ++k) {
        const ConvLaunch& l = p.l[k];
        out += " |";
        F(l, kind); F(l, code); F(l, mblocks);
        F(l, a.lTW); F(l, a.lTH); F(l, a.TN); F(l, a.n_groups); F(l, a.tiles_y); F(l, a.tiles_x); F(l, a.stagger); F(l, a.prefetch);
        if (l.a.out_step != r.a.out_step) {              // a parity class of a stride-2 data gradient: the rewritten descriptor
            F(l, a.Ho); F(l, a.Wo); F(l, a.stride); F(l, a.pad); F(l, a.dilate); F(l, a.kh); F(l, a.kw); F(l, a.use_tapmap);
            F(l, a.tapmap[0]); F(l, a.tapmap[1]); F(l, a.tapmap[2]); F(l, a.tapmap[3]);
            F(l, a.out_step); F(l, a.out_offy); F(l, a.out_offx); F(l, a.OH); F(l, a.OW);
        }
        F(l, smem); F(l, pbuf); F(l, mpw); F(l, mph); F(l, mf16); F(l, stream); F(l, producer); F(l, narrow);
        F(l, res.tiles_per_expert); F(l, res.wgs_per_expert); F(l, res.log_rb); F(l, res.smem); F(l, res_dma); F(l, res_pipe);
        F(l, wpe); F(l, tpe); F(l, tiles_x); F(l, slabs); F(l, mt); F(l, log_rb); F(l, wm); F(l, wn); F(l, lite);
    }
    return out;
}

static std::string wgrad_answer(const WgradRow& r) {
    WgradPlan p;
    wgrad_select(r.a, r.dtype, r.bn, &p);
    out.clear();
    F(p, kind); F(p, code);
    if (p.code < 0) return out;                         // refused: nothing else is read
    F(p, a.lTW); F(p, a.lTH); F(p, a.TN); F(p, a.n_groups); F(p, a.tiles_y); F(p, a.tiles_x); F(p, a.mb_per_wg); F(p, a.slice_fastest);
    F(p, esz); F(p, maxv); F(p, pin); F(p, wci); F(p, pairs); F(p, req);
    F(p, grid.x); F(p, grid.y); F(p, grid.z); F(p, block.x); F(p, block.y); F(p, block.z);
    F(p, smem); F(p, mpw); F(p, mph); F(p, E); F(p, taps); F(p, nsplit); F(p, ws_floats);
    return out;
}

template <typename Row, typename Fn> static void sweep(const char* tag, const std::vector<Row>& rows, const std::vector<const char*>& envs, Fn answer) {
    std::vector<std::string> base;
    for (const char* env : envs) {                      // "" (the defaults) first, then "NAME=value[ NAME=value]"
        std::vector<std::string> names;
        for (std::string s = env; !s.empty();) {
            const size_t sp = s.find(' '), eq = s.find('=');
            names.push_back(s.substr(0, eq));
            setenv(names.back().c_str(), s.substr(eq + 1, sp == std::string::npos ? sp : sp - eq - 1).c_str(), 1);
            s = sp == std::string::npos ? "" : s.substr(sp + 1);
        }
        for (size_t i = 0; i < rows.size(); ++i) {
            const std::string got = answer(rows[i]);
            if (!*env) { base.push_back(got); printf("%s %zu [%s]%s\n", tag, i, rows[i].name.c_str(), got.c_str()); }
            else if (got != base[i]) printf("%s %zu {%s}%s\n", tag, i, env, got.c_str());
        }
        for (auto& n : names) unsetenv(n.c_str());
    }
}

int main() {
    // every switch the planners read, at every value some test sets (and the combinations tests/test_ops_gpu.py sets together)
    sweep("conv", conv_rows(),
          {"", "PMOE_CONV_C16=0", "PMOE_CONV_C1X1=0", "PMOE_CONV_DMA=0", "PMOE_CONV_F8DMA=0", "PMOE_DMA_NARROW=0", "PMOE_DMA_STREAM=0",
           "PMOE_DMA_STREAM=2", "PMOE_DMA_MF16=0", "PMOE_DMA_MF16=1", "PMOE_DMA_PRODUCER=0", "PMOE_DMA_PRODUCER=2",
           "PMOE_DMA_MF16=1 PMOE_DMA_STREAM=0 PMOE_DMA_PRODUCER=2", "PMOE_DMA_PRODUCER=0 PMOE_DMA_STREAM=0", "PMOE_RES_DMA=0",
           "PMOE_RES_PIPE=0", "PMOE_RES_DMA=0 PMOE_CONV_C16=0"},
          conv_answer);
    sweep("wgrad", wgrad_rows(),
          {"", "PMOE_WGRAD_DMA=0", "PMOE_WGRAD_V2=0", "PMOE_WGRAD_NARROW=0", "PMOE_WGRAD_PIPE=0", "PMOE_WGRAD_REQ=0", "PMOE_WGRAD_REQ=2"},
          wgrad_answer);
    return 0;
}
