"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads and exports every symbol
include/pmoe_hip.h declares, with the argument counts the ctypes binding uses (no compute calls)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from pmoe_amd import hip

REPO = Path(__file__).resolve().parents[1]
HEADER = (REPO / "include" / "pmoe_hip.h").read_text()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    text = re.sub(r"typedef struct.*?\}\s*\w+;", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"(?:int|int64_t|const char\*)\s+(pmoe_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        n = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
        out[m.group(1)] = n
    return out


@pytest.fixture(scope="module")
def lib():
    if not hip.lib_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def test_header_declares_the_bound_symbols():
    decl = _declared()
    assert set(decl) == set(hip.SIGNATURES), set(decl) ^ set(hip.SIGNATURES)
    for name, n in decl.items():
        assert len(hip.SIGNATURES[name]) == n, (name, n, len(hip.SIGNATURES[name]))


def test_library_exports_every_symbol(lib):
    for name in _declared():
        assert hasattr(lib, name), name
    assert lib.pmoe_version() == hip.ABI_VERSION == 401
    assert b"invalid" in lib.pmoe_error_string(-1)


def test_struct_layouts_match_c(lib):
    # sizes computed by hand from include/pmoe_hip.h (LP64): 6 pointers + 22 int32 + float + pad + u64 + 2 int32 + float +
    # pad + pointer + int32 + pad + pointer + int32 + pad
    assert ctypes.sizeof(hip.ConvDesc) == 200 == lib.pmoe_abi_sizeof(0)
    assert ctypes.sizeof(hip.WgradDesc) == lib.pmoe_abi_sizeof(1)
    # int32 block padded to 8, part_ws + its size, grads + 3 int32 + bn_fused, 4 bn_* pointers, bn_z_ld (+ pad)   (round 4: 144 -> 184)
    assert ctypes.sizeof(hip.WgradDesc) == 3 * 8 + 19 * 4 + 4 + 2 * 8 + 8 + 4 * 4 + 4 * 8 + 4 + 4 == 184
    from pmoe_amd import optim
    assert ctypes.sizeof(optim.OptTensor) == 64 == lib.pmoe_abi_sizeof(2)
    assert optim.CHUNK == 16384          # PMOE_OPT_CHUNK


def test_no_cpu_fallback(lib):
    import torch
    from pmoe_amd import ops
    x = torch.zeros(1, 4, 4, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.maxpool_fwd(x, torch.zeros(1, 2, 2, 16), torch.zeros(1, 2, 2, 16, dtype=torch.uint8))


def test_conv_plan_reports_the_kernel_instantiation():
    """pmoe_conv2d_plan (bench.py uses it to attribute launch times to rocprof kernel symbols)."""
    import ctypes as C
    from pmoe_amd.hip import ConvDesc, load

    def plan(cin, cout, H, ks, stride, dtype, B=64, E=4, dilate=False, Hout=None):
        d = ConvDesc()
        pad = ks // 2
        Ho = Hout or (H + 2 * pad - ks) // stride + 1
        d.n, d.h, d.w_, d.cin, d.ho, d.wo, d.cout, d.coutp = E * B, H, H, cin, Ho, Ho, cout, (cout + 63) // 64 * 64
        d.in_ld, d.out_ld, d.ipe, d.ks, d.stride, d.pad, d.dilate = cin, cout, B, ks, stride, pad, int(dilate)
        d.dtype = 0 if dtype == torch.bfloat16 else 1
        return load().pmoe_conv2d_plan(C.byref(d))
    assert plan(64, 64, 128, 3, 1, torch.bfloat16) == 1207                 # conv3x3_respipe_kernel<false, 0> (filter bank resident, LDS-DMA patches)
    assert plan(16, 64, 256, 3, 1, torch.bfloat16) == 1316                 # 12(16)-channel stem: conv3x3_c16_kernel (direct form)
    assert plan(256, 256, 32, 3, 1, torch.bfloat16) == 5057                # conv3x3_dma_stream_kernel<true> (LDS-DMA staged, 16x16x32 MFMA shape from 256 input channels, persistent + producer wave)
    assert plan(128, 128, 64, 3, 1, torch.bfloat16) == 5047                # conv3x3_dma_stream_kernel<false> (32x32x16)
    assert plan(128, 256, 64, 1, 2, torch.bfloat16) == 1404                # 1x1 stride 2 (downsample): conv1x1_direct_kernel<4>
    assert plan(256, 512, 32, 1, 2, torch.bfloat16) == 1402                # ... 64-channel slabs from 256 input channels
    assert plan(256, 256, 32, 3, 1, torch.float32) == 722                  # f32: 4-wave 128x128 tile, 32-channel chunks
    assert plan(1536, 512, 1, 1, 1, torch.bfloat16) == 3000                # expert MLP GEMM: gemm_skinny_kernel
    assert plan(1536, 512, 1, 1, 1, torch.float32) == 722                  # ... in f32: generic 4-wave tile
    assert plan(512, 512, 14, 3, 1, torch.bfloat16, B=1, E=3) == 3000      # B=1 inference layer4: tap-looping skinny kernel
    assert plan(128, 128, 56, 3, 1, torch.bfloat16, B=1, E=3) == 3000      # ... layer2 (3136 pixels per expert <= 3200)
    assert plan(128, 128, 64, 3, 1, torch.bfloat16, B=1, E=3) == 5047      # 4096 pixels per expert: the LDS-DMA tile
    assert plan(128, 64, 64, 3, 1, torch.bfloat16, dilate=True, Hout=128) == 4741   # stride-2 dgrad, 64 gradient rows: 4 class launches <7,4,1>
    assert plan(256, 128, 32, 3, 1, torch.bfloat16, dilate=True, Hout=64) == 9207   # ... >= 128 rows: 4 class launches of conv3x3s2_dma_kernel<true>
    assert plan(64, 128, 128, 3, 2, torch.bfloat16) == 5207                # stride-2 forward: conv3x3s2_dma_kernel<false>
    assert plan(128, 64, 64, 3, 1, torch.float32, dilate=True, Hout=128) // 1000 == 4   # ... in f32: 4 class launches of the generic kernel


def test_planning_calls_see_the_same_descriptor_as_the_launch():
    """The kernel choice can depend on the row lengths (32-bit offset ranges): a planning descriptor that leaves them 0 means
    DENSE rows, and must agree with the one the launch gets -- at E=8, B=64 (BASELINE config 3's shard) the 16-channel stem
    convolution once sized its BatchNorm partial-sum buffer for a different kernel than the one that ran."""
    import ctypes as C
    from pmoe_amd.hip import ConvDesc, load

    def desc(E, B, cin, cout, H, in_ld, out_ld):
        d = ConvDesc()
        d.n, d.h, d.w_, d.cin, d.ho, d.wo, d.cout, d.coutp = E * B, H, H, cin, H, H, cout, 64
        d.in_ld, d.out_ld, d.ipe, d.ks, d.stride, d.pad, d.dtype, d.in_shared = in_ld, out_ld, B, 3, 1, 1, 0, 1
        return d
    for E, B in ((4, 64), (8, 64), (1, 1)):
        a, b = desc(E, B, 16, 64, 256, 0, 0), desc(E, B, 16, 64, 256, 16, 64)
        assert load().pmoe_conv2d_plan(C.byref(a)) == load().pmoe_conv2d_plan(C.byref(b)) == 1316
        assert load().pmoe_conv2d_stat_rows(C.byref(a)) == load().pmoe_conv2d_stat_rows(C.byref(b)) > 0
    # rows 16x as long (a window of a wide buffer): one expert's images no longer fit 32-bit offsets -> another kernel, and the
    # planning call says so
    wide = desc(8, 64, 16, 64, 256, 16, 1024)
    assert load().pmoe_conv2d_plan(C.byref(wide)) == 1005


def _plan_and_rows(d):
    import ctypes as C
    from pmoe_amd.hip import load
    return load().pmoe_conv2d_plan(C.byref(d)), load().pmoe_conv2d_stat_rows(C.byref(d))


def test_shuffle_c_runs_on_the_1x1_direct_kernel_or_nothing():
    """pmoe_conv_desc.shuffle_c: the scatter exists in conv1x1_direct_kernel only -- with e4m3 operands, a dilated source or a 3x3
    filter nothing serves the descriptor (the plan once reported the e4m3 tile, which would have ignored the scatter), and a
    launch that writes statistics never takes it."""
    from pmoe_amd import hip
    from pmoe_amd.hip import ConvDesc

    def desc(ks=1, w_fp8=0, in_fp8=0, dilate=0):
        d = ConvDesc()
        c = 32
        d.n, d.h, d.w_, d.cin, d.ho, d.wo, d.cout, d.coutp = 4, 64, 64, 64, 64, 64, 4 * c, 128
        d.in_ld, d.out_ld, d.out_coff, d.ipe, d.ks, d.stride, d.pad, d.dilate = 64, 2 * c, c, 4, ks, 1, ks // 2, dilate
        d.shuffle_c, d.w_fp8, d.in_fp8, d.in_scale, d.out_scale = c, w_fp8, in_fp8, 1.0, 1
        return d
    plan, rows = _plan_and_rows(desc())
    assert plan in (1452, 1454) and rows == hip.ERR_UNSUPPORTED
    for d in (desc(w_fp8=1), desc(w_fp8=1, in_fp8=1), desc(dilate=1), desc(ks=3)):
        assert _plan_and_rows(d) == (hip.ERR_UNSUPPORTED, hip.ERR_UNSUPPORTED)


def test_stride2_1x1_inplace_data_gradient_plans_its_single_launch():
    """The stride-2 1x1 data gradient accumulated in place (res == out, PMOE_RES_ADD) runs ONE class-(0,0) launch of the generic
    tile over the even-even pixels: the plan and the statistics rows are that launch's -- those of a stride-1 1x1 conv over the
    half-size map -- not a zero-dilated tile that never runs, and not the 4000 + code of four class launches."""
    from pmoe_amd.hip import ConvDesc

    def desc(cin, cout, H, dtype, dilate, inplace=True, E=4, B=64):
        d = ConvDesc()
        Ho = 2 * H if dilate else H
        d.n, d.h, d.w_, d.cin, d.ho, d.wo, d.cout, d.coutp = E * B, H, H, cin, Ho, Ho, cout, (cout + 63) // 64 * 64
        d.in_ld, d.out_ld, d.ipe, d.ks, d.stride, d.pad, d.dilate, d.dtype = cin, cout, B, 1, 1, 0, int(dilate), dtype
        if dilate:
            d.out, d.res = 0x1000, (0x1000 if inplace else 0x2000)     # in place: the residual IS the output
            d.res_ld, d.res_mode = cout, 1
        return d
    for cin, cout, H in ((128, 64, 32), (256, 128, 16), (512, 256, 8), (256, 256, 4)):
        plan, rows = _plan_and_rows(desc(cin, cout, H, 1, True))
        assert plan < 4000 and (plan, rows) == _plan_and_rows(desc(cin, cout, H, 1, False))
    # 4 x 4 maps: the zero-dilated 8 x 8 form would have taken the 8-wave LITE tile; the launch runs the 4-wave 128 x 128 one
    assert _plan_and_rows(desc(256, 256, 4, 0, True)) == (722, 32)
    assert _plan_and_rows(desc(256, 256, 4, 0, True, inplace=False)) == (2007, 64)     # (a separate residual: that form runs)


def test_stat_rows_are_those_of_the_kernel_that_runs(monkeypatch):
    """pmoe_conv2d_stat_rows goes through the same selection as the launch: the BatchNorm modes (PMOE_RES_DBN, PMOE_RES_INBN) get the
    rows of the kernel that serves them, and PMOE_ERR_UNSUPPORTED where none does -- a row count of another kernel would size a
    buffer that the launch never writes, or write past it."""
    from pmoe_amd import hip
    from pmoe_amd.hip import ConvDesc

    def desc(cin, cout, H, ks=3, stride=1, res_mode=0, E=4, B=64):
        d = ConvDesc()
        Ho = (H + 2 * (ks // 2) - ks) // stride + 1
        d.n, d.h, d.w_, d.cin, d.ho, d.wo, d.cout, d.coutp = E * B, H, H, cin, Ho, Ho, cout, (cout + 63) // 64 * 64
        d.in_ld, d.out_ld, d.ipe, d.ks, d.stride, d.pad = cin, cout, B, ks, stride, ks // 2
        d.res_mode, d.stats, d.bn_coef = res_mode, 1, 1
        if res_mode == hip.RES_DBN:
            d.res, d.res_ld = 1, cout
        return d
    plain = _plan_and_rows(desc(64, 64, 128))
    assert plain[0] == 1207
    assert _plan_and_rows(desc(64, 64, 128, res_mode=hip.RES_INBN)) == (1267, plain[1])      # the same resident-filter tiles
    assert _plan_and_rows(desc(64, 64, 128, res_mode=hip.RES_DBN)) == (1247, plain[1])
    assert _plan_and_rows(desc(128, 128, 64, res_mode=hip.RES_DBN))[0] in (5007, 5017)
    assert _plan_and_rows(desc(128, 128, 64, res_mode=hip.RES_DBN))[1] == _plan_and_rows(desc(128, 128, 64))[1]
    # nothing serves these: no rows either
    for d in (desc(128, 128, 64, res_mode=hip.RES_INBN), desc(128, 128, 64, stride=2, res_mode=hip.RES_DBN)):
        assert _plan_and_rows(d) == (hip.ERR_UNSUPPORTED, hip.ERR_UNSUPPORTED)
    monkeypatch.setenv("PMOE_RES_DMA", "0")           # (read per launch) the resident kernels without LDS-DMA serve neither mode
    for mode in (hip.RES_INBN, hip.RES_DBN):
        assert _plan_and_rows(desc(64, 64, 128, res_mode=mode)) == (hip.ERR_UNSUPPORTED, hip.ERR_UNSUPPORTED)


def test_wgrad_plan_reports_the_kernel_instantiation():
    """pmoe_conv2d_wgrad_plan: the LDS-DMA weight-gradient kernel for the dense 3x3 bf16 layers, its 2 x 4 wave layout for layers
    with <= 32 input channels (the stem's first convolution), the register-staged kernel for the strided ones."""
    import ctypes as C
    from pmoe_amd.hip import WgradDesc, load

    def plan(cin, cinp, cout, H, ks, stride, B=64, E=4, per_image=0):
        d = WgradDesc()
        pad = ks // 2
        Ho = (H + 2 * pad - ks) // stride + 1
        d.n, d.h, d.w_, d.cin, d.cinp, d.ho, d.wo, d.cout, d.coutp = E * B, H, H, cin, cinp, Ho, Ho, cout, (cout + 63) // 64 * 64
        d.x_ld, d.dy_ld, d.ipe, d.ks, d.stride, d.pad, d.dtype, d.per_image = cin, cout, B, ks, stride, pad, 0, per_image
        return load().pmoe_conv2d_wgrad_plan(C.byref(d))
    assert plan(64, 64, 64, 128, 3, 1) == 7309          # conv_wgrad_dma2_kernel (round 4: one accumulating wave per SIMD + a request-only wave)
    assert plan(256, 256, 256, 32, 3, 1) == 7309
    assert plan(16, 64, 64, 256, 3, 1) == 7109
    assert 6000 <= plan(64, 64, 128, 128, 3, 2) < 7000


WGRAD_SWEEP = REPO / "tests" / "golden" / "wgrad_select.json"
WGRAD_SWEEP_ENVS = ("", "PMOE_WGRAD_DMA=0", "PMOE_WGRAD_V2=0", "PMOE_WGRAD_NARROW=0", "PMOE_WGRAD_PIPE=0")
_WGRAD_MAPS = ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (40, 24), (71, 55), (13, 9), (7, 10),
               (256, 8), (200, 6), (32, 8))             # (the last three: output rows of <= 8 pixels, many of them)
WGRAD_SWEEP_EXEMPT_ROWS = 949                           # of the fixture's 1915 (test_wgrad_selection_table_is_the_recorded_one)


def _wgrad_sweep_descriptors():
    """(dtype, ks, stride, H, W, cin, ipe, E, per_image, bn_fused): every 14th row, by a multiplicative hash of its index, of
    the full cross (26880 rows; the fixture has to stay small)."""
    import itertools
    cross = itertools.product((0, 1), ((1, 1), (1, 2), (3, 1), (3, 2)), _WGRAD_MAPS, (16, 32, 64, 128, 256, 512),
                              (1, 2, 5, 64, 512), (1, 4), (0, 1), (0, 1))
    for i, (dtype, (ks, stride), (H, W), cin, ipe, E, per_image, bn_fused) in enumerate(cross):
        if (((i * 2654435761) & 0xFFFFFFFF) >> 16) % 14 == 0:
            yield (dtype, ks, stride, H, W, cin, ipe, E, per_image, bn_fused)


def _wgrad_desc(dtype, ks, stride, H, W, cin, ipe, E, per_image, bn_fused, cout=None):
    from pmoe_amd.hip import WgradDesc
    d = WgradDesc()
    cout = cout or max(cin, 64)
    ckw, pad = (64 if dtype == 0 else 32), ks // 2
    d.n, d.h, d.w_, d.cin, d.cinp = E * ipe, H, W, cin, (cin + ckw - 1) // ckw * ckw
    d.ho, d.wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    d.cout, d.coutp = cout, (cout + ckw - 1) // ckw * ckw
    d.x_ld, d.dy_ld, d.ipe, d.ks, d.stride, d.pad, d.dtype = cin, cout, ipe, ks, stride, pad, dtype
    d.per_image, d.bn_fused, d.bn_z_ld = per_image, bn_fused, cout
    return d


def _wgrad_plan_and_size(row):
    import ctypes as C
    from pmoe_amd.hip import load
    d = _wgrad_desc(*row)
    return [load().pmoe_conv2d_wgrad_plan(C.byref(d)), load().pmoe_conv2d_wgrad_ws_floats(C.byref(d))]


def _wgrad_record_sweep(monkeypatch_setenv):
    """-> the fixture's content: the default answers per row, and per switch only the rows it changes"""
    rows = list(_wgrad_sweep_descriptors())
    base = [_wgrad_plan_and_size(r) for r in rows]
    diffs = {}
    for env in WGRAD_SWEEP_ENVS[1:]:
        monkeypatch_setenv(*env.split("="))
        got = [_wgrad_plan_and_size(r) for r in rows]
        monkeypatch_setenv(env.split("=")[0], None)
        diffs[env] = {str(i): g for i, (g, b) in enumerate(zip(got, base)) if g != b}
    return {"fields": "dtype ks stride H W cin ipe E per_image bn_fused plan ws_floats",
            "rows": [list(r) + b for r, b in zip(rows, base)], "switch_changes": diffs}


def test_wgrad_selection_table_is_the_recorded_one(lib, monkeypatch):
    """pmoe_conv2d_wgrad_plan / pmoe_conv2d_wgrad_ws_floats over a sweep of descriptors (bf16 and f32, 1x1 and 3x3, both strides,
    4 x 4 to 256 x 256 and ragged maps, 16..512 channels, 1..512 images per expert, per-image and BatchNorm-fused forms), with the
    switches at their defaults and with PMOE_WGRAD_DMA / _V2 / _NARROW / _PIPE = 0: row by row the answers recorded in
    tests/golden/wgrad_select.json.

    The fixture was recorded from the library of commit 22a9f0b (the last one with the selection inside wgrad_dtype<T>), with
    this module's _wgrad_record_sweep: ``json.dump(_wgrad_record_sweep(setenv), open(WGRAD_SWEEP, "w"))`` where setenv(name, value)
    sets os.environ[name] (value None: removes it).

    One class of rows differs on purpose: a bn_fused descriptor that conv_wgrad_bnbwd_kernel does not serve (its plan is a
    PMOE_ERR_*).  The launch refuses it with that code; the size query used to answer 0 for every bn_fused descriptor and now
    answers the launch's code.  The exempt rows are exactly the fixture's rows with bn_fused = 1, plan < 0 and size 0, and their
    number is pinned."""
    import json
    fx = json.loads(WGRAD_SWEEP.read_text())
    rows = [tuple(r[:10]) for r in fx["rows"]]
    assert rows == list(_wgrad_sweep_descriptors())
    exempt = 0
    for env in WGRAD_SWEEP_ENVS:
        if env:
            monkeypatch.setenv(*env.split("="))
        changed = fx["switch_changes"].get(env, {})
        for i, r in enumerate(fx["rows"]):
            plan, ws = changed.get(str(i), r[10:])
            if r[9] and plan < 0:
                assert ws == 0
                ws = plan
                exempt += not env
            assert _wgrad_plan_and_size(rows[i]) == [plan, ws], (env, rows[i], plan, ws)
        if env:
            monkeypatch.delenv(env.split("=")[0])
    assert exempt == WGRAD_SWEEP_EXEMPT_ROWS
    # the sweep reaches every kernel family and both failure codes
    codes = {r[10] for r in fx["rows"]} | {v[0] for c in fx["switch_changes"].values() for v in c.values()}
    assert {7009, 7109, 7209, 7309, 6106, 6906, 6910, 6112, 6912, 6920, hip.ERR_UNSUPPORTED} <= codes, sorted(codes)


CONV_PLANS = REPO / "tests" / "golden" / "conv_plans.txt"


def test_whole_launch_plans_are_the_recorded_ones(lib, tmp_path):
    """tools/dump_plans.cpp against tests/golden/conv_plans.txt, line by line: every non-pointer field of every ConvLaunch and
    WgradPlan (tile geometry, grid, LDS bytes, patch buffer, magic numbers, instantiation parameters, K-split, workspace) that
    conv_select / wgrad_select fill over a sampled sweep -- both dtypes, 3x3 and 1x1, both strides, the stride-2 data gradients,
    the fused requests, the expert MLP layers, e4m3 operands -- at the defaults and at every switch value some test sets.

    The fixture was recorded from the library of commit d0a8bf3 (the last one with a tile-geometry computation per planner, the
    launch sequence written out per site and 34 switches), with tools/dump_plans.cpp built against that commit's kernels.h and
    library: ``dump_plans > tests/golden/conv_plans.txt``.  It prints the tile fields from the descriptor a kernel receives and
    none of the plan fields that went with the retired switches, so one source builds against both."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "dump_plans"
    libdir = hip.lib_path().parent
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", str(REPO / "tools" / "dump_plans.cpp"), f"-L{libdir}",
                           "-lpmoe_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], stderr=subprocess.DEVNULL)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = CONV_PLANS.read_text().split("\n")
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, (n + 1, g, w)
    assert len(got) == len(want)
    # the sweep reaches every kernel family of both selections, both failure codes, and every switch changes some row
    conv = [l for l in want if l.startswith("conv ")]
    wgrad = [l for l in want if l.startswith("wgrad ")]
    assert {int(k) for l in conv for k in re.findall(r"\| kind=(\d+)", l)} == set(range(1, 10))           # ConvKind
    assert {int(k) for l in wgrad for k in re.findall(r"[\]}] kind=(\d+)", l)} == {1, 2, 3, 4}               # WgradKind
    for lines in (conv, wgrad):
        assert {hip.ERR_ARG, hip.ERR_UNSUPPORTED} <= {int(c) for l in lines for c in re.findall(r"[\]}] code=(-\d+)", l)}
    flipped = {name for l in want for env in re.findall(r"\{([^}]*)\}", l) for name in re.findall(r"(PMOE_\w+)=", env)}
    assert flipped == _switch_table() - {"PMOE_STEM_WALK", "PMOE_STEM_WALK_KO"}                             # (those two plan nothing)


def _switch_table():
    """the names in the table of DESIGN.md's section "Switches the library reads" """
    text = (REPO / "DESIGN.md").read_text()
    section = text.split("### Switches the library reads", 1)[1].split("\n#", 1)[0]
    return set(re.findall(r"^\| `(PMOE_\w+)` \|", section, flags=re.M))


def test_switch_table_is_what_the_sources_read():
    """One reader (sw, csrc/common.h), one read rule (at the call), and a switch exists only while some test names it: the names
    the native sources pass to sw() are exactly DESIGN.md's table, nothing else in csrc/ reads the environment, and every name
    occurs in a file under tests/."""
    csrc = REPO / "pmoe_amd" / "csrc"
    sources = {f: f.read_text() for f in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h")) + sorted(csrc.glob("*.inc"))}
    read = {name for text in sources.values() for name in re.findall(r'\bsw\(\s*"(\w+)"', text)}
    assert read and read == _switch_table(), read ^ _switch_table()
    calls = [(f.name, n + 1) for f, text in sources.items() for n, l in enumerate(text.split("\n")) if re.search(r"\bsw\(", l)]
    named = [(f.name, n + 1) for f, text in sources.items() for n, l in enumerate(text.split("\n")) if re.search(r'\bsw\(\s*"PMOE_', l)]
    assert [c for c in calls if c not in named] == [("common.h", dict(calls)["common.h"])]       # (the definition; no computed names)
    getenv = [(f.name, n + 1) for f, text in sources.items() for n, l in enumerate(text.split("\n")) if "getenv" in l]
    assert len(getenv) == 1 and getenv[0][0] == "common.h", getenv
    tests = "".join(f.read_text() for f in sorted((REPO / "tests").rglob("*.py")) if f.name != "test_abi.py")
    tests += (REPO / "tests" / "test_abi.py").read_text().split("def _switch_table", 1)[0]
    unnamed = sorted(name for name in read if not re.search(name + r"\b", tests))
    assert not unnamed, unnamed


def test_one_launch_call_dtype_dispatch_and_grid_rule():
    """The host side of an entry point has one definition of each step (csrc/common.h): the launch and its error code, the dtype
    dispatch, the grid rule of the grid-stride kernels."""
    csrc = REPO / "pmoe_amd" / "csrc"
    sources = {f.name: f.read_text() for f in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h")) + sorted(csrc.glob("*.inc"))}
    assert len(sources) > 17
    for word in ("hipLaunchKernelGGL", "hipGetLastError"):
        assert [name for name, text in sources.items() if word in text] == ["common.h"], word
    for definition in (r"#\s*define\s+DISPATCH_DT\b", r"\bgrid_for\w*\s*\([^;{}]*\)\s*\{"):
        found = [name for name, text in sources.items() for _ in re.findall(definition, text, flags=re.M)]
        assert found == ["common.h"], (definition, found)


def _option_table():
    """the attribute names in the table of DESIGN.md's section "Options of the Python engines" """
    text = (REPO / "DESIGN.md").read_text()
    section = text.split("### Options of the Python engines", 1)[1].split("\n#", 1)[0]
    return set(re.findall(r"^\| `([a-z_0-9]+)` \|", section, flags=re.M))


def test_option_table_is_what_the_engines_declare():
    """The Python engines keep the library's rule: the boolean class attributes of the engine classes are exactly DESIGN.md's
    option table, every one is named by a file under tests/, and the package reads three environment names."""
    import inspect
    from pmoe_amd import engine, engine_punet
    classes = [c for m in (engine, engine_punet) for _, c in inspect.getmembers(m, inspect.isclass)
               if issubclass(c, engine.ExpertGroupEngine) and c.__module__ == m.__name__]
    assert {c.__name__ for c in classes} >= {"ExpertGroupEngine", "UNetEngine", "PredictiveUnetEngine", "PUNetEngine"}
    declared = {k for c in classes for k, v in vars(c).items() if isinstance(v, bool)}
    assert declared and declared == _option_table(), declared ^ _option_table()
    tests = "".join(f.read_text() for f in sorted((REPO / "tests").rglob("*.py")) if f.name != "test_abi.py")
    tests += (REPO / "tests" / "test_abi.py").read_text().split("def _switch_table", 1)[0]
    unnamed = sorted(name for name in declared if not re.search(r"\b" + name + r"\b", tests))
    assert not unnamed, unnamed
    py = "".join(f.read_text() for f in sorted((REPO / "pmoe_amd").rglob("*.py")))
    assert "getenv" not in py and len(re.findall(r"\benviron\b", py)) == len(re.findall(r"\benviron\.get\(\s*\"", py))      # (no computed names)
    assert set(re.findall(r"\benviron\.get\(\s*\"(\w+)\"", py)) == {"PMOE_OVERLAP_WGRAD", "PMOE_DP_COLLECTIVE", "PMOE_HIP_LIB"}


def test_wgrad_queries_answer_what_the_launch_does(lib):
    """Plan, size and fold go through the launch's own selection.  Three places where they once answered differently:"""
    import ctypes as C
    fused_ok = _wgrad_desc(0, 3, 1, 32, 32, 16, 2, 2, 1, 1)
    assert (lib.pmoe_conv2d_wgrad_plan(C.byref(fused_ok)), lib.pmoe_conv2d_wgrad_ws_floats(C.byref(fused_ok))) == (7209, 0)
    # 1. the size of a bn_fused descriptor that the fused kernel refuses is that refusal, not "no scratch needed"
    for bad in (_wgrad_desc(0, 3, 1, 32, 32, 64, 2, 2, 1, 1), _wgrad_desc(0, 3, 1, 32, 32, 16, 2, 2, 0, 1),
                _wgrad_desc(1, 3, 1, 32, 32, 16, 2, 2, 1, 1), _wgrad_desc(0, 3, 1, 8, 8, 16, 2, 2, 1, 1)):
        assert lib.pmoe_conv2d_wgrad_plan(C.byref(bad)) == lib.pmoe_conv2d_wgrad_ws_floats(C.byref(bad)) == hip.ERR_UNSUPPORTED
    bad = _wgrad_desc(0, 3, 1, 32, 32, 16, 2, 2, 1, 1)
    bad.bn_z_ld = 60                                            # (rows of z not 16-byte aligned)
    assert lib.pmoe_conv2d_wgrad_plan(C.byref(bad)) == lib.pmoe_conv2d_wgrad_ws_floats(C.byref(bad)) == hip.ERR_ARG
    # 2. the fold of a per_image descriptor has nothing to do (no launch: runs without a GPU), but only for a descriptor that the
    #    launch accepts -- it used to answer 0 before looking at it
    per_image = _wgrad_desc(0, 3, 1, 32, 32, 64, 2, 2, 1, 0)
    per_image.dw_ws = 0x1000
    assert lib.pmoe_conv2d_wgrad_fold(C.byref(per_image), None) == 0
    fused_ok.dw_ws = 0x1000
    assert lib.pmoe_conv2d_wgrad_fold(C.byref(fused_ok), None) == 0
    per_image.cinp = 128                                        # (the tiles would not cover dw exactly)
    assert lib.pmoe_conv2d_wgrad_fold(C.byref(per_image), None) == lib.pmoe_conv2d_wgrad_plan(C.byref(per_image)) == hip.ERR_ARG
    two_per_tile = _wgrad_desc(0, 3, 1, 8, 8, 64, 2, 2, 1, 0)   # (8 x 8 maps: four images per pixel block, not one workgroup per image)
    two_per_tile.dw_ws = 0x1000
    assert lib.pmoe_conv2d_wgrad_fold(C.byref(two_per_tile), None) == hip.ERR_UNSUPPORTED
    # 3. a bn_fused descriptor is the fused kernel's or nobody's in EVERY call: the fold once planned it as a plain one
    not_fused = _wgrad_desc(0, 3, 1, 32, 32, 64, 2, 2, 0, 1)
    not_fused.dw_ws = 0x1000
    assert lib.pmoe_conv2d_wgrad_fold(C.byref(not_fused), None) == hip.ERR_UNSUPPORTED


def test_launch_recorder_is_transparent_for_planning_calls():
    """hip.LaunchRecorder (pmoe_amd/infer.py:PlannedMixture): planning / query entry points pass through unrecorded, and the
    proxy is only in place while a recorder is active."""
    import ctypes as C
    from pmoe_amd import hip
    if torch.cuda.is_available():
        pytest.skip("the recorder's stream query is exercised by tests/test_model_gpu.py on a GPU")
    lib = hip.load()
    assert not isinstance(lib, hip._RecordingLib)
    rec = hip.LaunchRecorder()
    hip._recorder = rec                        # (entering the context needs a GPU stream)
    try:
        proxy = hip.load()
        assert isinstance(proxy, hip._RecordingLib)
        assert proxy.pmoe_abi_sizeof(0) == C.sizeof(hip.ConvDesc)
        assert rec.calls == []
    finally:
        hip._recorder = None
    assert hip.load() is lib


def test_cycle_stamped_tools_build_compiles(tmp_path):
    """tools/stamp_conv.py's -DPMOE_STAMP variant of the dominant conv kernel (never the product build) keeps compiling."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for name in ("conv_igemm", "conv_dma", "conv_wgrad"):
        src = REPO / "pmoe_amd" / "csrc" / f"{name}.hip"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DPMOE_STAMP",
                               "-c", str(src), "-o", str(tmp_path / f"{name}_stamp.o")], stderr=subprocess.DEVNULL)
    assert (tmp_path / "conv_igemm_stamp.o").stat().st_size > 0


def test_buffer_stores_with_sgpr_offset_keep_their_data_registers(tmp_path):
    """gfx950 reads the data registers of a > 64-bit buffer store after the instruction has issued; hipcc pads the ISA's
    "store data -> VALU write" hazard only for stores WITHOUT an SGPR offset (round 3: with one, conv3x3_respipe_kernel stored
    lanes 12-15 / 44-47 of a dword that the next instruction had already overwritten).  Static guard over the kernels that use
    raw buffer stores: no VALU write to a store's data registers within two instructions of a store that carries an SGPR offset."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for name in ("conv_c16", "conv_c1x1", "conv_res"):
        out = tmp_path / f"{name}.s"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                               str(REPO / "pmoe_amd" / "csrc" / f"{name}.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
        lines = out.read_text().split("\n")
        for n, l in enumerate(lines):
            m = re.match(r"\s*buffer_store_dwordx[34] v\[(\d+):(\d+)\], v\d+, s\[\d+:\d+\], (s\d+)", l)
            if not m:
                continue
            lo, hi = int(m.group(1)), int(m.group(2))
            k, seen = n + 1, 0
            while seen < 2 and k < len(lines):
                t = lines[k].strip()
                k += 1
                if not t or t[0] in ";.":
                    continue
                seen += 1
                if t.startswith("s_nop"):
                    break
                w = re.match(r"v_(?!cmp)\S+ v\[?(\d+)", t)
                assert not (w and lo <= int(w.group(1)) <= hi), (name, l.strip(), t)


def test_vmcnt_counting_kernels_have_no_scratch_in_their_main_loops(tmp_path):
    """the LDS-DMA kernels order their operands with COUNTED `s_waitcnt vmcnt(N)`; a register spill would put scratch
    loads / stores -- which count in vmcnt too -- into the stream and let an MFMA read a tile that has not landed, silently.
    Static guard on the ISA: conv3x3_dma_kernel<*> (incl. the producer-wave instantiations), conv3x3s2_dma_kernel<*>,
    conv3x3_dma_f8_kernel and conv3x3_respipe_kernel<*> have NO scratch access at all; conv_wgrad_dma2_kernel's request-only
    waves may spill set-up values once (they wait for vmcnt(0) anyway), but nothing between its accumulating waves' MFMAs."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.split("\n")[0]

    def kernels(name):
        out = tmp_path / f"{name}.s"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                               str(REPO / "pmoe_amd" / "csrc" / f"{name}.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
            yield m.group(1), m.group(2).split("\n")
    checked = 0
    for src, pats in (("conv_dma", ("conv3x3_dma_kernel", "conv3x3_dma_stream_kernel", "conv3x3s2_dma_kernel", "conv3x3_dma_f8_kernel")),
                      ("conv_res", ("conv3x3_respipe_kernel",))):
        for sym, body in kernels(src):
            if any(p in sym for p in pats):
                bad = [l.strip() for l in body if "scratch_" in l]
                assert not bad, (ver, sym, bad[:4])
                checked += 1
    for sym, body in kernels("conv_wgrad"):
        if "conv_wgrad_dma2_kernel" in sym:
            mf = [k for k, l in enumerate(body) if "v_mfma" in l]
            assert mf and not [l for l in body[mf[0]:mf[-1] + 1] if "scratch_" in l], (ver, sym)
            checked += 1
    assert checked >= 10, checked
