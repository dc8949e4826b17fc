"""Every kernel of csrc/stem_tail.hip against the float64 reference of its own operation (tests/stem_tail_ref.py), at the smallest
shapes that reach each edge: odd sizes, partial strips and lane groups, windows that are mostly padding, image and expert
boundaries, C = 32 / 64 / 128, more partitions than rows; gather kernels and both row-walking widths.

Two kinds of input (tests/test_stem_tail_cpu.py checks on the CPU what is assumed of them here):
  lattice     every intermediate is a multiple of 2^-10 small enough that float32 arithmetic is EXACT in any order, fused or not:
              the kernels must reproduce the reference bit for bit, through exact ties, zero plateaus and an all-way-tie channel.
  continuous  randn data, redrawn where a float32 evaluation could land on the other side of a ReLU or of a bfloat16 rounding
              boundary; the bounds are derived from float32 rounding alone:
                sums   |got - ref| <= (L + 8) 2^-24 sum|term|, L = longest chain of sequential float32 additions of the launch
                dz2    |got - ref| <= 8 2^-24 sum|addends| + half a unit in the last place of the storage type
                y      bfloat16: equal to the rounded reference; float32 (nothing is rounded, so the rule of a rounding boundary
                       has no meaning there): within 8 2^-24 sum|addends| + half a unit in the last place, and outputs whose two
                       best candidates are that close count as ambiguous
Backward kernels receive the REFERENCE's arg-max, so that a forward mistake cannot hide or cause a backward one.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops  # noqa: E402
from tests import stem_tail_ref as R  # noqa: E402

DEV = "cuda"
F64 = torch.float64
EPS = 2.0 ** -24
IDS = [R.case_id(c) for c in R.CASES]
KINDS = ("lattice", "continuous")
MODES = {"gather": ("0", None), "walk2": ("1", "2"), "walk4": ("1", "4")}
NPARTS = ("one", "four", "rows+1")


def set_mode(monkeypatch, mode):
    walk, ko = MODES[mode]
    monkeypatch.setenv("PMOE_STEM_WALK", walk)
    if ko is None:
        monkeypatch.delenv("PMOE_STEM_WALK_KO", raising=False)
    else:
        monkeypatch.setenv("PMOE_STEM_WALK_KO", ko)


@functools.lru_cache(maxsize=None)
def setup(case, kind):
    """inputs on the device and every reference result, computed once per (case, kind) and never modified"""
    E, B, H, W, C, dtype = case
    d = R.lattice_case(case) if kind == "lattice" else R.continuous_case(case)
    z, dpool, k = d["z"], d["dpool"], d["k"]
    amb = R.ambiguous_outputs(case, d)
    po = amb["pool"]
    s = {"z": z, "dpool": dpool, "k": k, "pool": po, "amb": amb["outputs"],
         "stats": R.stats(z, k["sc2"], k["sh2"], k["mu2"], B),
         "p1": R.bwd(1, z, dpool, po["code"], k, B), "p2": R.bwd(2, z, dpool, po["code"], k, B),
         "p3": R.bwd(3, z, dpool, po["code"], k, B), "pooled": R.pooled(po["y"], dpool, po["code"], k, E)}
    s["zd"], s["dpd"] = z.to(dtype).to(DEV), dpool.to(dtype).to(DEV)
    s["yd"], s["coded"] = po["y"].to(dtype).to(DEV), po["code"].to(DEV)
    s["kd"] = {n: t.to(torch.float32).to(DEV) for n, t in k.items()}
    for n in R.CONSTS:
        assert torch.equal(s["kd"][n].cpu().to(F64), k[n])
    s["consts"] = [s["kd"][n] for n in R.CONSTS]
    return s


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(got, ref, what):
    """exact equality of every value (the sign of a zero apart: a masked gradient is +0 or -0 by how the mask is applied)"""
    got, ref = got.to(F64), ref.to(F64)
    bad = got != ref
    if bad.any():
        i = bad.flatten().nonzero()[:6, 0]
        pairs = list(zip(got.flatten()[i].tolist(), ref.flatten()[i].tolist()))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first (got, ref): {pairs}; "
                             f"indices {[tuple(int(v) for v in torch.unravel_index(j, got.shape)) for j in i]}")


def half_ulp(x, dtype):
    """upper bound of half a unit in the last place of |x| in the storage type"""
    return x.abs() * (2.0 ** -8 if dtype == torch.bfloat16 else EPS)


def geometry(case):
    E, B, H, W, C, dtype = case
    ve = 8 if dtype == torch.bfloat16 else 4
    return C // ve, 256 // (C // ve)          # CV lanes per pixel, RL pixels in flight per workgroup


def nparts_of(name, rows):
    return {"one": 1, "four": 4, "rows+1": rows + 1}[name]


def chain_rows(case, nparts):
    """stem_tail_kernel: a thread adds ceil(W / RL) pixels of each of its partition's rows, then one lane adds the RL columns"""
    E, B, H, W, C, dtype = case
    _, RL = geometry(case)
    rpp = -(-(B * H) // nparts)
    return rpp * -(-W // RL) + RL


def chain_pooled(case, nparts):
    """stem_tail_pooled_kernel: a thread adds every RL-th pooled pixel of its partition"""
    E, B, H, W, C, dtype = case
    _, RL = geometry(case)
    rpp = -(-(B * R.out_size(H) * R.out_size(W)) // nparts)
    return -(-rpp // RL) + RL


def check_sum(got, ref, ref_abs, L, kind, what, keep=None):
    if keep is not None:
        got, ref, ref_abs = got[..., keep], ref[..., keep], ref_abs[..., keep]
    assert not torch.isnan(got).any(), f"{what}: unwritten elements"
    err = (got - ref).abs()
    print(f"{what}: max |err| {err.max().item():.3e}, max err / (2^-24 sum|term|) {(err / (EPS * ref_abs).clamp_min(1e-300)).max().item():.2f}, L {L}")
    if kind == "lattice":
        assert torch.equal(got, ref), f"{what}: not exact, max |err| {err.max().item():.3e}"
    else:
        assert (err <= (L + 8) * EPS * ref_abs).all(), what


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_pool_matches_reference(case, kind, mode, monkeypatch):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    po, kd = s["pool"], s["kd"]
    set_mode(monkeypatch, mode)
    y = torch.full(po["y"].shape, float("nan"), dtype=dtype, device=DEV)
    am = torch.full(po["y"].shape, 0xEE, dtype=torch.uint8, device=DEV)
    ops.stem_tail_pool(s["zd"], y, am, kd["sc2"], kd["sh2"], kd["sc1"], kd["sh1"], kd["mu2"], kd["mu1"], B)
    torch.cuda.synchronize()
    y, am = y.cpu(), am.cpu()
    assert not torch.isnan(y.float()).any() and int((am & 0x7f).max()) <= 8, "unwritten outputs"
    ref_y = po["y"].to(dtype)
    if kind == "lattice":
        assert torch.equal(bits(y), bits(ref_y))
        assert torch.equal(am, po["code"])
        return
    ok = ~s["amb"]
    tap = (am & 0x7f).to(torch.int64)
    at_tap = lambda t9: t9.gather(0, tap[None])[0]
    assert torch.equal(am[ok], po["code"][ok])
    if dtype == torch.bfloat16:
        assert torch.equal(bits(y)[ok], bits(ref_y)[ok])
        slack = po["y"] * 2.0 ** -7                                        # one unit in the last place of the maximum
    else:
        full = R.windows(po["chain"]["p3_full"], 0.0)
        err = (y.to(F64) - po["y"]).abs()
        bound = 8 * EPS * at_tap(full) + half_ulp(po["y"], dtype)
        print(f"y: max err / bound {(err / bound.clamp_min(1e-300))[ok].max().item():.3f}")
        assert (err <= bound)[ok].all()
        slack = 2.0 ** -18 * at_tap(full)
    # ambiguous outputs: the kernel still names a candidate of the window that is as good as the maximum
    assert (at_tap(po["cand"]) >= po["y"] - slack).all()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_dz2_matches_reference(case, kind, mode, monkeypatch):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    set_mode(monkeypatch, mode)
    dz = torch.full(s["z"].shape, float("nan"), dtype=dtype, device=DEV)
    part = torch.empty(E, 1, 2, C, device=DEV)
    ops.stem_tail_bwd(3, s["zd"], s["dpd"], s["coded"], dz, s["consts"], part, 1, E, B)
    torch.cuda.synchronize()
    dz = dz.cpu()
    assert not torch.isnan(dz.float()).any(), "unwritten elements"
    ref = s["p3"]["dz2"]
    if kind == "lattice":
        same(dz, ref.to(torch.float32).to(dtype), "dz2")
        return
    err = (dz.to(F64) - ref).abs()
    f32 = 8 * EPS * s["p3"]["dz2_abs"]
    bound = f32 + half_ulp(ref.abs() + f32, dtype)
    print(f"dz2: max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_dz2_from_the_kernels_own_argmax(mode, monkeypatch):
    """forward and backward chained as the engine chains them: same dz2, bit for bit"""
    case = R.CASES[0]
    E, B, H, W, C, dtype = case
    s = setup(case, "lattice")
    kd = s["kd"]
    set_mode(monkeypatch, mode)
    y = torch.empty(s["pool"]["y"].shape, dtype=dtype, device=DEV)
    am = torch.full(y.shape, 0xEE, dtype=torch.uint8, device=DEV)
    dz = torch.full(s["z"].shape, float("nan"), dtype=dtype, device=DEV)
    ops.stem_tail_pool(s["zd"], y, am, kd["sc2"], kd["sh2"], kd["sc1"], kd["sh1"], kd["mu2"], kd["mu1"], B)
    ops.stem_tail_bwd(3, s["zd"], s["dpd"], am, dz, s["consts"], torch.empty(E, 1, 2, C, device=DEV), 1, E, B)
    torch.cuda.synchronize()
    same(dz.cpu(), s["p3"]["dz2"].to(torch.float32).to(dtype), "dz2")


@pytest.mark.parametrize("parts", NPARTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reductions_match_reference(case, kind, parts, monkeypatch):
    """stats (with shiftc and the three part_x moments), phases 1 and 2, the pooled pass and the closed-form combine"""
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    kd = s["kd"]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    fold = lambda p: p.cpu().to(F64).sum(1)                      # the partition rows, added in float64
    npr = nparts_of(parts, B * H)
    L = chain_rows(case, npr)

    st = s["stats"]
    part, part_x, shiftc = nan(E, npr, 2, C), nan(E, npr, 3, C), nan(E, C)
    ops.stem_tail_stats(s["zd"], kd["sc2"], kd["sh2"], kd["mu2"], part, npr, E, B, shiftc=shiftc, part_x=part_x)
    torch.cuda.synchronize()
    assert not torch.isnan(part).any() and not torch.isnan(part_x).any(), "unwritten partition rows"
    shiftc = shiftc.cpu().to(F64)
    if kind == "lattice":
        assert torch.equal(shiftc, st["shiftc"])
    else:
        first = st["chain"]["p2_mag"].reshape(E, -1, C)[:, 0]
        assert ((shiftc - st["shiftc"]).abs() <= 8 * EPS * first).all()
    for i, n in enumerate(("s1", "s2")):
        check_sum(fold(part)[:, i], st[n], st["abs_" + n], L, kind, f"stats {n}")
    for i, n in enumerate(("x0", "x1", "x2")):
        check_sum(fold(part_x)[:, i], st[n], st["abs_" + n], L, kind, f"part_x {n}")

    for phase in (1, 2):
        ref = s[f"p{phase}"]
        part = nan(E, npr, 2, C)
        ops.stem_tail_bwd(phase, s["zd"], s["dpd"], s["coded"], None, s["consts"], part, npr, E, B)
        torch.cuda.synchronize()
        assert not torch.isnan(part).any(), "unwritten partition rows"
        for i, n in enumerate(("s1", "s2")):
            check_sum(fold(part)[:, i], ref[n], ref["abs_" + n], L, kind, f"phase {phase} {n}")

    # the pooled path recovers xhat from y / sc: a channel with sc1 == 0 is DEFINED as contributing 0 there
    keep = [c for c in range(C) if kind != "lattice" or c != R.ZERO_SC1_CHANNEL]
    np4 = nparts_of(parts, B * R.out_size(H) * R.out_size(W))
    part4 = nan(E, np4, 4, C)
    ops.stem_tail_pooled(s["yd"], s["dpd"], s["coded"], s["consts"], part4, np4, E)
    torch.cuda.synchronize()
    assert not torch.isnan(part4).any(), "unwritten partition rows"
    pl = s["pooled"]
    for i in range(4):
        check_sum(fold(part4)[:, i], pl["sums"][:, i], pl["abs"][:, i], chain_pooled(case, np4), kind, f"pooled {i}", keep)

    # combine: the same closed forms from the same partition rows; its count is no power of two, so the bound in both kinds
    out1, out2 = nan(E, 2, C), nan(E, 2, C)
    count = B * H * W
    ops.stem_tail_combine(part4, np4, part_x, npr, s["consts"], count, out1, out2, E, C)
    torch.cuda.synchronize()
    cb = R.combine(part4.cpu().to(F64), part_x.cpu().to(F64), s["k"], count)
    Lc = max(np4, npr)
    check_sum(out1.cpu().to(F64), cb["out1"], cb["abs1"], Lc, "continuous", "combine out1", keep)
    check_sum(out2.cpu().to(F64), cb["out2"], cb["abs2"], Lc, "continuous", "combine out2", keep)


def test_bad_arguments_are_refused_before_any_launch():
    E, B, H, W, C = 1, 2, 4, 4, 64
    lib = hip.load()
    N, Ho, Wo = E * B, R.out_size(H), R.out_size(W)
    bf = torch.bfloat16
    z, dz = torch.zeros(N, H, W, C, dtype=bf, device=DEV), torch.full((N, H, W, C), 7.0, dtype=bf, device=DEV)
    y, dp = torch.full((N, Ho, Wo, C), 7.0, dtype=bf, device=DEV), torch.zeros(N, Ho, Wo, C, dtype=bf, device=DEV)
    am = torch.full((N, Ho, Wo, C), 0xEE, dtype=torch.uint8, device=DEV)
    part, part_x, shiftc = (torch.full((E, 4, 4, C), 7.0, device=DEV) for _ in range(3))
    k = [torch.ones(E, C, device=DEV) for _ in range(12)]
    kp = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in k])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    BF = hip.DT_BF16

    def stats(nparts=4, c=C, dtype=BF):
        return lib.pmoe_stem_tail_stats(p(z), p(k[0]), p(k[1]), p(k[2]), p(part), nparts, p(shiftc), p(part_x), E, B, H, W, c,
                                        dtype, None)

    def pool(n=N, c=C, dtype=BF):
        return lib.pmoe_stem_tail_pool(p(z), p(y), p(am), *(p(k[i]) for i in range(6)), n, B, H, W, c, dtype, None)

    def bwd(phase, nparts=4, c=C, dtype=BF):
        return lib.pmoe_stem_tail_bwd(phase, p(z), p(dp), p(am), p(dz), kp, p(part), nparts, E, B, H, W, c, dtype, None)

    def pooled(nparts=4, rpe=B * Ho * Wo, c=C, dtype=BF):
        return lib.pmoe_stem_tail_pooled(p(y), p(dp), p(am), kp, p(part), nparts, E, rpe, c, dtype, None)

    calls = {
        "C not a multiple of the vector width": [lambda: stats(c=12), lambda: pool(c=12), lambda: bwd(1, c=12), lambda: bwd(3, c=12),
                                                 lambda: pooled(c=12), lambda: stats(c=6, dtype=hip.DT_F32)],
        "C / ve not a power of two": [lambda: stats(c=24), lambda: pool(c=24), lambda: bwd(2, c=24), lambda: bwd(3, c=24),
                                      lambda: pooled(c=24), lambda: pool(c=12, dtype=hip.DT_F32)],
        "nparts < 1": [lambda: stats(nparts=0), lambda: bwd(1, nparts=0), lambda: bwd(3, nparts=-1), lambda: pooled(nparts=0)],
        "phase outside 1..3": [lambda: bwd(0), lambda: bwd(4)],
        "N % ipe != 0": [lambda: pool(n=1)],
        "rows_per_expert < 1": [lambda: pooled(rpe=0)],
        "unknown dtype": [lambda: stats(dtype=7), lambda: pool(dtype=7), lambda: bwd(1, dtype=7), lambda: bwd(3, dtype=7),
                          lambda: pooled(dtype=7)],
    }
    for mode_env in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PMOE_STEM_WALK", mode_env)
            for what, fs in calls.items():
                for i, f in enumerate(fs):
                    assert f() == hip.ERR_ARG, f"{what} (call {i}, PMOE_STEM_WALK={mode_env})"
    torch.cuda.synchronize()
    for t in (dz, y, part, part_x, shiftc):
        assert (t == 7.0).all(), "a refused call wrote to its outputs"
    assert (am == 0xEE).all()
    # the same buffers ARE valid: the well-formed calls succeed
    assert stats() == 0 and pool() == 0 and bwd(1) == 0 and bwd(3) == 0 and pooled() == 0
    torch.cuda.synchronize()
