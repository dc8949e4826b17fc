"""The engines issue the same launches as before they asked ``ops.ConvLaunch.served()`` instead of comparing plan codes (-m gpu).

tests/golden/launch_sequences.json holds, per engine pass of tests/launch_seq.py, every library call of the pass reduced to its
entry-point name and the non-pointer fields of its descriptor; it was recorded with ``python tests/launch_seq.py`` on the revision
BEFORE the prepared-launch API (its engines still compared plan codes with hand-copied lists), so equality here says that each
fusion is taken and refused exactly where it was.  Every case is chosen so that its probes answer both ways."""
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops  # noqa: E402
from tests.launch_seq import cases, field, record  # noqa: E402

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "launch_sequences.json").read_text())

# (probe, answer) pairs that must occur in a case.  dbn: _dgrad_with_bn_reduce; wgrad_bn: _backbone_fwd's bn_defer; in_fp8: _conv;
# inbn3: _conv3's planning call; inbn: _conv1x1_after_bn; shuffle_c: _upconv_fused (with and without a pending BatchNorm)
BOTH = {
    # yes: the 64-channel layers / H * W >= 256.  no: the stride-2 and small-map layers
    "mixture_train_bf16": {("dbn", True), ("dbn", False), ("wgrad_bn", True)},
    # yes: layer2 (4096 pixels per expert).  no: layer3 / layer4
    "mixture_fp8_forward": {("in_fp8", True), ("in_fp8", False)},
    "punet_untaped_train_forward": {("shuffle_c", False), ("inbn3", True), ("inbn3", False), ("inbn", True)},
    "punet_untaped_train_forward_b2_128": {("shuffle_c", True), ("shuffle_c", False), ("inbn3", True), ("inbn3", False), ("inbn", True)},
    "punet_untaped_train_forward_b1_64": {("shuffle_c", False), ("inbn3", True), ("inbn", False)},
    "unet_train_taped": set(),
}


@pytest.fixture
def asked(monkeypatch):
    """every answer the engines' probes get: [(probe, served)]"""
    log = []
    served, plan, wgrad_bn = ops.ConvLaunch.served, ops.conv2d_plan, ops.conv2d_wgrad_bn_served

    def spy_served(self):
        d, ok = self.d, served(self)
        log.append(("shuffle_c" if d.shuffle_c else "in_fp8" if d.in_fp8 else
                    {hip.RES_DBN: "dbn", hip.RES_INBN: "inbn"}.get(d.res_mode, "plain"), ok))
        return ok

    def spy_plan(*a, **kw):
        code = plan(*a, **kw)
        if kw.get("res_mode") == hip.RES_INBN:
            log.append(("inbn3", code >= 0))
        return code

    def spy_wgrad_bn(*a, **kw):
        ok = wgrad_bn(*a, **kw)
        log.append(("wgrad_bn", ok))
        return ok
    monkeypatch.setattr(ops.ConvLaunch, "served", spy_served)
    monkeypatch.setattr(ops, "conv2d_plan", spy_plan)
    monkeypatch.setattr(ops, "conv2d_wgrad_bn_served", spy_wgrad_bn)
    return log


def _fused(seq):
    """the fused requests of a reduced sequence: [(res_mode if a BatchNorm mode else 0, ks, shuffle_c > 0, in_fp8)]"""
    convs = [r for r in seq if r[0] == "pmoe_conv2d_igemm"]
    return [(field(r, "res_mode") if field(r, "res_mode") in (hip.RES_DBN, hip.RES_INBN) else 0, field(r, "ks"),
             field(r, "shuffle_c") > 0, field(r, "in_fp8")) for r in convs]


@pytest.mark.parametrize("name", list(BOTH))
def test_same_launches_as_with_the_plan_code_lists(tmp_path, asked, name):
    model, run, seq, outs = record(cases(tmp_path)[name])
    assert ("plain", True) not in asked and ("plain", False) not in asked, "a launch without a fused request needs no question"
    assert BOTH[name] <= set(asked), (name, sorted(set(asked)))
    fused = _fused(seq)
    if name == "unet_train_taped":      # the taped U-Net: nothing applied on load, no fused scatter (only PMOE_RES_DBN, as before)
        assert not any(f[0] == hip.RES_INBN or f[2] or f[3] for f in fused)
    want = GOLDEN[name]
    assert len(seq) == len(want), (len(seq), len(want))
    for i, (a, b) in enumerate(zip(seq, want)):
        assert a == b, (name, i, a, b)
    if name in ON_LOAD:
        # ... and the fused launches compute what the unfused pairs do, bit for bit (tests/test_punet_gpu.py:
        # test_punet_fused_forward_paths_match_the_unfused_ones holds the same at batch 4, 128 x 128)
        assert ON_LOAD[name] <= set(fused), sorted(set(fused))
        plain, run_plain = cases(tmp_path)[name]()
        for sw in ("fuse_in_bn", "fuse_in_bn_1x1", "fuse_upconv_shuffle"):
            assert getattr(type(plain._engine()), sw) is True, sw
            setattr(plain._engine(), sw, False)
        ref = run_plain()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, ref))


# the launches with a BatchNorm + ReLU applied on load that a PU-Net case must contain: (res_mode, ks, shuffle_c, in_fp8)
ON_LOAD = {"punet_untaped_train_forward": {(hip.RES_INBN, 3, False, 0), (hip.RES_INBN, 1, False, 0)},
           "punet_untaped_train_forward_b2_128": {(hip.RES_INBN, 3, False, 0), (hip.RES_INBN, 1, False, 0), (hip.RES_INBN, 1, True, 0)}}


def test_conv3_asks_on_every_pass(tmp_path, monkeypatch):
    """The library reads PMOE_RES_PIPE per launch (tools/ab_*.py flip such switches inside one process): a second pass after the
    switch went off must run the unfused pair in the 64-channel blocks -- the verdict of the first pass is not kept."""
    make = cases(tmp_path)["punet_untaped_train_forward"]
    model, run, seq, _ = record(make)
    on_load = [f for f in _fused(seq) if f[:2] == (hip.RES_INBN, 3)]
    applies = sum(r[0] == "pmoe_bn_apply" for r in seq)
    assert on_load
    monkeypatch.setenv("PMOE_RES_PIPE", "0")
    with hip.LaunchRecorder() as rec:
        run()
    torch.cuda.synchronize()
    from tests.launch_seq import reduce_calls
    seq2 = reduce_calls(rec.calls)
    assert not [f for f in _fused(seq2) if f[:2] == (hip.RES_INBN, 3)]
    assert sum(r[0] == "pmoe_bn_apply" for r in seq2) == applies + len(on_load)          # one BatchNorm + ReLU pass per block instead


# ---- the passes of tests/launch_seq.py engine_cases: recorded from the revision before the engines' untested options were retired and
# the U-Net primitives got a base class of their own (python tests/launch_seq.py tests/golden/launch_sequences_engines.json)
ENGINES = json.loads((Path(__file__).resolve().parent / "golden" / "launch_sequences_engines.json").read_text())

# entry points (or a descriptor field) that show the branch a case is there for, and ones it must not contain
TAKES = {
    "mixture_eval_bf16": ({"pmoe_pack_conv_weights_scaled"}, {"pmoe_bn_apply", "pmoe_colstats"}),            # folded BatchNorms
    "mixture_train_f32": ({"pmoe_colstats", "pmoe_unpack_conv_wgrad"}, {"pmoe_mlp_wgrad"}),                   # no epilogue statistics
    "moealt_train_bf16": ({"pmoe_copy_window", "pmoe_mlp_wgrad"}, set()),                                     # _merge_alt_head
    "punet_expert_train_taped": ({"pmoe_eca_stem_fold", "pmoe_pixel_shuffle2"}, {"pmoe_pixel_unshuffle2"}),   # frozen PU-Net
    "punet_expert_train_taped_f6": ({"pmoe_eca_stem_fold"}, {"pmoe_pixel_unshuffle2"}),
    "stage1_train_taped": ({"pmoe_add_window", "pmoe_pixel_unshuffle2", "pmoe_unpack_conv_wgrad"}, set()),    # through time
}


@pytest.mark.parametrize("name", list(TAKES))
def test_engine_passes_issue_the_recorded_launches(tmp_path, name):
    """eval mode, f32, ``moe_alt``, the taped PU-Net expert and stage-1 back-propagation through time: call for call and
    descriptor field for descriptor field what the engines issued before."""
    from tests.launch_seq import engine_cases
    _, _, seq, _ = record(engine_cases(tmp_path)[name])
    want = ENGINES[name]
    names = {r[0] for r in seq}
    has, has_not = TAKES[name]
    assert has <= names and not (has_not & names), (sorted(has - names), sorted(has_not & names))
    if name.endswith("_f6"):            # the 138-channel stem input lives in rows of 192 channels
        assert any(r[0] == "pmoe_conv2d_igemm" and field(r, "cin") == 192 and field(r, "ks") == 3 for r in seq)
    assert len(seq) == len(want), (len(seq), len(want))
    for i, (a, b) in enumerate(zip(seq, want)):
        assert a == b, (name, i, a, b)


# ---- every argument of every launch (tests/launch_seq.py reduce_scalars): the goldens above keep descriptor fields only, so the
# partition counts, rows per expert, ReLU flags and element counts of the BatchNorm, GAP and stem-tail launches were unpinned.
# Recorded from the revision before the engines' BatchNorm hand-offs became named records (BNCoef, Partials)
SCALARS = json.loads((Path(__file__).resolve().parent / "golden" / "launch_sequences_scalars.json").read_text())


@pytest.mark.parametrize("name", list(SCALARS))
def test_every_launch_gets_the_recorded_scalar_arguments(tmp_path, name):
    from tests.launch_seq import reduce_scalars, scalar_cases
    _, _, seq, _ = record(scalar_cases(tmp_path)[name], reduce_scalars)
    want = SCALARS[name]
    assert {"pmoe_bn_finalize", "pmoe_gap_partial"} <= {r[0] for r in seq}
    assert len(seq) == len(want), (len(seq), len(want))
    for i, (a, b) in enumerate(zip(seq, want)):
        assert a == b, (name, i, a, b)
