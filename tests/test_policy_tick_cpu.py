"""Host-side checks of the closed-loop tick (pmoe_amd.infer.PolicyTick): the two new C-ABI symbols, the numpy restatement of
the draw rule that tests/test_policy_tick_gpu.py holds the kernel to, and the errors raised before any device is touched."""
import numpy as np
import pytest
import torch

from pmoe_amd import hip
from tests.test_abi import _declared
from tests.test_policy_tick_gpu import EDGE, MAX_EXCLUDED, hash_uniform, restated_all


@pytest.fixture(scope="module")
def lib():
    if not hip.lib_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def test_library_exports_the_tick_kernels(lib):
    decl = _declared()
    for name, nargs in (("pmoe_history_push", 11), ("pmoe_mixture_draw", 14)):
        assert hasattr(lib, name), name
        assert decl[name] == nargs == len(hip.SIGNATURES[name])
    assert lib.pmoe_version() == 401
    # argument checks that need no device: a null ring, a zero-slot ring, an NHWC copy of a bf16 ring, a missing state
    assert lib.pmoe_history_push(None, None, 1, 1, 16, hip.DT_F32, None, 0, 0, 0, None) == hip.ERR_ARG
    one = 16
    assert lib.pmoe_history_push(one, one, 1, 0, 16, hip.DT_F32, None, 0, 0, 0, None) == hip.ERR_ARG
    assert lib.pmoe_history_push(one, one, 1, 2, 48, hip.DT_BF16, one, 3, 16, hip.DT_BF16, None) == hip.ERR_ARG
    assert lib.pmoe_mixture_draw(one, one, one, None, one, None, None, None, None, None, None, 1, 4, None) == hip.ERR_ARG
    assert lib.pmoe_mixture_draw(one, one, one, one, one, one, None, None, None, None, None, 1, 4, None) == hip.ERR_ARG


def test_hash_uniform_restatement():
    u = hash_uniform(12345, np.arange(1 << 16, dtype=np.uint64))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * np.float32(16777216.0), np.round(u * np.float32(16777216.0)))      # multiples of 2^-24
    assert abs(float(u.mean()) - 0.5) < 4.0 / (12.0 * u.size) ** 0.5
    # splitmix64 of 0 with seed 0 (the finalizer's well-known first output e220a8397b1dcdaf): top 24 bits
    assert hash_uniform(0, np.array([1], dtype=np.uint64))[0] == np.float32(0xE220A8 / 16777216.0)


def test_restated_draw_f32_against_f64():
    """the component choice of the f32 statement against the same rule in f64: they may differ only where the threshold lies
    within EDGE of a cumulative edge, and that must stay rare for the inputs the GPU test uses"""
    c32, a32, _, m32 = restated_all(np.float32)
    c64, a64, _, _ = restated_all(np.float64)
    safe = m32 > EDGE
    assert (~safe).mean() <= MAX_EXCLUDED
    assert np.array_equal(c32[safe], c64[safe])
    assert np.array_equal(a32[c32 == c64], a64[c32 == c64])
    assert c32.shape == (1024, 64) and set(np.unique(c32)) == {0, 1, 2, 3}


def _cpu_model():
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import stage2_model_cfg
    return get_model(stage2_model_cfg("moe", 2, dropout=0.0))


def test_policy_tick_refuses_train_mode_and_unknown_modes_before_any_device_call(monkeypatch):
    from pmoe_amd import infer

    def no_device(*a, **k):
        raise AssertionError("PolicyTick touched the device layer before validating its arguments")
    monkeypatch.setattr(hip, "load", no_device)
    model = _cpu_model()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        infer.PolicyTick(model)
    model.eval()
    with pytest.raises(ValueError, match="mode"):
        infer.PolicyTick(model, mode="graph")
    with pytest.raises(TypeError):
        infer.PolicyTick(torch.nn.Linear(2, 2).eval())


def test_infer_does_not_import_the_oracle():
    import pathlib
    import subprocess
    import sys
    repo = pathlib.Path(__file__).resolve().parents[1]
    code = "import sys; import pmoe_amd.infer; assert not [m for m in sys.modules if m.split('.')[0] == 'oracle'], 'oracle imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=repo)
    assert "oracle" not in (repo / "pmoe_amd" / "infer.py").read_text()
