"""FusedRMSprop without a GPU: the two entry points of the C ABI, the constructor and the state it makes, the trainers'
dispatch, the refusal of CPU tensors -- and the conditioning of the schedule that tests/test_rmsprop_gpu.py runs."""
import ctypes
import types

import pytest
import torch

from pmoe_amd import hip, optim
from tests import rmsprop_util as U
from tests.test_abi import _declared

ENTRY = {"pmoe_mt_rmsprop": 12, "pmoe_mt_rmsprop_packs": 14}


@pytest.fixture(scope="module")
def lib():
    if not hip.lib_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def test_entry_points_are_declared_bound_exported_and_check_their_arguments(lib):
    decl = _declared()
    for name, n in ENTRY.items():
        assert decl.get(name) == n == len(hip.SIGNATURES[name]), name
        assert hasattr(lib, name), name
    assert lib.pmoe_version() == hip.ABI_VERSION == 401
    assert lib.pmoe_abi_sizeof(2) == 64 == ctypes.sizeof(optim.OptTensor)
    h = (1e-2, 0.99, 1e-8, 0.0, 0.0, 1)
    for n, ptr in ((1, None), (0, 0x1000)):                   # (refused before any launch: runs without a GPU)
        assert lib.pmoe_mt_rmsprop(ptr, ptr, ptr, n, *h, None, None) == hip.ERR_ARG
        assert lib.pmoe_mt_rmsprop_packs(ptr, ptr, ptr, ptr, ptr, n, *h, None, None) == hip.ERR_ARG
    assert lib.pmoe_mt_rmsprop_packs(0x1000, None, 0x1000, 0x1000, 0x1000, 1, *h, None, None) == hip.ERR_ARG     # no pack table


def test_constructor_has_torchs_defaults_and_errors():
    def p():
        return [torch.nn.Parameter(torch.zeros(3))]
    ours, theirs = optim.FusedRMSprop(p()), torch.optim.RMSprop(p())
    assert set(ours.defaults) == {"lr", "alpha", "eps", "weight_decay", "momentum", "centered"}
    for k, v in ours.defaults.items():
        assert theirs.defaults[k] == v and type(theirs.defaults[k]) is type(v), k
    for bad in (dict(lr=-1e-3), dict(eps=-1e-8), dict(momentum=-0.1), dict(weight_decay=-0.01), dict(alpha=-0.5)):
        with pytest.raises(ValueError) as want:
            torch.optim.RMSprop(p(), **bad)
        with pytest.raises(ValueError) as got:
            optim.FusedRMSprop(p(), **bad)
        assert str(got.value) == str(want.value)
    # the block every shipped conf/stage_*.yaml carries (lr 2e-4 in stage 2, 1e-3 in stages 1 and 3)
    for lr in (2e-4, 1e-3):
        block = dict(lr=lr, momentum=0, alpha=0.99, eps=1e-8, centered=True, weight_decay=0)
        assert optim.FusedRMSprop(p(), **block).param_groups[0]["centered"] is True
    with pytest.raises(ValueError, match="hosts no engine"):
        optim.FusedRMSprop(p(), packs=torch.nn.Linear(2, 2))


@pytest.mark.parametrize("momentum,centered", [(0, False), (0, True), (0.9, False), (0.9, True)])
def test_state_keys_are_torchs(momentum, centered):
    """after an empty step (no gradient anywhere) there is no state, like torch; after a refused one -- CPU tensors: the state is
    made before the launch looks at the tensors -- the keys, their order, and ``step`` as torch's CPU float32 scalar"""
    kw = dict(lr=1e-3, momentum=momentum, centered=centered)
    a, b = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
    ours, theirs = optim.FusedRMSprop([a], **kw), torch.optim.RMSprop([b], **kw)
    ours.step()
    theirs.step()
    assert len(ours.state) == len(theirs.state) == 0
    a.grad, b.grad = torch.ones(4), torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ours.step()
    theirs.step()
    got, want = ours.state[a], theirs.state[b]
    assert list(got) == list(want) == ["step"] + list(U.state_keys(momentum, centered))
    assert got["step"].dtype == want["step"].dtype == torch.float32 and got["step"].device == want["step"].device
    assert got["step"].shape == want["step"].shape == () and float(got["step"]) == float(want["step"]) == 1.0
    for k in U.state_keys(momentum, centered):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype
    assert torch.equal(a, torch.ones(4))                        # the refused step changed nothing
    # checkpoints interchange in both directions
    theirs.load_state_dict(ours.state_dict())
    ours.load_state_dict(theirs.state_dict())
    assert list(ours.state[a]) == ["step"] + list(U.state_keys(momentum, centered))


def test_get_optimizer_is_the_trainers_dispatch():
    cfg = types.SimpleNamespace(adam=dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True),
                                rmsprop=dict(lr=2e-4, momentum=0, alpha=0.99, eps=1e-8, centered=True, weight_decay=0))

    def p():
        return [torch.nn.Parameter(torch.zeros(3))]
    for name in ("adam", "Adam", "ADAM"):
        o = optim.get_optimizer(name, p(), cfg)
        assert type(o) is optim.FusedAdam and o.defaults["amsgrad"] is True and o.defaults["lr"] == 2e-4
    for name in ("rmsprop", "RMSprop", "RMSPROP"):
        o = optim.get_optimizer(name, p(), cfg)
        assert type(o) is optim.FusedRMSprop and o.defaults["centered"] is True and o.defaults["alpha"] == 0.99
    for name in ("sgd", "", "adamw"):
        with pytest.raises(ValueError) as e:
            optim.get_optimizer(name, p(), cfg)
        assert str(e.value) == f"Unknown optimizer {name}"
    with pytest.raises(ValueError, match="hosts no engine"):      # packs= reaches the optimizer
        optim.get_optimizer("rmsprop", p(), cfg, packs=torch.nn.Linear(2, 2))


def test_refuses_cpu_tensors_and_sparse_gradients():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        optim.FusedRMSprop([p]).step()
    q = torch.nn.Parameter(torch.zeros(4))
    q.grad = torch.ones(4).to_sparse()
    with pytest.raises(RuntimeError, match="FusedRMSprop does not support sparse gradients"):
        optim.FusedRMSprop([q]).step()
    with pytest.raises(ValueError, match=r"FusedRMSprop.step\(clip=...\)"):
        optim.FusedRMSprop([p]).step(clip=torch.zeros(()))


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_schedule_is_well_conditioned_in_float32(case):
    """The guard of the bounds that tests/test_rmsprop_gpu.py applies: torch's own float32 RMSprop against the float64 yardstick,
    on the same schedule, stays within HALF of them.  (Passes without the feature: it runs none of it.)

    The guard is about the update rule, so the float32 side takes its clip coefficient from the yardstick's norm: torch's float32
    ``clip_grad_norm_`` on the CPU sums 3.3 M squares in float32 and is off by 3e-5 of the norm, 0.7 of the state bound by itself
    -- an error of that norm, not of RMSprop (pmoe_amd.optim.clip_grad_norm_ sums its partials in double: 2e-6,
    tests/test_optim_gpu.py).  With torch's own float32 ``clip_grad_norm_`` instead, measured on the CPU: its norm is off by up to
    3.4e-5; case 0 reaches 0.17 of the parameter bound and 0.74 of the state bound, case 3 1.40 of the parameter bound and 0.58 of
    the state bound (cases 1 and 2 do not clip, or clip at 1e4 and never scale) -- that variant cannot pass, at 0.5 or at 1."""
    yard = U.Yardstick(case)
    f32 = [torch.nn.Parameter(v) for v in U.values(0)]
    opt = torch.optim.RMSprop(f32, foreach=False, **U.hyper(case))
    worst_p = 0.0
    for grads in U.gradient_steps():
        norm = yard.step(grads)
        coef = 1.0 if norm is None else min(1.0, case[4] / (norm.item() + 1e-6))
        for p, g in zip(f32, grads):
            p.grad = None if g is None else g * coef
        opt.step()
        worst_p = max(worst_p, max(U.param_excess(a, b) for a, b in zip(f32, yard.params)))
    worst_s = max(U.state_excess(opt.state[p][k], yard.state(i, k))
                  for i, p in enumerate(f32) for k in U.state_keys(case[2], case[3]))
    print(f"float32 torch against float64: {worst_p:.3f} of the parameter bound, {worst_s:.3f} of the state bound")
    assert worst_p <= 0.5 and worst_s <= 0.5, (worst_p, worst_s)
    for i, p in enumerate(f32):
        assert float(opt.state[p]["step"]) == float(yard.state(i, "step")) == (U.STEPS - 1 if i == 1 else U.STEPS)
