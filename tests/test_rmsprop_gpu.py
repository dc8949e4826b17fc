"""FusedRMSprop on the GPU (csrc/optim.hip: rmsprop_upd, mt_rmsprop_kernel, mt_rmsprop_pack_kernel).

Against float64: the four cases of tests/rmsprop_util.py, clip in place and clip fused, checkpoints both ways.  Alignment: the
scalar path gives the bits of the 16-byte path.  ``packs=``: parameters and state bit-identical to the plain launch, the
destinations bit-identical to an ordinary pack, on the layer list and through the engines of tests/test_optim_packs_gpu.py.  And
FusedAdam, which now shares its base class and its kernel bodies with FusedRMSprop, still does what it did."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import optim  # noqa: E402
from tests import rmsprop_util as U  # noqa: E402
from tests.parity_util import GOLDEN, build_pair  # noqa: E402
from tests.test_optim_gpu import SHAPES as ADAM_SHAPES  # noqa: E402
from tests.test_optim_packs_gpu import (BF, F32, GUARD, HEAD_CIN, HEAD_PARTS, LAYERS, SENTINEL, _Conv, _Provider, _Run,  # noqa: E402
                                        _same_state, pack_calls)  # noqa: E402,F401  (pack_calls: a fixture)


def test_shapes_are_the_adam_tests_and_the_chunk_edges():
    assert U.SHAPES == list(ADAM_SHAPES) + [(optim.CHUNK,), (optim.CHUNK - 1,)]


# ------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_fused_rmsprop_and_clip_match_float64(case):
    lr, wd, momentum, centered, max_norm = case
    keys = U.state_keys(momentum, centered)
    yard = U.Yardstick(case)
    got = [torch.nn.Parameter(v.cuda()) for v in U.values(0)]
    o_got = optim.FusedRMSprop(got, **U.hyper(case))
    worst = 0.0
    for step, grads in enumerate(U.gradient_steps()):
        for b, g in zip(got, grads):
            b.grad = None if g is None else g.cuda()
        n_ref = yard.step(grads)
        if max_norm > 0:
            if step % 2:                   # (a) clip in place like torch, (b) fused into the update
                n_got = optim.clip_grad_norm_(got, max_norm)
                o_got.step()
            else:
                n_got = optim.clip_grad_norm_(got, max_norm, scale=False)
                o_got.step(clip=n_got)
            assert n_got.is_cuda and abs(n_got.item() - n_ref.item()) <= 2e-6 * n_ref.item()
        else:
            o_got.step()
        excess = max(U.param_excess(b, a) for a, b in zip(yard.params, got))
        worst = max(worst, excess)
        print(f"step {step}: {excess:.3f} of the parameter bound")
        assert excess <= 1.0, (step, excess)
    for i, b in enumerate(got):
        assert list(o_got.state[b]) == ["step"] + list(keys)
        for k in keys:
            excess = U.state_excess(o_got.state[b][k], yard.state(i, k))
            assert excess <= 1.0, (U.SHAPES[i], k, excess)
        assert float(o_got.state[b]["step"]) == float(yard.state(i, "step")) == (U.STEPS - 1 if i == 1 else U.STEPS)
    print(f"worst over the run: {worst:.3f} of the parameter bound")
    # checkpoint interchange: the fused optimizer's state loads into torch's RMSprop on the GPU, and that one's into a fresh
    # fused optimizer; one more step of each on equal gradients
    theirs = [torch.nn.Parameter(b.detach().clone()) for b in got]
    again = [torch.nn.Parameter(b.detach().clone()) for b in got]
    o_theirs, o_again = torch.optim.RMSprop(theirs, **U.hyper(case)), optim.FusedRMSprop(again, **U.hyper(case))
    o_theirs.load_state_dict(copy.deepcopy(o_got.state_dict()))          # (load_state_dict keeps a tensor that needs no cast)
    o_again.load_state_dict(copy.deepcopy(o_theirs.state_dict()))
    gen = torch.Generator().manual_seed(5)
    for a, b, c in zip(theirs, again, got):
        gr = (torch.randn(a.shape, generator=gen) * 0.5).cuda()
        a.grad, b.grad, c.grad = gr.clone(), gr.clone(), gr.clone()
    o_theirs.step()
    o_again.step()
    o_got.step()
    for i, (a, b, c) in enumerate(zip(theirs, again, got)):
        assert torch.equal(b, c), U.SHAPES[i]                   # the state went round unchanged
        torch.testing.assert_close(b, a, rtol=U.PARAM_RTOL, atol=U.PARAM_ATOL)
        assert float(o_theirs.state[a]["step"]) == float(o_again.state[b]["step"]) == float(o_got.state[c]["step"])


# ------------------------------------------------------------------------------------------------------------------ alignment
def _off_by_one_float(t):
    """a contiguous copy of ``t`` that starts one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    lead = 1 + (-(buf.data_ptr() // 4) % 4)                     # buf + lead floats = 4 bytes past a 16-byte boundary
    view = buf[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("case", U.CASES[:2], ids=U.CASE_IDS[:2])
def test_unaligned_tensors_take_the_scalar_path_to_the_same_bits(case):
    lr, wd, momentum, centered, max_norm = case
    keys = U.state_keys(momentum, centered)
    gen = torch.Generator().manual_seed(3)
    init = [v.cuda() for v in U.values(0)]
    # a state some way into a run; grad_avg^2 <= 0.0025 < 0.01 <= square_avg, so the centered root stays real
    start = {"square_avg": lambda r: 0.01 + r, "grad_avg": lambda r: (r - 0.5) * 0.1, "momentum_buffer": lambda r: r - 0.5}
    state0 = [{k: start[k](torch.rand(v.shape, generator=gen)).cuda() for k in keys} for v in init]
    runs = []
    for shift in (lambda t: t.clone(), _off_by_one_float):
        ps = [torch.nn.Parameter(shift(v)) for v in init]
        assert all(p.data_ptr() % 16 == (0 if shift is not _off_by_one_float else 4) for p in ps)
        opt = optim.FusedRMSprop(ps, **U.hyper(case))
        for p, st in zip(ps, state0):
            opt.state[p] = {"step": torch.tensor(0.0), **{k: shift(v) for k, v in st.items()}}
        runs.append((ps, opt, shift))
    for _, grads in zip(range(3), U.gradient_steps()):
        clip = None
        for ps, opt, shift in runs:
            for p, g in zip(ps, grads):
                p.grad = None if g is None else shift(g.cuda())
            if max_norm > 0 and clip is None:      # one coefficient for both copies (the norm kernel sums unaligned gradients
                clip = optim.clip_grad_norm_(ps, max_norm, scale=False)         # in another order: its last bit may differ)
            opt.step(clip=clip)
        (pa, oa, _), (pb, ob, _) = runs
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert torch.equal(a, b), U.SHAPES[i]
            for k in keys:
                assert ob.state[b][k].data_ptr() % 16 == 4
                assert torch.equal(oa.state[a][k], ob.state[b][k]), (U.SHAPES[i], k)


def test_one_state_tensor_as_momentum_buffer_then_as_grad_avg():
    """The optimizer's device tables are cached on the pointers they hold.  A momentum-only and a centered-only optimizer fill
    equally many columns -- (param, grad, square_avg, X) -- but X travels in another slot of the row: the key names the columns,
    so the second optimizer over the SAME tensors gets its own table (the first one's has a NULL where this kernel reads)."""
    gen = torch.Generator().manual_seed(11)
    shape = (3, optim.CHUNK + 5)
    p0, g0 = torch.randn(shape, generator=gen).cuda() * 0.1, torch.randn(shape, generator=gen).cuda()
    sq0, x0 = 0.01 + torch.rand(shape, generator=gen).cuda(), (torch.rand(shape, generator=gen).cuda() - 0.5) * 0.1
    p, sq, x = torch.nn.Parameter(p0.clone()), sq0.clone(), x0.clone()
    p.grad = g0.clone()

    def run(param, state, **mode):
        opt = optim.FusedRMSprop([param], lr=1e-3, alpha=U.ALPHA, eps=U.EPS, **mode)
        opt.state[param] = {"step": torch.tensor(0.0), **state}
        opt.step()
        return opt

    def fresh(**mode):
        q = torch.nn.Parameter(p0.clone())
        q.grad = g0.clone()
        key = "momentum_buffer" if mode["momentum"] > 0 else "grad_avg"
        state = {"square_avg": sq0.clone(), key: x0.clone()}
        run(q, state, **mode)
        return q, state["square_avg"], state[key]
    for mode, key in ((dict(momentum=0.5, centered=False), "momentum_buffer"), (dict(momentum=0, centered=True), "grad_avg")):
        with torch.no_grad():                                   # the same tensors, at the same addresses, with their first values
            p.copy_(p0)
            sq.copy_(sq0)
            x.copy_(x0)
        run(p, {"square_avg": sq, key: x}, **mode)
        want = fresh(**mode)
        for have, w, what in zip((p, sq, x), want, ("param", "square_avg", key)):
            assert torch.equal(have, w) and not torch.equal(have, {"param": p0, "square_avg": sq0}.get(what, x0)), (mode, what)


def test_momentum_below_float32_still_has_its_buffer():
    """a momentum that is positive as a double and 0 in float32: torch keeps a momentum_buffer and so does the kernel (buf = g / d)"""
    ps = [torch.nn.Parameter(torch.full((5,), 0.5).cuda()) for _ in range(2)]
    kw = dict(lr=1e-2, momentum=1e-60, centered=True)
    ours, theirs = optim.FusedRMSprop([ps[0]], **kw), torch.optim.RMSprop([ps[1]], **kw)
    for _ in range(2):
        for q in ps:
            q.grad = torch.arange(1.0, 6.0).cuda()
        ours.step()
        theirs.step()
    assert list(ours.state[ps[0]]) == list(theirs.state[ps[1]])
    torch.testing.assert_close(ours.state[ps[0]]["momentum_buffer"], theirs.state[ps[1]]["momentum_buffer"], rtol=1e-5, atol=0)
    assert ours.state[ps[0]]["momentum_buffer"].abs().min() > 0
    torch.testing.assert_close(ps[0], ps[1], rtol=U.PARAM_RTOL, atol=U.PARAM_ATOL)


# --------------------------------------------------------------------------------------------------------- kernel-level packs
def _packs_against_plain(dtype, make, keys, clip):
    """``make(params, packs)`` -> optimizer.  Three steps of one with ``packs=provider`` against one without, on the layer list
    of tests/test_optim_packs_gpu.py: parameters and ``keys`` of the state equal, every destination -- padding and the sentinels
    round it included -- equal to an ordinary pack of the updated parameters."""
    gen = torch.Generator().manual_seed(7)
    convs = [_Conv(co, ci, ks, dg, dtype, gen, bias=(co == 130)) for co, ci, ks, dg in LAYERS]
    convs.append(_Conv(5, HEAD_CIN, 1, True, dtype, gen, parts=HEAD_PARTS, bias=True))
    dests = [c.pack() for c in convs]
    got = [p for c in convs for p in c.params()]
    got.append(torch.nn.Parameter(torch.randn(777, generator=gen).cuda()))        # no sink: takes the plain launch
    by_param = {}
    for c, d in zip(convs, dests):
        by_param.update(c.sinks(*d))
    prov = _Provider(by_param, got)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in got]
    o_got, o_ref = make(got, prov), make(ref, None)
    for step in range(3):
        for a, b in zip(ref, got):
            gr = (torch.randn(a.shape, generator=gen) * 3.0).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        if step == 1:                      # a packed parameter without a gradient keeps its value and its pack
            ref[0].grad = got[0].grad = None
            kept = got[0].detach().clone()
        if clip:
            o_ref.step(clip=optim.clip_grad_norm_(ref, 1.0, scale=False))
            o_got.step(clip=optim.clip_grad_norm_(got, 1.0, scale=False))
        else:
            o_ref.step()
            o_got.step()
        assert prov._packed_version == prov.param_version()
        if step == 1:
            assert torch.equal(got[0], kept)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (step, i, tuple(a.shape))
            assert list(o_ref.state[a]) == list(o_got.state[b]) == ["step"] + list(keys)
            for k in keys:
                assert torch.equal(o_ref.state[a][k], o_got.state[b][k]), (step, i, k)
            assert float(o_ref.state[a]["step"]) == float(o_got.state[b]["step"]) == (step + 1 if i or step < 1 else step)
        for c, d in zip(convs, dests):
            for have, want in zip(d, c.pack()):
                if have is not None:       # the whole buffer: destination, its padding, the sentinels around it
                    assert torch.equal(have.whole, want.whole), (step, c.cout, c.cin, c.ks)
                    assert (have.whole[:GUARD] == SENTINEL).all() and (have.whole[-GUARD:] == SENTINEL).all()
    assert sorted(o_ref.state_dict()["state"]) == sorted(o_got.state_dict()["state"])
    assert o_ref.state_dict()["param_groups"] == o_got.state_dict()["param_groups"]


@pytest.mark.parametrize("case,clip", [(U.CASES[1], False), (U.CASES[0], True)], ids=["centered-momentum-wd", "centered-clip"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_kernel_updates_like_the_plain_launch_and_packs_like_the_pack(dtype, case, clip):
    _packs_against_plain(dtype, lambda ps, packs: optim.FusedRMSprop(ps, packs=packs, **U.hyper(case)),
                         U.state_keys(case[2], case[3]), clip)


def test_adam_still_updates_like_its_plain_launch_and_packs_like_the_pack():
    """the copy of tests/test_optim_packs_gpu.py's kernel-level test that sits beside the shared base and kernel bodies"""
    kw = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=True)
    _packs_against_plain(BF, lambda ps, packs: optim.FusedAdam(ps, packs=packs, **kw),
                         ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), True)


# -------------------------------------------------------------------------------------------------------------- engine level
class _RmspropRun(_Run):
    """tests/test_optim_packs_gpu.py's run (forward, moe_loss, backward, clip_grad_norm_(1.0, scale=False), step(clip=)) with the
    trainers' rmsprop block as its optimizer -- at a tenth of its learning rate.  The first centred update is
    lr * g / sqrt(0.0099 g^2) = 10 lr for EVERY weight, whatever its gradient: at the block's 2e-4 that is 2e-3 per weight.
    Observed once, on g4 in float32 and not checked by anything here: at 2e-4 the copy WITHOUT ``packs`` came back from its second
    forward with standard deviations of exactly 0 (torch's Normal refuses them).  2e-5 takes the 2e-4 first step that the Adam runs
    of tests/test_optim_packs_gpu.py take; the assertions below include that the losses stay finite."""

    def __init__(self, model, ocfg, dev, calls, packs):
        self.model, self.ocfg, self.dev, self.calls = model, ocfg, dev, calls
        ps = [p for p in model.parameters() if p.requires_grad]
        self.opt = optim.FusedRMSprop(ps, lr=2e-5, momentum=0, alpha=0.99, eps=1e-8, centered=True, weight_decay=0,
                                      packs=model if packs else None)
        self.eng = model._engine()


def _pair(name, dtype, calls):
    g = torch.load(GOLDEN / f"{name}.pt", weights_only=False)
    ocfg, _, model, inp = build_pair(g, dtype)
    dev = {k: v.cuda() for k, v in inp.items()}
    return (_RmspropRun(copy.deepcopy(model), ocfg, dev, calls, False), _RmspropRun(copy.deepcopy(model), ocfg, dev, calls, True))


@pytest.mark.parametrize("name,dtype", [("g4_moealt_e4_b2_64", F32), ("g1_moe_e4_b2_128", BF)], ids=["g4-f32", "g1-bf16"])
def test_training_with_packs_is_bit_identical_and_packs_nothing(name, dtype, pack_calls):
    plain, packs = _pair(name, dtype, pack_calls)
    full = None
    for k in range(3):
        key_before = packs.eng.replay_key()
        (la, _), (lb, nb) = plain.iteration(), packs.iteration()
        assert torch.equal(la, lb) and torch.isfinite(la), (k, la.item(), lb.item())
        if k == 0:
            full = nb
            assert full >= len(packs.eng.all_convs) > 0
        else:
            assert nb == 0, (k, nb)
        assert packs.eng.replay_key() != key_before            # a recorded chain still sees that the weights changed
        assert packs.eng._packed_version == packs.eng.param_version()
        assert _same_state(plain, packs, k) == (full, 0)       # the plain model repacks everything, every step


def test_currency_parameter_changed_in_place(pack_calls):
    plain, packs = _pair("g4_moealt_e4_b2_64", F32, pack_calls)
    seen = []
    for k in range(3):
        (la, _), (lb, nb) = plain.iteration(), packs.iteration()
        assert torch.equal(la, lb), (k, la.item(), lb.item())
        repacked, needed = _same_state(plain, packs, k)
        assert repacked > 0
        seen.append((nb, needed))
        if k == 0:
            for run in (plain, packs):
                with torch.no_grad():
                    next(p for n, p in run.model.named_parameters() if "layer2.0.conv1.weight" in n).mul_(1.03125)
    full = seen[0][0]
    assert full > 0 and seen == [(full, 0), (full, 0), (0, 0)], seen     # the change forces one full repack, then current again
