"""FusedAdam(packs=...): the Adam launch that also writes the engine's packed weights (csrc/optim.hip: mt_adam_pack_kernel).

Kernel level: parameters and moments bit-identical to the plain launch, the destinations bit-identical to an ordinary pack of
the updated parameters (padding and the memory around them included).  Engine level: a training run with ``packs=model`` is
bit-identical to one without, and from the second forward on it packs nothing.  Currency: whatever makes the optimizer's claim
unsafe ends in the ordinary full repack and the same results."""
import collections
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops, optim  # noqa: E402
from pmoe_amd.engine import PackSinks, r16, r64  # noqa: E402
from tests.parity_util import GOLDEN, build_pair  # noqa: E402

F32, BF = torch.float32, torch.bfloat16
E = 2
SENTINEL = -512.0          # exact in bf16; no weight gets near it
GUARD = 64                 # sentinel elements before and after every destination

# (cout, cin, ks, has a data-gradient operand)
LAYERS = [(64, 12, 3, True),          # cin padded to 16
          (5, 1536, 1, True),         # cout below one 16-row block
          (130, 70, 3, True),         # ragged in both directions, more than one tile each way
          (128, 256, 3, False)]       # many tiles; no data-gradient operand
HEAD_CIN, HEAD_PARTS = 40, [(0, 4), (4, 1)]       # (first row, rows) of a 64-row fused operand


class _Dest:
    """a destination inside a larger sentinel-filled buffer"""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + n].view(shape)


class _Conv:
    """one layer of E experts packed the ordinary way: rows [r0, r0 + rows) of its operands belong to each of ``parts``"""

    def __init__(self, cout, cin, ks, dgrad, dtype, gen, parts=None, bias=False):
        self.cout, self.cin, self.ks, self.taps, self.dtype = cout, cin, ks, ks * ks, dtype
        self.coutp, self.cinp, self.dg_rows, self.dg_red = r64(cout), r16(cin), r64(cin), r16(cout)
        self.parts = parts or [(0, cout)]
        self.w = [[torch.nn.Parameter((torch.randn(rows, cin, ks, ks, generator=gen) * 0.1).cuda()) for _ in range(E)]
                  for _, rows in self.parts]
        self.b = [[torch.nn.Parameter((torch.randn(rows, generator=gen) * 0.1).cuda()) for _ in range(E)]
                  for _, rows in self.parts] if bias else None
        self.dgrad = dgrad

    def pack(self):
        """-> (fwd, dgrd, bias) destinations holding the ordinary pack of the present parameters"""
        fwd = _Dest((E, self.coutp, self.taps, self.cinp), self.dtype)
        dg = _Dest((E, self.dg_rows, self.taps, self.dg_red), self.dtype) if self.dgrad else None
        full = [torch.cat([self.w[k][e].detach() for k in range(len(self.parts))]).contiguous() for e in range(E)]
        ops.pack_conv_weights(hip.ptr_table(full, "cuda"), fwd.t, dg.t if dg else None, E, self.cout, self.cin, self.ks,
                              self.coutp, self.cinp, self.dg_rows, self.dg_red, self.dtype)
        bias = None
        if self.b is not None:
            bias = _Dest((E, self.coutp), F32)
            fullb = [torch.cat([self.b[k][e].detach() for k in range(len(self.parts))]).contiguous() for e in range(E)]
            ops.pack_bias(hip.ptr_table(fullb, "cuda"), bias.t, E, self.cout, self.coutp)
        torch.cuda.synchronize()           # (the concatenated sources die here)
        return fwd, dg, bias

    def sinks(self, fwd, dg, bias):
        out = {}
        for k, (r0, rows) in enumerate(self.parts):
            for e in range(E):
                out[id(self.w[k][e])] = (fwd.t[e].data_ptr(), dg.t[e].data_ptr() if dg else 0, rows, self.cin, self.taps,
                                         hip._TORCH_DT[self.dtype], self.cinp, r0, self.dg_red if dg else 0, r0)
                if self.b is not None:
                    out[id(self.b[k][e])] = (bias.t[e].data_ptr(), 0, rows, 1, 1, hip._TORCH_DT[F32], 1, r0, 0, 0)
        return out

    def params(self):
        return [p for part in self.w for p in part] + ([p for part in self.b for p in part] if self.b else [])


class _Provider:
    """what FusedAdam(packs=...) asks of an engine"""

    def __init__(self, by_param, params):
        self.by_param, self.params = by_param, params
        self._packed_version = self.param_version()

    def pack_sinks(self):
        return PackSinks(1, self.by_param)

    def param_version(self):
        return sum(p._version for p in self.params)

    def packs_written(self, before):
        assert before == self._packed_version
        self._packed_version = self.param_version()
        return True


@pytest.mark.parametrize("amsgrad,clip", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_kernel_updates_like_the_plain_launch_and_packs_like_the_pack(dtype, amsgrad, clip):
    gen = torch.Generator().manual_seed(7)
    convs = [_Conv(co, ci, ks, dg, dtype, gen, bias=(co == 130)) for co, ci, ks, dg in LAYERS]
    convs.append(_Conv(5, HEAD_CIN, 1, True, dtype, gen, parts=HEAD_PARTS, bias=True))
    dests = [c.pack() for c in convs]
    got = [p for c in convs for p in c.params()]
    extra = torch.nn.Parameter(torch.randn(777, generator=gen).cuda())           # no sink: takes the plain launch
    got.append(extra)
    by_param = {}
    for c, d in zip(convs, dests):
        by_param.update(c.sinks(*d))
    prov = _Provider(by_param, got)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in got]
    kw = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=amsgrad)
    o_got, o_ref = optim.FusedAdam(got, packs=prov, **kw), optim.FusedAdam(ref, **kw)
    for step in range(3):
        for a, b in zip(ref, got):
            gr = (torch.randn(a.shape, generator=gen) * 3.0).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        if step == 1:                      # a packed parameter without a gradient keeps its value and its pack
            ref[0].grad = got[0].grad = None
        if clip:
            o_ref.step(clip=optim.clip_grad_norm_(ref, 1.0, scale=False))
            o_got.step(clip=optim.clip_grad_norm_(got, 1.0, scale=False))
        else:
            o_ref.step()
            o_got.step()
        assert prov._packed_version == prov.param_version()
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (step, i, tuple(a.shape))
            for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
                assert torch.equal(o_ref.state[a][k], o_got.state[b][k]), (step, i, k)
            assert float(o_ref.state[a]["step"]) == float(o_got.state[b]["step"])
        for c, d in zip(convs, dests):
            for have, want in zip(d, c.pack()):
                if have is not None:       # the whole buffer: destination, its padding, the sentinels around it
                    assert torch.equal(have.whole, want.whole), (step, c.cout, c.cin, c.ks)
                    assert (have.whole[:GUARD] == SENTINEL).all() and (have.whole[-GUARD:] == SENTINEL).all()
    assert sorted(o_ref.state_dict()["state"]) == sorted(o_got.state_dict()["state"])
    assert o_ref.state_dict()["param_groups"] == o_got.state_dict()["param_groups"]


def test_entry_point_checks_its_arguments():
    lib = hip.load()
    assert lib.pmoe_abi_sizeof(3) == 64
    assert lib.pmoe_mt_adam_packs(None, None, None, None, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0.1, 0.1, None,
                                  None) == hip.ERR_ARG
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    assert lib.pmoe_mt_adam_packs(p, p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0.1, 0.1, None, None) == hip.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- engine level
_PACK_OPS = ("pack_conv_weights", "pack_bias", "pack_conv_weights_fp8")


@pytest.fixture
def pack_calls(monkeypatch):
    calls = collections.Counter()
    for name in _PACK_OPS:
        def counted(*a, _fn=getattr(ops, name), _name=name, **kw):
            calls[_name] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


def _banks(eng):
    out = []
    for layer in eng.all_convs:
        out += [layer.w_fwd, layer.w_dg, layer.bias_packed, layer.w_f8]
    return out


class _Run:
    """one model, its optimizer, and the count of pack calls of each of its forwards"""

    def __init__(self, model, ocfg, dev, calls, packs, only=None):
        self.model, self.ocfg, self.dev, self.calls = model, ocfg, dev, calls
        ps = [p for n, p in model.named_parameters() if p.requires_grad and (only is None or only in n)]
        assert ps
        self.opt = optim.FusedAdam(ps, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, amsgrad=True, packs=model if packs else None)
        self.eng = model._engine()

    def counted(self, fn):
        before = sum(self.calls.values())
        out = fn()
        return out, sum(self.calls.values()) - before

    def iteration(self):
        """-> (loss, pack calls of the forward)"""
        from pmoe_amd.loss import moe_loss
        d = self.dev
        (dist, speeds), n = self.counted(lambda: self.model(d["images"], d["speed"], d["command"]))
        loss = moe_loss(dist, speeds, d["control"], d["target_speed"], self.ocfg.loss_coefs)
        self.opt.zero_grad()
        loss.backward()
        gn = optim.clip_grad_norm_(self.model.parameters(), 1.0, scale=False)
        self.opt.step(clip=gn)
        return loss.detach(), n


def _pair(name, dtype, calls, only=None):
    g = torch.load(GOLDEN / f"{name}.pt", weights_only=False)
    ocfg, _, model, inp = build_pair(g, dtype)
    dev = {k: v.cuda() for k, v in inp.items()}
    return (_Run(copy.deepcopy(model), ocfg, dev, calls, False, only), _Run(copy.deepcopy(model), ocfg, dev, calls, True, only))


def _same_state(plain, packs, what):
    for (n, a), (_, b) in zip(plain.model.named_parameters(), packs.model.named_parameters()):
        assert torch.equal(a, b), (what, n)
    # both copies pack now what their next forward would: as many calls as ever for the plain one, none for the other where
    # the optimizer has kept its packs current
    _, repacked = plain.counted(plain.eng._pack_all)
    _, needed = packs.counted(packs.eng._pack_all)
    assert plain.eng.replay_key() != () and len(_banks(plain.eng)) == len(_banks(packs.eng))
    for i, (a, b) in enumerate(zip(_banks(plain.eng), _banks(packs.eng))):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), (what, i, plain.eng.all_convs[i // 4].name)
    return repacked, needed


@pytest.mark.parametrize("name,dtype", [("g1_moe_e4_b2_128", F32), ("g4_moealt_e4_b2_64", F32), ("g6_moeshared_k4_b6_96", F32),
                                        ("g1_moe_e4_b2_128", BF)], ids=["g1-f32", "g4-f32", "g6-f32", "g1-bf16"])
def test_training_with_packs_is_bit_identical_and_packs_nothing(name, dtype, pack_calls):
    """Three iterations of forward + moe_loss + backward + clip + step on two deep copies, one with ``packs=model``: losses,
    parameters and every packed bank equal; the ``packs=`` model makes no pack call from its second forward on, the plain one
    as many as ever.  (Fails without the feature: FusedAdam takes no ``packs``.)"""
    plain, packs = _pair(name, dtype, pack_calls)
    full = None
    for k in range(3):
        key_before = packs.eng.replay_key()
        (la, _), (lb, nb) = plain.iteration(), packs.iteration()
        assert torch.equal(la, lb), (k, la.item(), lb.item())
        if k == 0:
            full = nb
            assert full >= len(packs.eng.all_convs) > 0
        else:
            assert nb == 0, (k, nb)
        assert packs.eng.replay_key() != key_before            # a recorded chain still sees that the weights changed
        assert packs.eng._packed_version == packs.eng.param_version()
        assert _same_state(plain, packs, k) == (full, 0)       # the plain model repacks everything, every step


def _currency(name, dtype, calls, event, only=None, expect_after=None):
    """three iterations; ``event(run)`` happens on both copies after the first one.  -> per iteration, the pack calls of the
    ``packs=`` model (in its forward, and after its step to make its packs current again); losses, parameters and banks equal
    those of the plain copy throughout"""
    plain, packs = _pair(name, dtype, calls, only)
    seen = []
    for k in range(3):
        (la, _), (lb, nb) = plain.iteration(), packs.iteration()
        assert torch.equal(la, lb), (k, la.item(), lb.item())
        repacked, needed = _same_state(plain, packs, k)
        assert repacked > 0
        seen.append((nb, needed))
        if k == 0 and event is not None:
            event(plain)
            event(packs)
    return seen


def test_currency_parameter_changed_in_place(pack_calls):
    def event(run):
        with torch.no_grad():
            next(p for n, p in run.model.named_parameters() if "layer2.0.conv1.weight" in n).mul_(1.03125)
    seen = _currency("g4_moealt_e4_b2_64", F32, pack_calls, event)
    full = seen[0][0]
    assert full > 0 and seen == [(full, 0), (full, 0), (0, 0)], seen     # the change forces one full repack, then current again


def test_currency_optimizer_with_the_head_parameters_only(pack_calls):
    seen = _currency("g4_moealt_e4_b2_64", F32, pack_calls, None, only="action_pred")
    full = seen[0][0]
    assert full > 0 and seen == [(full, full), (0, full), (0, full)], seen      # it never claims: a full repack after every step


def test_currency_load_state_dict(pack_calls):
    def event(run):
        run.model.load_state_dict(copy.deepcopy(run.model.state_dict()))
    seen = _currency("g4_moealt_e4_b2_64", F32, pack_calls, event)
    full = seen[0][0]
    assert full > 0 and seen == [(full, 0), (full, 0), (0, 0)], seen


def test_currency_compute_dtype_switch(pack_calls):
    """the banks are built again in the other dtype: the step after the switch writes into the NEW banks (its table is keyed on
    them), never into the freed ones"""
    def event(run):
        run.model.compute_dtype = BF
    seen = _currency("g4_moealt_e4_b2_64", F32, pack_calls, event)
    full = seen[0][0]
    assert full > 0 and seen == [(full, 0), (full, 0), (0, 0)], seen


def test_currency_fp8_policy(pack_calls):
    def event(run):
        run.model.fp8_weights = True
    seen = _currency("g10_moe_e4_b32_64", BF, pack_calls, event)
    full, f8 = seen[0][0], seen[1][0]
    assert full > 0 and f8 > 0 and seen == [(full, 0), (f8, f8), (0, f8)], seen  # fp8 on: not eligible, a full repack per step
