"""pmoe_amd.infer.PolicyTick: the closed-loop tick of every model type against ``model.sample`` on the stacked history, the two
kernels under it (history push, device-side mixture draw) against their statements.  Bit-identity is ``torch.equal``: the tick
reaches the same kernels on the same shapes as the full call for every launch it keeps."""
import collections
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"


# ------------------------------------------------------------------------------------------------ the draw, restated in numpy
_M1, _M2, _M3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def hash_uniform(seed, idx):
    """csrc/common.h:hash_uniform in 64-bit integer arithmetic (wrapping): uniform f32 in [0, 1), a multiple of 2^-24"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.asarray(idx, dtype=np.uint64) * _M1
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def restated_draw(probs, mean, std, seed, done, ft=np.float32):
    """The rule of include/pmoe_hip.h:pmoe_mixture_draw for launch number ``done``: probs [B,E], mean / std [B,E,2].
    ``ft``: the float type of the running sums and the threshold (f32 is the statement; f64 measures how often f32 rounding could
    decide a component).  -> component [B], action [B,2] (f64), z [B,2], margin [B] = distance of the threshold to the nearest
    cumulative edge."""
    B, E = probs.shape
    with np.errstate(over="ignore"):
        ctr = (np.uint64(done) * np.uint64(B) + np.arange(B, dtype=np.uint64)) * np.uint64(4)
    u0, u1, u2 = (hash_uniform(seed, ctr + np.uint64(i)) for i in range(3))
    p = probs.astype(ft)
    cum = np.empty((B, E), dtype=ft)
    run = np.zeros(B, dtype=ft)
    for k in range(E):                                  # accumulated in index order, in ft
        run = (run + p[:, k]).astype(ft)
        cum[:, k] = run
    thr = (u0.astype(ft) * cum[:, -1]).astype(ft)
    over = cum > thr[:, None]
    comp = np.where(over.any(1), over.argmax(1), E - 1)
    margin = np.abs(cum.astype(np.float64) - thr.astype(np.float64)[:, None]).min(1)
    r = np.sqrt(-2.0 * np.log((np.float32(1.0) - u1).astype(np.float64)))
    ang = (np.float32(6.28318530717958647692) * u2).astype(np.float64)
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    rows = np.arange(B)
    action = mean[rows, comp].astype(np.float64) + std[rows, comp].astype(np.float64) * z
    return comp, action, z, margin


DRAW_B, DRAW_E, DRAW_LAUNCHES, DRAW_SEED = 64, 4, 1024, 0x5EED0123456789AB
EDGE, MAX_EXCLUDED = 1e-6, 1e-3


def draw_inputs():
    """probs {0.1, 0.2, 0.3, 0.4} permuted per row, means in [-1, 1], stds in [0.05, 0.5] (fixed generator)"""
    rng = np.random.default_rng(20261017)
    base = np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32)
    probs = np.stack([rng.permutation(base) for _ in range(DRAW_B)])
    mean = rng.uniform(-1.0, 1.0, (DRAW_B, DRAW_E, 2)).astype(np.float32)
    std = rng.uniform(0.05, 0.5, (DRAW_B, DRAW_E, 2)).astype(np.float32)
    return probs, mean, std


def restated_all(ft=np.float32):
    probs, mean, std = draw_inputs()
    outs = [restated_draw(probs, mean, std, DRAW_SEED, c, ft) for c in range(DRAW_LAUNCHES)]
    return tuple(np.stack([o[i] for o in outs]) for i in range(4))          # [launch, B, ...]


# ------------------------------------------------------------------------------------------------ models from the goldens
def _punet_model(tmp, name, dtype, exclude_freeze=()):
    from tests.punet_parity import build_pair
    g = torch.load(GOLDEN / f"{name}.pt", weights_only=False)
    _, _, model, inp = build_pair(tmp, g, dtype, exclude_freeze=exclude_freeze)
    return model.eval(), g["meta"], {k: v.cuda().float().contiguous() for k, v in inp.items()}


def _moe_model(name, dtype):
    from tests.parity_util import build_pair
    g = torch.load(GOLDEN / f"{name}.pt", weights_only=False)
    _, _, model, inp = build_pair(g, dtype)
    return model.eval(), g["meta"], {k: v.cuda().float().contiguous() for k, v in inp.items()}


class _History:
    """the agent's deque (image_agent.py:63-64,136,158) on the host: T zero frames, then one frame per tick"""

    def __init__(self, T, B, H, W, seed):
        self.q = collections.deque([torch.zeros(B, 3, H, W) for _ in range(T)], maxlen=T)
        self.gen = torch.Generator().manual_seed(seed)
        self.shape = (B, 3, H, W)

    def step(self):
        frame = torch.rand(self.shape, generator=self.gen)
        self.q.append(frame)
        return frame.cuda().contiguous(), torch.stack(list(self.q), 1).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ tick == stack
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", ["p2_punet_b1_64_f6_eval", "p3_punetinter_b2_64_f2"])
def test_tick_equals_stack_deterministic_models(tmp_path, name, dtype):
    """punet / punet_inter: every tick (the first after reset() included) equals model.sample on the stacked history bit for bit,
    in both modes; an eager tick runs 1 + F U-Net passes where the full call runs T + F."""
    from pmoe_amd.infer import PolicyTick
    model, meta, dev = _punet_model(tmp_path, name, dtype)
    B, S, F_ = meta["batch"], meta["size"], meta["future_frames"]
    eng = model._engine()
    for mode in ("eager", "plan"):
        tick = PolicyTick(model, batch=B, height=S, width=S, mode=mode)
        T = tick.T
        hist = _History(T, B, S, S, seed=11)
        for i in range(T + 3):
            frame, stack = hist.step()
            eng.debug_pass_out = []
            got = tick(frame, dev["speed"], dev["command"]).clone()
            n_tick = len(eng.debug_pass_out)
            eng.debug_pass_out = []
            with torch.no_grad():
                ref, ref_speed = model(stack, dev["speed"], dev["command"])
                assert torch.equal(model.sample(stack, dev["speed"], dev["command"]), ref)
            n_full = len(eng.debug_pass_out) // 2
            eng.debug_pass_out = None
            assert torch.equal(got, ref), (mode, i, (got - ref).abs().max().item())
            assert torch.equal(tick.last.punet_actions, ref) and torch.equal(tick.last.pred_speed, ref_speed)
            assert tick.last.raw is None and tick.last.probs is None
            assert n_full == T + F_
            if mode == "eager":
                assert n_tick == 1 + F_, (n_tick, F_)
        if mode == "plan":
            assert len(tick.plan.calls) > 50
        # a new episode: the history is zeros again, the first tick equals the stack of T - 1 zero frames and the frame
        tick.reset()
        hist = _History(T, B, S, S, seed=12)
        frame, stack = hist.step()
        with torch.no_grad():
            ref = model.sample(stack, dev["speed"], dev["command"])
        assert torch.equal(tick(frame, dev["speed"], dev["command"]), ref)
    # the engine's own calls, without PolicyTick: the masks mask_of makes frame by frame, then forward_cached, against forward on
    # the stacked frames
    from pmoe_amd import ops
    from pmoe_amd.engine import r16
    pu = model.punet
    hist = _History(T, B, S, S, seed=13)
    for _ in range(T):
        frame, stack = hist.step()
    with torch.no_grad():
        eng, dt, _ = model.resolve_engine()
        assert dt == dtype
        eng.prepare_cached(stack, dt)
        ring = torch.zeros(1, T, B, S, S, r16(pu.num_classes), dtype=dt, device="cuda")
        newest = torch.zeros(B, S, S, r16(pu.in_features), dtype=dt, device="cuda")
        for t in range(T):                               # on entry slots 1..T-1 hold the older frames' masks, oldest first
            ops.nchw_to_nhwc(stack[:, t].contiguous(), newest)
            mask = eng.mask_of(stack, newest, dt).clone()
            if t < T - 1:
                ring[0, t + 1].copy_(mask)
        got, got_speed = eng.forward_cached(stack, newest, ring, dev["speed"], dev["command"], dt)
        assert torch.equal(ring[0, T - 1], mask)         # the newest frame's mask: the one pass forward_cached runs itself
        ref, ref_speed = model(stack, dev["speed"], dev["command"])
    assert torch.equal(got, ref) and torch.equal(got_speed, ref_speed)


def _check_mixture_tick(model, moe, dev, B, S, with_punet):
    from pmoe_amd.infer import PolicyTick
    for mode in ("eager", "plan"):
        tick = PolicyTick(model, batch=B, height=S, width=S, mode=mode, seed=5)
        hist = _History(tick.T, B, S, S, seed=21)
        for i in range(tick.T + 1):
            frame, stack = hist.step()
            got = tick(frame, dev["speed"], dev["command"]).clone()
            last = tick.last
            with torch.no_grad():
                ref = moe.mixture_params(stack, dev["speed"], dev["command"])
                for a, b, k in zip((last.probs, last.mean, last.std, last.speeds), ref, ("probs", "mean", "std", "speeds")):
                    assert torch.equal(a, b), (mode, i, k)
                if with_punet:
                    pa = model.punet(stack, dev["speed"], dev["command"])[0]
                    assert torch.equal(last.punet_actions, pa), (mode, i)
                    assert torch.equal(got, model.blend(last.raw, pa)), (mode, i)
                else:
                    assert torch.equal(got, last.raw)
            assert got.shape == (B, 2) and got.dtype == torch.float32 and torch.isfinite(got).all()
        assert tick.draws_done == tick.T + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g2_moe_e4_b1_224_eval", "g7_moeshared_k6_b1_224_eval", "g4_moealt_e4_b2_64"])
def test_tick_equals_stack_mixtures(name):
    """moe / moe_shared at the agent's shape, moe_alt (the kind of mixture PMoE holds) at its golden's: the tick's mixture
    parameters equal mixture_params on the stacked history"""
    model, meta, dev = _moe_model(name, torch.bfloat16)
    _check_mixture_tick(model, model, dev, meta["batch"], meta["size"], with_punet=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_tick_equals_stack_pmoe(tmp_path, dtype):
    """pmoe: mixture parameters, the PU-Net expert's actions and the blend of the raw draw, all bit for bit"""
    model, meta, dev = _punet_model(tmp_path, "p5_pmoe_e2_b2_64_f2", dtype, exclude_freeze=["lat_weights", "long_weights"])
    _check_mixture_tick(model, model.moe, dev, meta["batch"], meta["size"], with_punet=True)


# ------------------------------------------------------------------------------------------------ plan hygiene
@pytest.mark.gpu
def test_plan_survives_allocations_and_notices_weight_and_dtype_changes(tmp_path):
    """mirrors test_planned_inference_replays_the_recorded_launches on the PU-Net tick: private pool, automatic refresh after a
    weight change (the masks of the three older frames included) and after a compute-dtype round trip"""
    from pmoe_amd.infer import PolicyTick
    model, meta, dev = _punet_model(tmp_path, "p2_punet_b1_64_f6_eval", torch.bfloat16)
    B, S = meta["batch"], meta["size"]
    tick = PolicyTick(model, batch=B, height=S, width=S, mode="plan")
    hist = _History(tick.T, B, S, S, seed=31)

    def step():
        frame, stack = hist.step()
        got = tick(frame, dev["speed"], dev["command"]).clone()
        with torch.no_grad():
            ref = model.sample(stack, dev["speed"], dev["command"])
        return got, ref
    for _ in range(tick.T):
        got, ref = step()
        assert torch.equal(got, ref)
    plan = tick.plan
    junk = [torch.full((1 << 20,), float(i), device="cuda") for i in range(8)]       # would land in the plan's buffers if they were free
    got, ref = step()
    assert torch.equal(got, ref) and tick.plan is plan
    del junk
    with torch.no_grad():
        for p_ in model.parameters():
            p_.mul_(1.01)
    got, ref3 = step()                                   # no explicit refresh(): the masks of the older frames are recomputed too
    assert tick.plan is not plan and torch.equal(got, ref3)
    plan = tick.plan
    model.compute_dtype = torch.float32
    with torch.no_grad():
        model.sample(torch.zeros(B, tick.T, 3, S, S, device="cuda"), dev["speed"], dev["command"])
        model.compute_dtype = torch.bfloat16
        model.sample(torch.zeros(B, tick.T, 3, S, S, device="cuda"), dev["speed"], dev["command"])
    got, ref = step()                                    # every packed bank was re-allocated twice in between
    assert tick.plan is not plan and torch.equal(got, ref)
    model.compute_dtype = torch.float32                  # ... and a switch nobody has run yet
    got, ref = step()
    assert torch.equal(got, ref)
    with pytest.raises(ValueError, match="frame"):
        tick(torch.zeros(B, 3, S, S // 2, device="cuda"), dev["speed"], dev["command"])
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        tick(torch.zeros(B, 3, S, S, device="cuda"), dev["speed"], dev["command"])


# ------------------------------------------------------------------------------------------------ replay key
def _check_replay_key(host, dev, changes):
    """host.eval() forward -> replay_key() is stable over a second forward; after each of ``changes`` (name, callable) and one
    forward it is another key, and stable again"""
    def run():
        with torch.no_grad():
            host(dev["images"], dev["speed"], dev["command"])
        return host._engine().replay_key()
    key = run()
    assert run() == key
    for name, change in changes:
        with torch.no_grad():
            change()
        new = run()
        assert new != key, name
        assert run() == new, name
        key = new


def _dtype_switch(model):
    def change():
        model.compute_dtype = torch.float32 if model.compute_dtype == torch.bfloat16 else torch.bfloat16
    return change


def _fp8_toggle(host):
    def change():
        host.fp8_weights = not host.fp8_weights
    return change


def _punet_changes(model, host):
    pu = host.punet
    up = pu.pred_unet.up_2

    def new_storage():
        up.weight.data = up.weight.data.clone()
    return [("parameter", lambda: host.action_pred[1].weight.mul_(1.01)),
            ("frozen parameter", lambda: pu.unet.dwn_1[0].weight.mul_(1.01)),
            ("running buffer", lambda: pu.unet.dwn_3[1].running_mean.add_(0.01)),
            ("running buffer behind a shadow", lambda: pu.entry_block.layer2.conv2[1].running_var.mul_(1.01)),
            ("compute dtype", _dtype_switch(model)), ("compute dtype back", _dtype_switch(model)),
            ("ConvTranspose2d weight storage", new_storage)]


def _mixture_changes(model, host):
    bb = host.moe[0].backbone
    return [("parameter", lambda: host.moe[1].action_pred.weight.mul_(1.01)),
            ("running buffer", lambda: bb.layer2[0].bn1.running_var.mul_(1.01)),
            ("compute dtype", _dtype_switch(model)), ("compute dtype back", _dtype_switch(model)),
            ("fp8_weights on", _fp8_toggle(host)), ("fp8_weights off", _fp8_toggle(host))]


@pytest.mark.gpu
def test_replay_key_punet(tmp_path):
    model, meta, dev = _punet_model(tmp_path, "p2_punet_b1_64_f6_eval", torch.bfloat16)
    _check_replay_key(model, dev, _punet_changes(model, model))


@pytest.mark.gpu
def test_replay_key_mixture():
    model, meta, dev = _moe_model("g4_moealt_e4_b2_64", torch.bfloat16)
    _check_replay_key(model, dev, _mixture_changes(model, model))


@pytest.mark.gpu
def test_replay_key_pmoe(tmp_path):
    """both engines of a PMoE, each under the switches of the whole model (``PMoE.compute_dtype`` sets both halves)"""
    model, meta, dev = _punet_model(tmp_path, "p5_pmoe_e2_b2_64_f2", torch.bfloat16, exclude_freeze=["lat_weights", "long_weights"])
    _check_replay_key(model.punet, dev, _punet_changes(model, model.punet))
    _check_replay_key(model.moe, dev, _mixture_changes(model, model.moe))


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.gpu
def test_draws_are_fresh_and_reproducible():
    from pmoe_amd.infer import PolicyTick
    model, meta, dev = _moe_model("g2_moe_e4_b1_224_eval", torch.bfloat16)
    B, S = meta["batch"], meta["size"]
    runs = {}
    for mode in ("plan", "eager"):
        tick = PolicyTick(model, batch=B, height=S, width=S, mode=mode, seed=1)
        frame = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(3)).cuda()
        a, pa = tick(frame, dev["speed"], dev["command"]).clone(), tick.last.probs.clone()
        tick.frames.zero_()                              # identical inputs: the same (empty) history in front of the same frame
        b = tick(frame, dev["speed"], dev["command"]).clone()
        assert torch.equal(tick.last.probs, pa) and not torch.equal(a, b), mode
        assert tick.draws_done == 2
        seqs = []
        for _ in range(2):
            tick.reseed(77)
            tick.reset()
            hist = _History(tick.T, B, S, S, seed=41)
            seqs.append([tick(hist.step()[0], dev["speed"], dev["command"]).clone() for _ in range(tick.T + 2)])
            assert tick.draws_done == tick.T + 2
        for x, y in zip(*seqs):
            assert torch.equal(x, y), mode
        runs[mode] = seqs[0]
    for x, y in zip(runs["plan"], runs["eager"]):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_draw_kernel_against_its_statement():
    """65 536 draws (B = 64, E = 4, 1024 launches of ops.mixture_draw on one device-resident state) against restated_draw:
    exact component wherever f32 rounding cannot decide it, actions to a few dozen f32 ulps (the device's logf / cosf / sinf are
    not numpy's; nothing else differs), component frequencies and per-component moments within 4 standard deviations."""
    from pmoe_amd import ops
    probs, mean, std = draw_inputs()
    comp, action, z, margin = restated_all()
    d = [torch.from_numpy(a).cuda() for a in (probs, mean, std)]
    seed = DRAW_SEED - (1 << 64) if DRAW_SEED >> 63 else DRAW_SEED
    state = torch.tensor([seed, 0], dtype=torch.int64).cuda()
    raw = torch.zeros(DRAW_LAUNCHES, DRAW_B, 2, device="cuda")
    for c in range(DRAW_LAUNCHES):
        ops.mixture_draw(d[0], d[1], d[2], state, raw[c])
    assert state.tolist() == [seed, DRAW_LAUNCHES]
    got = raw.cpu().numpy().astype(np.float64)                                  # [launch, B, 2]
    rows = np.arange(DRAW_B)
    # the component the device took: the one whose mean + std * z is nearest to what it returned
    cand = mean[None].astype(np.float64) + std[None].astype(np.float64) * z[:, :, None, :]      # [launch, B, E, 2]
    dev_comp = np.abs(cand - got[:, :, None, :]).sum(-1).argmin(-1)
    safe = margin > EDGE
    print("excluded draws:", int((~safe).sum()), "of", safe.size, " component mismatches on the rest:",
          int((dev_comp != comp)[safe].sum()))
    assert (~safe).mean() <= MAX_EXCLUDED
    assert np.array_equal(dev_comp[safe], comp[safe])
    m_k, s_k = mean[rows[None], dev_comp].astype(np.float64), std[rows[None], dev_comp].astype(np.float64)
    z_dev = (got - m_k) / s_k
    same = dev_comp == comp
    bound = 1e-5 * (np.abs(m_k) + s_k * (1.0 + np.abs(z)))
    err = np.abs(got - action)
    print("worst |action - restated| / bound:", float((err / bound)[same].max()))
    assert (err <= bound)[same].all()
    n = float(safe.size)
    for v in (0.1, 0.2, 0.3, 0.4):                       # rows grouped by the probability of the component they took
        hits = float((np.abs(probs[rows[None], dev_comp] - v) < 1e-3).sum())
        sd = (n * v * (1.0 - v)) ** 0.5
        print(f"p = {v}: {hits:.0f} draws, expected {n * v:.0f} +- {sd:.1f}")
        assert abs(hits - n * v) <= 4.0 * sd
    for k in range(DRAW_E):
        for axis in range(2):
            zs = z_dev[..., axis][dev_comp == k]
            m, var, cnt = zs.mean(), zs.var(), zs.size
            print(f"component {k} axis {axis}: n = {cnt}, mean {m:+.4f}, variance {var:.4f}")
            assert abs(m) <= 4.0 / cnt ** 0.5                                   # standard error of the mean of N(0, 1)
            assert abs(var - 1.0) <= 4.0 * (2.0 / cnt) ** 0.5                   # ... and of its variance


@pytest.mark.gpu
def test_draw_with_blend_equals_blend_fwd():
    from pmoe_amd import ops
    g = torch.Generator().manual_seed(9)
    B, E = 37, 3
    probs = torch.softmax(torch.randn(B, E, generator=g), 1).cuda()
    mean, std = torch.randn(B, E, 2, generator=g).cuda(), (torch.rand(B, E, 2, generator=g) + 0.1).cuda()
    pu = torch.tanh(torch.randn(B, 2, generator=g)).cuda()
    lin = [torch.randn(s, generator=g).cuda() for s in ((1, 2), (1,), (1, 2), (1,))]
    state = torch.tensor([123, 7], dtype=torch.int64).cuda()
    raw, out, ref = (torch.zeros(B, 2, device="cuda") for _ in range(3))
    ops.mixture_draw(probs, mean, std, state, raw, pu, tuple(lin), out)
    ops.blend_fwd(raw, pu, *lin, ref, B)
    assert torch.equal(out, ref) and state.tolist() == [123, 8]
    raw2 = torch.zeros_like(raw)
    state.copy_(torch.tensor([123, 7]))
    ops.mixture_draw(probs, mean, std, state, raw2)
    assert torch.equal(raw, raw2)                        # the blend is optional and does not change the draw


# ------------------------------------------------------------------------------------------------ push
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_history_push_equals_a_rolled_host_ring(dtype):
    """T + 2 pushes of the frame ring (f32 [B,T,3,H,W] + the NHWC copy in ``dtype``) and of a mask ring (``dtype`` [1,T,B,H,W,32])
    against torch.roll on the host; B = 3 pins the per-row slot stride"""
    from pmoe_amd import ops
    gen = torch.Generator().manual_seed(17)
    for T in (1, 2, 4):
        for B in (1, 3):
            for H, W in ((32, 32), (64, 48)):
                ring = torch.rand(B, T, 3, H, W, generator=gen)
                host = ring.clone()
                ring = ring.cuda()
                mring = torch.rand(1, T, B, H, W, 32, generator=gen).to(dtype)
                mhost = mring.clone()
                mring = mring.cuda()
                nhwc = torch.full((B, H, W, 16), 7.0, dtype=dtype, device="cuda")
                for _ in range(T + 2):
                    frame = torch.rand(B, 3, H, W, generator=gen)
                    host = torch.roll(host, -1, 1)
                    host[:, -1] = frame
                    ops.history_push(ring, frame.cuda(), nhwc=nhwc)
                    ref = torch.empty_like(nhwc)
                    ops.nchw_to_nhwc(frame.cuda(), ref)
                    assert torch.equal(ring.cpu(), host), (T, B, H, W)
                    assert torch.equal(nhwc, ref), (T, B, H, W)
                    item = torch.rand(1, B, H, W, 32, generator=gen).to(dtype)
                    mhost = torch.roll(mhost, -1, 1)
                    mhost[:, -1] = item
                    ops.history_push(mring, item.cuda())
                    assert torch.equal(mring.cpu(), mhost), (T, B, H, W)
    # an odd row length takes the element-wise form of the same walk
    ring = torch.rand(2, 3, 5, 7, generator=gen)
    host, ring = ring.clone(), ring.cuda()
    item = torch.rand(2, 5, 7, generator=gen)
    ops.history_push(ring, item.cuda())
    host = torch.roll(host, -1, 1)
    host[:, -1] = item
    assert torch.equal(ring.cpu(), host)
    with pytest.raises(ValueError, match="history_push"):
        ops.history_push(ring, torch.zeros(2, 5, 8, device="cuda"))
