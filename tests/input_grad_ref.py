"""float64 restatement of the two input-gradient formulas (csrc/input_grad.hip), written from the formulas and evaluated with
torch on whatever device the operands live on.

Stem.  The frames x[b] (C real channels) are shared by the E experts; expert e computes
    gate_e = sigmoid(conv1d(GAP(x))),      z1_e = conv3x3(x * gate_e, W_e)      (stride 1, pad 1, Co output channels)
and with dz1_e the gradient of z1_e

    dx[b,c,h,w] = sum_e ( gate_e[b,c] * sum_{r,s,co} dz1[e,b,h+1-r,w+1-s,co] * W_e[co,c,r,s]  +  dgap_e[b,c] / (H W) )

where dgap_e is the gradient that reaches the gate's pooled input.  The kernel reads the products ``wg = gate * W`` from a pack in
its storage dtype and ``dgap / (H W)`` as one f32 operand, so the restatement takes exactly those two.

Shared Linear.  speed / command rows are shared too:  dx[b,j] = sum_e sum_o dh[e,b,o] * W_e[o,j].

Tensors here: dz1 [E,B,H,W,Co], w [E,Co,C,3,3], gate [E,B,C], wg [E,B,Co,C,3,3], dgap_hw [E,B,C], dh [E,B,O], wl [E,O,J]."""
import torch

F64 = torch.float64
EPS24 = 2.0 ** -24


def gated(w, gate):
    """wg[e,b,co,c,r,s] = gate_e[b,c] * W_e[co,c,r,s]"""
    return w.to(F64)[:, None] * gate.to(F64)[:, :, None, :, None, None]


def _shift(t, dr, ds):
    """u[..., h, w, :] = t[..., h + dr, w + ds, :], zero outside the map"""
    H, W = t.shape[-3], t.shape[-2]
    u = torch.zeros_like(t)
    hs, he = max(0, -dr), min(H, H - dr)
    ws, we = max(0, -ds), min(W, W - ds)
    if hs < he and ws < we:
        u[..., hs:he, ws:we, :] = t[..., hs + dr:he + dr, ws + ds:we + ds, :]
    return u


def stem_input_grad(dz1, wg, dgap_hw=None, absolute=False):
    """-> dx [B,C,H,W] float64; ``absolute``: the sum of the absolute values of the same terms (the error bound's scale)"""
    f = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    dz, g = f(dz1), f(wg)
    E, B, H, W, Co = dz.shape
    dx = torch.zeros(B, g.shape[3], H, W, dtype=F64, device=dz.device)
    for r in range(3):
        for s in range(3):
            dx += torch.einsum("ebhwo,eboc->bchw", _shift(dz, 1 - r, 1 - s), g[..., r, s])
    if dgap_hw is not None:
        dx += f(dgap_hw).sum(0)[:, :, None, None]
    return dx


def stem_terms(E, Co=64):
    """K of the bound: the products summed per output element"""
    return E * 9 * Co


def gate_of(x, w1d):
    """x [B,C,H,W], w1d [E,k] -> (gate [E,B,C], pooled [B,C]): sigmoid of the k-tap cross-correlation over channels (zero padded)"""
    gap = x.to(F64).mean((2, 3))
    k = w1d.shape[1]
    pad = k // 2
    gp = torch.nn.functional.pad(gap, (pad, pad))
    pre = torch.stack([sum(w1d[e, t].to(F64) * gp[:, t:t + gap.shape[1]] for t in range(k)) for e in range(w1d.shape[0])])
    return torch.sigmoid(pre), gap


def dgap_of(x, w, w1d, gate, dz1):
    """the gradient reaching the pooled input of each expert's gate, [E,B,C]: with u_e = conv^T(dz1_e, W_e) (ungated),
    ds = sum_hw x * u_e,  dpre = ds * gate (1 - gate),  dgap[c'] = sum_t dpre[c' - t + pad] * w1d[t]"""
    E, B, H, W, Co = dz1.shape
    C = w.shape[2]
    ones = torch.ones(E, B, C, dtype=F64, device=dz1.device)
    dgap = torch.zeros(E, B, C, dtype=F64, device=dz1.device)
    k = w1d.shape[1]
    pad = k // 2
    for e in range(E):
        u = stem_input_grad(dz1[e:e + 1], gated(w[e:e + 1], ones[e:e + 1]))          # [B,C,H,W]
        ds = (x.to(F64) * u).sum((2, 3))
        dpre = ds * gate[e] * (1 - gate[e])
        dp = torch.nn.functional.pad(dpre, (pad, pad))
        for t in range(k):
            # pre[c] takes gap[c + t - pad] * w1d[t]  ->  dgap[c'] takes dpre[c' - t + pad] * w1d[t]
            dgap[e] += w1d[e, t].to(F64) * dp[:, 2 * pad - t:2 * pad - t + C]
    return dgap


def shared_linear_input_grad(dh, wl, absolute=False):
    f = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    return torch.einsum("ebo,eoj->bj", f(dh), f(wl))


# ---- dyadic lattices: every product and every partial sum is an exact f32 (and the operands exact bf16), so any summation
# order gives the float64 result bit for bit.  dz1 in k/4 (|k| <= 8), W in k/8 (|k| <= 7), gate in {1,2,3,4}/4: gate * W has a
# numerator of at most 28 over 32 (6 bits: exact in bf16), a product is a multiple of 1/128 below 1.75
LATTICE_UNIT = 1.0 / 128


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


def lattice_stem(seed, E, B, H, W, C, Co=64):
    g = torch.Generator().manual_seed(seed)
    return dict(dz1=_ints(g, (E, B, H, W, Co), 8) / 4, w=_ints(g, (E, Co, C, 3, 3), 7) / 8,
                gate=torch.randint(1, 5, (E, B, C), generator=g).to(F64) / 4, dgap_hw=_ints(g, (E, B, C), 16) / 8)


def random_stem(seed, E, B, H, W, C, Co=64):
    g = torch.Generator().manual_seed(seed)
    return dict(dz1=torch.randn(E, B, H, W, Co, generator=g, dtype=F64), w=torch.randn(E, Co, C, 3, 3, generator=g, dtype=F64) / 8,
                gate=torch.rand(E, B, C, generator=g, dtype=F64), dgap_hw=torch.randn(E, B, C, generator=g, dtype=F64) / 4)


def lattice_linear(seed, E, B, O, J):
    g = torch.Generator().manual_seed(seed)
    return dict(dh=_ints(g, (E, B, O), 8) / 4, wl=_ints(g, (E, O, J), 7) / 8)


def random_linear(seed, E, B, O, J):
    g = torch.Generator().manual_seed(seed)
    return dict(dh=torch.randn(E, B, O, generator=g, dtype=F64), wl=torch.randn(E, O, J, generator=g, dtype=F64) / 8)


STEM_SHAPES = [(E, B, H, W, C) for E in (1, 3) for B in (1, 2) for H, W in ((16, 16), (17, 19), (5, 40)) for C in (12, 3)]
LINEAR_SHAPES = [(E, B, O, J) for E in (1, 3) for B in (1, 2, 5) for O, J in ((128, 1), (128, 4), (20, 6))]


def largest_partial_sum(d):
    """an upper bound, in lattice units, on |any partial sum| of the stem lattice data ``d``, whatever the order"""
    top = stem_input_grad(d["dz1"], gated(d["w"], d["gate"]), d["dgap_hw"], absolute=True).max().item()
    return top / LATTICE_UNIT
