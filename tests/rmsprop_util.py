"""What the FusedRMSprop tests share: shapes, the gradient schedule, the cases, the float64 yardstick and the bounds.

The yardstick is ``torch.optim.RMSprop(foreach=False)`` in float64 on the CPU, fed the same (float32) gradients.

The gradient schedule starts with the LARGE gradients (3.0 on even steps, 0.01 on odd ones), the other way round from
tests/test_optim_gpu.py, and the order matters: under weight decay the first update is g' / (0.0995 |g'| + eps) with
g' = g + wd * p, and with |g| ~ 0.01 next to |wd * p| ~ 0.005 the sum cancels -- float32 then cannot know the SIGN of g' where it
is near zero, while the update has full size whatever |g'| is.  torch's own float32 RMSprop is 18x over the parameter bound on
that order; on this one two float32 implementations (torch's, and one that rounds every product and sum separately) stay at
<= 0.30 of the parameter bound and <= 0.17 of the state bound (tests/test_rmsprop_cpu.py keeps the first of those checked)."""
import torch

F32, F64 = torch.float32, torch.float64

# tests/test_optim_gpu.py:SHAPES (sizes 1, 3, 5 and 16385 columns among them) + one chunk exactly + one element short of it
SHAPES = [(64, 12, 3, 3), (64,), (1, 1, 3), (512, 1536), (5,), (70001,), (3, 16385), (512, 512, 3, 3), (16384,), (16383,)]
STEPS = 8
ALPHA, EPS = 0.99, 1e-8
# (lr, weight_decay, momentum, centered, max_norm)
CASES = [(2e-4, 0, 0, True, 1.0), (1e-3, 0.01, 0.9, True, 0), (2e-4, 0.05, 0, False, 1e4), (1e-3, 0, 0.5, False, 1.0)]
CASE_IDS = ["centered-clip", "centered-momentum-wd", "plain-wd-loose-clip", "momentum-clip"]
PARAM_RTOL, PARAM_ATOL = 1e-5, 2e-7            # the project's Adam bounds (tests/test_optim_gpu.py)
STATE_RTOL, STATE_ATOL_OF_MAX = 1e-4, 1e-5


def hyper(case):
    lr, wd, momentum, centered, _ = case
    return dict(lr=lr, alpha=ALPHA, eps=EPS, weight_decay=wd, momentum=momentum, centered=centered)


def state_keys(momentum, centered):
    """torch's per-parameter state tensors, in its order of creation"""
    return ("square_avg",) + (("momentum_buffer",) if momentum > 0 else ()) + (("grad_avg",) if centered else ())


def values(seed, shapes=SHAPES):
    """the initial parameter values: float32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * 0.1 for s in shapes]


def gradient_steps(shapes=SHAPES, seed=1, steps=STEPS):
    """-> per step a list of float32 CPU gradients, None where the parameter has none: seeded randn, scaled 3.0 on even steps
    and 0.01 on odd ones; on step 5 the first half of every gradient is exactly zero; on step 3 parameter 1 has no gradient"""
    g = torch.Generator().manual_seed(seed)
    for step in range(steps):
        grads = [torch.randn(s, generator=g) * (0.01 if step % 2 else 3.0) for s in shapes]
        if step == 5:
            for gr in grads:
                gr.view(-1)[:gr.numel() // 2] = 0.0
        if step == 3 and len(grads) > 1:
            grads[1] = None
        yield grads


class Yardstick:
    """torch.optim.RMSprop(foreach=False) in float64 on the CPU, with torch's own clip_grad_norm_ where max_norm > 0"""

    def __init__(self, case, seed=0, shapes=SHAPES):
        self.max_norm = case[4]
        self.params = [torch.nn.Parameter(v.to(F64)) for v in values(seed, shapes)]
        self.opt = torch.optim.RMSprop(self.params, foreach=False, **hyper(case))

    def step(self, grads):
        """-> the total gradient norm (None where the case does not clip)"""
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else g.to(F64)
        norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm) if self.max_norm > 0 else None
        self.opt.step()
        return norm

    def state(self, i, key):
        return self.opt.state[self.params[i]][key]


def _worst(got, want, rtol, atol):
    """max over the elements of |got - want| / (atol + rtol |want|): <= 1 is torch.testing.assert_close's criterion"""
    got, want = got.detach().to("cpu", F64), want.detach().to("cpu", F64)
    assert got.shape == want.shape
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got - want).abs() / (atol + rtol * want.abs())).max().item() if want.numel() else 0.0


def param_excess(got, want):
    """how much of the parameter bound (rtol 1e-5, atol 2e-7) the worst element uses"""
    return _worst(got, want, PARAM_RTOL, PARAM_ATOL)


def state_excess(got, want):
    """how much of the state bound (rtol 1e-4, atol 1e-5 max|want|) the worst element uses"""
    return _worst(got, want, STATE_RTOL, STATE_ATOL_OF_MAX * want.detach().abs().max().item())
