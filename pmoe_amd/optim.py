"""Fused optimizer tail of the stage-2 step -- drop-ins for the three torch calls of the
reference trainer (``trainer/train_2.py:157-165,184``; hyper-parameters ``conf/stage_2_pmoe.yaml:11,137-144``):

    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)   ->  pmoe_amd.optim.clip_grad_norm_
    torch.optim.Adam(params, lr, betas, eps, wd, amsgrad=True) ->  pmoe_amd.optim.FusedAdam   (same constructor)
    torch.optim.RMSprop(params, **cfg.rmsprop)                 ->  pmoe_amd.optim.FusedRMSprop (same constructor)
    torch.optim.swa_utils.AveragedModel(model)                 ->  pmoe_amd.optim.FusedAveragedModel

Each call is one or two HIP launches over a chunk table (``csrc/optim.hip``) instead of several launches -- and, in
``check_grad_norm`` (utils/nn.py:10-19), one ``.item()`` host sync -- per parameter tensor (620 for E=4).  The
returned gradient norm is a device tensor; nothing here synchronises with the host.  ``FusedAdam.step(clip=norm)``
consumes the clip coefficient straight from device memory, so clip + step is: 2 launches for the norm, 1 for Adam.

``FusedAdam(..., packs=model)`` (opt-in): the update of a parameter that the model's engine keeps packed also writes the
packed operands (``mt_adam_pack_kernel``), and the next forward does not pack again (DESIGN.md "Packs kept current by the
optimizer").  ``FusedRMSprop`` -- the trainers' other optimizer (train_2.py:62-73) -- takes the same ``clip`` and ``packs``;
``get_optimizer(name, params, cfg)`` is the trainers' dispatch between the two.
"""
import ctypes as C

import numpy as np
import torch

from . import hip
from .hip import check, load, stream_ptr

CHUNK = 16384                      # PMOE_OPT_CHUNK (include/pmoe_hip.h)
F32 = torch.float32


class OptTensor(C.Structure):      # pmoe_opt_tensor
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("max_exp_avg_sq", C.c_void_p), ("swa", C.c_void_p), ("numel", C.c_int64), ("bc1", C.c_float),
                ("bc2_sqrt", C.c_float)]


_ROW = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("max_exp_avg_sq", "<u8"),
                 ("swa", "<u8"), ("numel", "<i8"), ("bc1", "<f4"), ("bc2_sqrt", "<f4")])
assert _ROW.itemsize == C.sizeof(OptTensor) == 64


class OptPack(C.Structure):        # pmoe_opt_pack
    _fields_ = [("fwd", C.c_void_p), ("dgrd", C.c_void_p), ("cout", C.c_int32), ("cin", C.c_int32), ("taps", C.c_int32),
                ("dtype", C.c_int32), ("cinp", C.c_int32), ("row0", C.c_int32), ("dgrd_ld", C.c_int32), ("col0", C.c_int32),
                ("tco", C.c_int32), ("tci", C.c_int32), ("reserved", C.c_int32 * 2)]


_PACK_FIELDS = ("fwd", "dgrd", "cout", "cin", "taps", "dtype", "cinp", "row0", "dgrd_ld", "col0")     # a sink, in this order
_PACK_ROW = np.dtype([("fwd", "<u8"), ("dgrd", "<u8")] + [(k, "<i4") for k in _PACK_FIELDS[2:] + ("tco", "tci")]
                     + [("reserved", "<i4", (2,))])
assert _PACK_ROW.itemsize == C.sizeof(OptPack) == 64
PACK_STAGE = 4640                  # PMOE_OPT_PACK_STAGE: floats of LDS one tile may take


def pack_tile_dims(cout, cin, taps):
    """Tile extents (tco, tci) of mt_adam_pack_kernel for a [cout][cin][taps] tensor; a tile is tco x tci channels x all taps.

    The forward operand is contiguous along ci and the data-gradient operand along co, so a tile stores runs of tci elements
    into the one and of tco elements into the other: both extents are >= 16 (32 bytes of bf16) wherever the layer has that
    many channels.  tci * taps is about 288 floats (32 channels of a 3x3 filter, 288 of a 1x1): with 16 rows that is a tile of
    ~4.6 K elements, 18 KB of LDS.  A tensor narrower than tci (a bias, the stem) takes more rows instead, in steps of 16; a
    filter so large that 16 rows of 16 channels do not fit the stage takes fewer rows."""
    if min(cout, cin, taps) < 1:
        raise ValueError("pack_tile_dims: empty tensor")
    tci = max(16, 288 // taps // 16 * 16)
    stride = (min(tci, cin) * taps) | 1                    # LDS row stride of a full-width tile
    if stride > PACK_STAGE:
        raise ValueError(f"pack_tile_dims: a {taps}-tap filter does not fit the LDS stage")
    fit = PACK_STAGE // stride
    tco = min(fit, max(16, 4096 // (min(tci, cin) * taps)))
    tco = tco // 16 * 16 if tco >= 16 else 1 << (tco.bit_length() - 1)
    return tco, tci


def pack_tiles(shapes):
    """The (tensor, co0, ci0) tile table of ``shapes`` = [(cout, cin, taps), ...] -> (dims, tensor, co0, ci0): dims[t] = (tco,
    tci) of tensor t and three equally long lists, one entry per workgroup.  Every tile lies inside its tensor and the tiles of
    a tensor partition it."""
    dims, tt, c0, i0 = [], [], [], []
    for t, (cout, cin, taps) in enumerate(shapes):
        tco, tci = pack_tile_dims(cout, cin, taps)
        dims.append((tco, tci))
        for co0 in range(0, cout, tco):
            for ci0 in range(0, cin, tci):
                tt.append(t)
                c0.append(co0)
                i0.append(ci0)
    return dims, tt, c0, i0


def _f32_cuda(t, what):
    if not t.is_cuda or t.dtype != F32 or not t.is_contiguous():
        raise RuntimeError(f"pmoe_amd.optim: {what} must be a contiguous float32 tensor on the MI355X (cuda) device; "
                           f"got {t.dtype} on {t.device} (there is no CPU path)")
    return t.data_ptr()


class _Table:
    """Device copy of a pmoe_opt_tensor array + its chunk lists.  Tables are cached on the tuple of raw pointers they
    hold PLUS their element counts and the device (parameter / state storage is stable, and torch's caching allocator
    hands the gradient arena back at the same address step after step; the allocator also reuses addresses across
    models, so pointers alone would not identify a table), so the steady state uploads nothing; a new table goes up
    through pinned memory without blocking the host."""

    _cache = {}

    @classmethod
    def get(cls, key, device, build_rows, numels=()):
        key = (str(device), tuple(int(n) for n in numels)) + tuple(key)
        tab = cls._cache.get(key)
        if tab is None:
            if len(cls._cache) > 8:
                cls._cache.clear()
            tab = cls._cache[key] = cls(build_rows(), device)
        return tab

    def __init__(self, rows, device):
        packs = None
        if isinstance(rows, tuple):        # (pmoe_opt_tensor rows, pmoe_opt_pack rows): a tile table instead of chunk lists
            rows, packs = rows
        self.n = len(rows)
        self.host = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).pin_memory()     # kept alive with the table
        self.table = self.host.to(device, non_blocking=True)
        if packs is not None:
            dims, tt, c0, i0 = pack_tiles(list(zip(packs["cout"].tolist(), packs["cin"].tolist(), packs["taps"].tolist())))
            packs["tco"], packs["tci"] = [d[0] for d in dims], [d[1] for d in dims]
            self._packs_host = torch.from_numpy(packs.view(np.uint8).reshape(-1).copy()).pin_memory()
            self.packs = self._packs_host.to(device, non_blocking=True)
            self._tiles_host = torch.tensor([tt, c0, i0], dtype=torch.int32).pin_memory()
            self.tiles = self._tiles_host.to(device, non_blocking=True)
            self.n_tiles = len(tt)
            return
        ct, ci = [], []
        for t, n in enumerate(rows["numel"]):
            k = (int(n) + CHUNK - 1) // CHUNK
            ct.extend([t] * k)
            ci.extend(range(k))
        self._chunks_host = torch.tensor([ct, ci], dtype=torch.int32).pin_memory()
        chunks = self._chunks_host.to(device, non_blocking=True)
        self.chunk_tensor, self.chunk_index = chunks[0], chunks[1]
        self.n_chunks = len(ct)

    def args(self):
        return (C.c_void_p(self.table.data_ptr()), C.c_void_p(self.chunk_tensor.data_ptr()),
                C.c_void_p(self.chunk_index.data_ptr()), self.n_chunks)

    def pack_args(self):
        return (C.c_void_p(self.table.data_ptr()), C.c_void_p(self.packs.data_ptr())) + tuple(
            C.c_void_p(self.tiles[i].data_ptr()) for i in range(3)) + (self.n_tiles,)


def _rows(n):
    return np.zeros(n, dtype=_ROW)


def _grad_table(params):
    ps = [p for p in params if p.grad is not None]
    if not ps:
        return None, ps
    ptrs = tuple(_f32_cuda(p.grad, "gradient") for p in ps)

    def build():
        rows = _rows(len(ps))
        rows["grad"] = ptrs
        rows["numel"] = [p.numel() for p in ps]
        return rows
    return _Table.get(("g",) + ptrs, ps[0].device, build, [p.numel() for p in ps]), ps


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, scale=True):
    """``torch.nn.utils.clip_grad_norm_`` (L2 only): returns the total norm as a 0-d DEVICE tensor and scales the
    gradients in place by ``min(1, max_norm / (norm + 1e-6))``.  ``scale=False`` only measures (the reference's
    ``check_grad_norm``, utils/nn.py:10-19, without its per-tensor ``.item()`` syncs); the returned tensor carries
    ``.clip_state`` for ``FusedAdam.step(clip=...)``."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("pmoe_amd.optim.clip_grad_norm_: only the L2 norm (the reference's default) is fused")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    tab, ps = _grad_table(list(parameters))
    if tab is None:
        return torch.zeros((), dtype=F32, device="cuda")
    dev = ps[0].device
    partial = torch.empty(tab.n_chunks, dtype=F32, device=dev)
    norm = torch.empty(2, dtype=F32, device=dev)
    check(load().pmoe_mt_grad_norm(*tab.args(), float(max_norm), C.c_void_p(partial.data_ptr()), C.c_void_p(norm.data_ptr()),
                                   int(bool(scale)), stream_ptr()), "pmoe_mt_grad_norm")
    if scale:
        torch.autograd.graph.increment_version([p.grad for p in ps])
    total = norm[0]
    total.clip_state = norm
    return total


def _pack_engines(packs, who="FusedAdam"):
    """``packs`` -> the engine hosts (pmoe_amd.model.host.EngineHost) among the given modules and their submodules; an object
    that has ``pack_sinks`` itself (an engine) is taken as it is"""
    from .model.host import EngineHost
    out = []
    for m in packs if isinstance(packs, (list, tuple)) else [packs]:
        if hasattr(m, "pack_sinks"):
            out.append(m)
        elif isinstance(m, torch.nn.Module):
            hosts = [h for h in m.modules() if isinstance(h, EngineHost)]
            if not hosts:
                raise ValueError(f"{who}(packs=...): {type(m).__name__} hosts no engine")
            out.extend(hosts)
        else:
            raise TypeError(f"{who}(packs=...): a module that hosts an engine, or a list of them")
    return out


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share -- everything but the update rule: state creation, the step loop (one launch per
    parameter group, or two where an engine's packs take part), the table of a launch with its cache key, the ``packs=`` rule
    and the version / ``packs_written`` tail.  A subclass names its two entry points and says which table column holds which
    state tensor (``_slots``), which arguments the launch takes (``_hyper``) and what else a table row carries (``_fill``)."""

    _NAME = None           # in error texts
    _TAG = None            # of the table cache keys
    _ENTRY = None          # (entry point over a chunk table, entry point over a tile table)

    def __init__(self, params, defaults, packs):
        super().__init__(params, defaults)
        self._pack_hosts = _pack_engines(packs, self._NAME) if packs is not None else []

    def _slots(self, group):
        """-> ((table column, state key), ...): the state tensors of a parameter of ``group``, in torch's order of creation"""
        raise NotImplementedError

    def _fill(self, rows, group, steps):
        """per-tensor values of a freshly built table other than pointers and sizes"""

    def _key_steps(self, steps):
        """what of the step counts a cached table depends on"""
        return ()

    def _hyper(self, group, steps):
        """-> the arguments of the launch between the table and the clip state"""
        raise NotImplementedError

    def _open_packs(self):
        """-> (sink of every parameter whose update goes through the pack launch, key of the banks they point into, the engines
        to tell afterwards with the version sum each had)"""
        sinks, key, claims = {}, (), []
        mine = None
        for h in self._pack_hosts:
            eng = h if hasattr(h, "pack_sinks") else h.__dict__.get("_eng")
            found = eng.pack_sinks() if eng is not None else None
            if found is None:
                continue
            before = eng.param_version()
            if eng._packed_version != before:
                continue                       # the packs are behind already: the next forward packs everything anyway
            if mine is None:
                mine = {id(p) for g in self.param_groups for p in g["params"]}
            if not mine.issuperset(found.by_param):
                continue                       # parameters this optimizer never sees: leave the whole engine to its own pack
            if not sinks.keys().isdisjoint(found.by_param):
                continue                       # a tensor another engine packs too: one launch writes one set of banks
            sinks.update(found.by_param)
            key += (id(eng), found.gen)
            claims.append((eng, before))
        return sinks, key, claims

    @torch.no_grad()
    def step(self, closure=None, clip=None):
        """``clip``: the tensor returned by ``clip_grad_norm_(..., scale=False)`` -- its coefficient is applied to the
        gradients inside the update kernel (gradients stay unscaled in memory)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip_state = getattr(clip, "clip_state", None) if clip is not None else None
        if clip is not None and clip_state is None:
            raise ValueError(f"{self._NAME}.step(clip=...): pass the tensor returned by pmoe_amd.optim.clip_grad_norm_")
        sinks, bank_key, claims = self._open_packs() if self._pack_hosts else ({}, (), [])
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            slots = self._slots(group)
            for p in ps:
                if p.grad.is_sparse:
                    raise RuntimeError(f"{self._NAME} does not support sparse gradients")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0, dtype=F32)      # torch keeps `step` as a CPU f32 scalar tensor
                    for _, k in slots:
                        st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
            if sinks:
                packed = [p for p in ps if id(p) in sinks]
                self._launch(group, [p for p in ps if id(p) not in sinks], slots, clip_state)
                self._launch(group, packed, slots, clip_state, [sinks[id(p)] for p in packed], bank_key)
            else:
                self._launch(group, ps, slots, clip_state)
            # the kernel wrote through raw pointers: tell autograd (and the engine's packed-weight cache, which keys
            # on the version counters) that these tensors changed in place
            torch.autograd.graph.increment_version(ps)
        for eng, before in claims:
            eng.packs_written(before)
        return loss

    def _launch(self, group, ps, slots, clip_state, sinks=None, bank_key=()):
        """one launch over ``ps``: the chunk-table entry point, or with ``sinks`` (one per tensor) the tile-table one"""
        if not ps:
            return
        steps = [float(self.state[p]["step"]) for p in ps]
        cols = {"param": tuple(_f32_cuda(p, "parameter") for p in ps),
                "grad": tuple(_f32_cuda(p.grad, "gradient") for p in ps)}
        for col, k in slots:
            cols[col] = tuple(_f32_cuda(self.state[p][k], k) for p in ps)

        def build():
            rows = _rows(len(ps))
            for k, v in cols.items():
                rows[k] = v
            rows["numel"] = [p.numel() for p in ps]
            self._fill(rows, group, steps)
            if sinks is None:
                return rows
            packs = np.zeros(len(ps), dtype=_PACK_ROW)
            for i, k in enumerate(_PACK_FIELDS):
                packs[k] = [s[i] for s in sinks]
            if max(int(p.numel()) for p in ps) >= 2 ** 31:
                raise RuntimeError(f"{self._NAME}(packs=...): a packed parameter has 2^31 or more elements")
            return rows, packs
        # a pack table also holds pointers into the engine's banks: its key carries them, the layout they are written in and the
        # engines' build counters -- banks built again (another compute dtype or device) never meet a table of the old ones
        # and every key names the columns its pointers went into: two modes of one optimizer can fill equally many columns (RMSprop
        # with momentum only and centered only), and a table of the one must never serve the other
        key = ((self._TAG,) if sinks is None else (self._TAG + "p", bank_key, tuple(sinks))) + (tuple(cols),) + tuple(
            v for c in cols.values() for v in c) + self._key_steps(steps)
        tab = _Table.get(key, ps[0].device, build, [p.numel() for p in ps])
        tail = (C.c_void_p(clip_state.data_ptr()) if clip_state is not None else None, stream_ptr())
        plain, tiled = self._ENTRY
        if sinks is None:
            check(getattr(load(), plain)(*tab.args(), *self._hyper(group, steps), *tail), plain)
        else:
            check(getattr(load(), tiled)(*tab.pack_args(), *self._hyper(group, steps), *tail), tiled)


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` semantics (same arguments, same per-parameter ``state`` keys ``step`` / ``exp_avg`` /
    ``exp_avg_sq`` / ``max_exp_avg_sq``, so ``state_dict()`` checkpoints interchange with the reference's optimizer,
    train_2.py:300-310), updated by one multi-tensor HIP launch per parameter group.

    ``packs``: a module that runs on an engine (or a list of them).  The parameters that the engine keeps packed -- conv /
    linear weights and biases -- are then updated by a second launch per group that also stores the new values into the engine's
    packed operands, and the engine is told that its packs hold the new parameter versions: the next forward packs nothing.
    An engine takes part in a step only if its packs were current when the step began, the optimizer holds every parameter
    the engine packs, and the engine is not on its fp8 policy; otherwise its parameters take the ordinary launch and the
    engine packs as usual.  ``packs=None``: exactly the launches of before.  ``state_dict()`` does not change."""

    _NAME, _TAG, _ENTRY = "FusedAdam", "a", ("pmoe_mt_adam", "pmoe_mt_adam_packs")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, packs=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("FusedAdam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad), packs)

    def _slots(self, group):
        return (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq")) + (
            (("max_exp_avg_sq", "max_exp_avg_sq"),) if group["amsgrad"] else ())

    def _fill(self, rows, group, steps):
        b1, b2 = group["betas"]
        rows["bc1"] = [1.0 - b1 ** k for k in steps]
        rows["bc2_sqrt"] = [(1.0 - b2 ** k) ** 0.5 for k in steps]

    def _key_steps(self, steps):
        return () if min(steps) == max(steps) else tuple(steps)

    def _hyper(self, group, steps):
        # all tensors at the same step (the normal case): bias corrections travel as kernel arguments and the cached
        # table is reused; otherwise the per-tensor values of a freshly built table are used (argument < 0)
        b1, b2 = group["betas"]
        uniform = min(steps) == max(steps)
        bc1 = 1.0 - b1 ** steps[0] if uniform else -1.0
        bc2s = (1.0 - b2 ** steps[0]) ** 0.5 if uniform else -1.0
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                int(bool(group["amsgrad"])), float(bc1), float(bc2s))


class FusedRMSprop(_FusedOptimizer):
    """``torch.optim.RMSprop`` semantics -- the trainers' ``optimizer: rmsprop`` (train_2.py:62-73; ``conf/stage_*.yaml``
    ``rmsprop:`` = lr, momentum 0, alpha 0.99, eps 1e-8, centered, weight_decay 0): torch's arguments, defaults and
    ``ValueError``s, and torch's per-parameter ``state`` (``step``, ``square_avg``, ``momentum_buffer`` where momentum > 0,
    ``grad_avg`` where centered), so ``state_dict()`` checkpoints interchange with ``torch.optim.RMSprop``.  One multi-tensor
    HIP launch per parameter group (``csrc/optim.hip``: ``rmsprop_upd``; the formula is in ``include/pmoe_hip.h`` at
    ``pmoe_mt_rmsprop``).  Like torch there is no clamp under the square root: a centered ``square_avg - grad_avg^2`` that
    rounds below zero gives NaN in both.  ``step(clip=...)`` and ``packs=`` are FusedAdam's."""

    _NAME, _TAG, _ENTRY = "FusedRMSprop", "r", ("pmoe_mt_rmsprop", "pmoe_mt_rmsprop_packs")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, packs=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= alpha:
            raise ValueError(f"Invalid alpha value: {alpha}")
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered,
                                      weight_decay=weight_decay), packs)

    def _slots(self, group):
        # the rows of the table are pmoe_opt_tensor's: square_avg travels in exp_avg_sq, momentum_buffer in exp_avg and
        # grad_avg in max_exp_avg_sq; a slot the mode does not use stays NULL and the kernel never looks at it
        return ((("exp_avg_sq", "square_avg"),) + ((("exp_avg", "momentum_buffer"),) if group["momentum"] > 0 else ())
                + ((("max_exp_avg_sq", "grad_avg"),) if group["centered"] else ()))

    def _hyper(self, group, steps):
        # the kernel takes `momentum > 0` in float32 as "there is a momentum_buffer", _slots takes it from the double like torch: a
        # positive momentum below float32's normal range travels as the smallest normal one (buf * momentum rounds away either way)
        momentum = float(group["momentum"])
        if momentum > 0:
            momentum = max(momentum, float(np.finfo(np.float32).tiny))
        return (float(group["lr"]), float(group["alpha"]), float(group["eps"]), float(group["weight_decay"]),
                momentum, int(bool(group["centered"])))


def get_optimizer(name, params, cfg, packs=None):
    """The trainers' dispatch on ``train_params.optimizer`` (train_2.py:62-73, train_1.py:64, train_0.py:61) onto the fused
    optimizers: ``cfg.adam`` / ``cfg.rmsprop`` are the keyword blocks of the stage's configuration."""
    name = str(name)
    if name.lower() == "adam":
        return FusedAdam(params, **cfg.adam, packs=packs)
    if name.lower() == "rmsprop":
        return FusedRMSprop(params, **cfg.rmsprop, packs=packs)
    raise ValueError(f"Unknown optimizer {name}")


class FusedAveragedModel(torch.optim.swa_utils.AveragedModel):
    """``AveragedModel(model)`` (train_2.py:120,184) whose ``update_parameters`` is one multi-tensor launch."""

    @torch.no_grad()
    def update_parameters(self, model):
        mine, theirs = list(self.module.parameters()), list(model.parameters())
        if len(mine) != len(theirs):
            raise ValueError("FusedAveragedModel: parameter lists differ")
        for a, p in zip(mine, theirs):
            if a.shape != p.shape:
                raise ValueError("FusedAveragedModel: parameter shapes differ")
        pp = tuple(_f32_cuda(p.detach(), "parameter") for p in theirs)
        aa = tuple(_f32_cuda(a.detach(), "averaged parameter") for a in mine)

        def build():
            rows = _rows(len(mine))
            rows["param"], rows["swa"] = pp, aa
            rows["numel"] = [p.numel() for p in theirs]
            return rows
        tab = _Table.get(("s",) + pp + aa, mine[0].device, build, [p.numel() for p in theirs])
        # host-side mirror of n_averaged: no device->host sync per update when the buffer lives on the GPU
        n = self.__dict__.get("_n_host")
        if n is None or self.__dict__.get("_n_seen") != (id(self.n_averaged), self.n_averaged._version):
            n = int(self.n_averaged.item())      # first call, or the buffer was replaced / loaded from a checkpoint
        check(load().pmoe_mt_swa_update(*tab.args(), n, stream_ptr()), "pmoe_mt_swa_update")
        torch.autograd.graph.increment_version(mine)
        self.n_averaged += 1
        self.__dict__["_n_host"], self.__dict__["_n_seen"] = n + 1, (id(self.n_averaged), self.n_averaged._version)
