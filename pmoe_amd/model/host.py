"""What every module that runs on an engine of its own shares (``_Grouped`` in moe.py, ``PredictiveUnet``, ``UNet``): the
engine cache, the deep copy that leaves it behind, the data-parallel switch, the compute-dtype rule, and the one autograd
node that wraps ``engine.forward`` / ``engine.backward``.  A host supplies ``_make_engine()`` and nothing else."""
import copy

import torch

_DEFAULT_DTYPE = torch.bfloat16


def set_default_compute_dtype(dtype):
    """bf16 (default; BASELINE config) or float32 (exact-f32 MFMA path, used for 1e-4 parity)."""
    global _DEFAULT_DTYPE
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("compute dtype must be torch.bfloat16 or torch.float32")
    _DEFAULT_DTYPE = dtype


class EngineFn(torch.autograd.Function):
    """A whole engine forward as one autograd node: ``args`` are the non-parameter arguments of ``engine.forward``; the
    differentiable inputs are the flat parameter list and, behind it, those input tensors (also held by ``args``) that want a
    gradient -- the ones the engine's state names in ``state["in_names"]``, in that order.  The engine's backward leaves their
    gradients in ``state["input_grads"]`` under those names; they are per rank, never reduced."""

    @staticmethod
    def forward(ctx, engine, args, *tensors):
        *outs, state = engine.forward(*args)
        ctx.engine, ctx.state = engine, state
        ctx.set_materialize_grads(False)      # an unused output (e.g. pred_speed under pmoe_loss) leaves its head's .grad None
        names = tuple(state.get("in_names", ())) if isinstance(state, dict) else ()
        n_par = len(tensors) - len(names)
        ctx.param_ids = [id(p) for p in tensors[:n_par]]
        ctx.inputs = [(name, t.shape, t.dtype) for name, t in zip(names, tensors[n_par:])]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        grads = ctx.engine.backward(ctx.state, *douts)
        found = ctx.state.get("input_grads", {}) if ctx.inputs else {}
        ctx.state = None
        out = [grads.get(i) if need else None for i, need in zip(ctx.param_ids, ctx.needs_input_grad[2:])]
        for (name, shape, dtype), need in zip(ctx.inputs, ctx.needs_input_grad[2 + len(ctx.param_ids):]):
            if need and name not in found:
                raise RuntimeError(f"pmoe_amd: the backward pass left no gradient for the input {name!r}")
            out.append(found[name].view(shape).to(dtype) if need else None)
        return (None, None) + tuple(out)


class EngineHost:
    """Mixin of an ``nn.Module`` whose ``forward`` is one engine call."""

    compute_dtype = None      # None -> the module-level default (bf16)
    fp8_weights = False       # True (with bf16 compute): BASELINE config 5 -- the ResNet layer1-4 forward convolutions run on
                              # e4m3 weights / e4m3 activations and the fp8 matrix cores (pmoe_conv_desc.w_fp8)

    def _engine(self):
        eng = self.__dict__.get("_eng")
        if eng is None:
            eng = self.__dict__["_eng"] = self._make_engine()      # not a submodule / not in state_dict / rebuilt after deepcopy
        return eng

    def __deepcopy__(self, memo):
        # AveragedModel(model) deep-copies (train_0.py:106, train_1.py:113, train_2.py:120): drop the engine (raw device
        # buffers), copy the rest
        eng = self.__dict__.pop("_eng", None)
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                new.__dict__[k] = copy.deepcopy(v, memo)
        finally:
            if eng is not None:
                self.__dict__["_eng"] = eng
        return new

    def enable_data_parallel(self, group=None, n_buckets=6, always=False):
        """Average parameter gradients over ``group`` (default WORLD) inside backward, bucketed and overlapped
        (pmoe_amd.parallel.BucketedAllReduce; the stage-1 roll-out accumulates shared-weight gradients until its first step has
        run, so there every bucket flies at the end of backward).  ``always``: issue the collectives even in a one-rank group
        (exercises the RCCL path on a single GPU)."""
        eng = self._engine()
        eng.dp_group, eng.dp_enabled, eng.dp_buckets, eng.dp_always = group, True, n_buckets, always
        return self

    def dtype_in_use(self):
        return self.compute_dtype or _DEFAULT_DTYPE

    def resolve_engine(self):
        """-> (engine, compute dtype, taping) of a call made now; the engine's fp8 switch follows ``fp8_weights`` here and nowhere
        else.  Grad mode is off inside Function.forward, so whether a backward tape is needed is decided here."""
        eng, dtype = self._engine(), self.dtype_in_use()
        eng.fp8 = bool(self.fp8_weights) and dtype == torch.bfloat16
        taping = torch.is_grad_enabled() and any(p.requires_grad for p in eng.flat_params)
        return eng, dtype, taping
