"""Drop-in for ``PMoE/model/moe.py``: ``get_model(cfg)``, ``MixtureOfExperts``, ``BaseExpert`` ...

Same constructor arguments (any attribute-style mapping, e.g. an OmegaConf node), same
``forward(images, speed, command)`` / ``sample(...)`` signatures and return types, same
``state_dict`` keys, so ``trainer/train_2.py`` and ``autoagents/image_agent.py``
can import it instead of the reference module.  All arithmetic runs in the grouped HIP engine.
"""
import torch
import torch.nn as nn
import torch.distributions as D

from .. import ops
from ..engine import ExpertGroupEngine
from ..utils import freeze  # noqa: F401  (re-exported: the reference imports it from utils.nn)
from . import blocks as B
from . import host as _host
from .host import EngineFn, EngineHost, set_default_compute_dtype  # noqa: F401  (re-exported: callers import it from here)
from .punet import PredictiveUnet


def __getattr__(name):
    # ``moe._DEFAULT_DTYPE`` reads the one default that host.set_default_compute_dtype writes (module-attribute semantics kept)
    if name == "_DEFAULT_DTYPE":
        return _host._DEFAULT_DTYPE
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def get_model(cfg):
    """``moe.py:25-47``."""
    model_type = cfg.type
    assert model_type is not None, "Network type can not be None"
    if model_type in ["moe", "moe_alt"]:
        return MixtureOfExperts(cfg)
    elif model_type == "moe_shared":
        return MixtureOfExpertsShared(cfg)
    elif model_type in ["punet", "punet_inter"]:
        return PUNetExpert(cfg)
    elif model_type in ["pmoe", "pmoe+pretrained"]:
        assert cfg.pmoe.moe_dir != "", "MoE pretrained weights directory should be specified"
        if model_type == "pmoe+pretrained":
            assert cfg.pmoe.punet_dir != "", "PU-Net pretrained weights directory should be specified"
        return PMoE(cfg)
    else:
        raise ValueError(
            f"{model_type} is UNKNOWN, model type should be one of 'moe', 'punet', "
            f"'punet_inter', 'pmoe', 'pmoe+pretrained', 'moe_alt'")


class _Grouped(EngineHost, nn.Module):
    """Shared forward plumbing of modules that own a list of experts."""

    def _shared_k(self):
        return 0

    def _make_engine(self):
        return ExpertGroupEngine(self._expert_list(), alt=self._alt(), shared_k=self._shared_k())

    input_grads = True        # images / speed / command that require grad get one (PUNetExpert: its frames pass a frozen PU-Net first)

    def _run(self, images, speed, command):
        eng, dtype, taping = self.resolve_engine()
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if self.training else 0
        args = (images, speed, command, self.training, taping, dtype, seed)
        # grad mode is off inside Function.forward: which inputs want a gradient is read here, and such a call is taped even
        # with every parameter frozen (saliency on an eval-mode, frozen policy)
        want = tuple(self.input_grads and torch.is_grad_enabled() and torch.is_tensor(t) and t.requires_grad
                     for t in (images, speed, command))
        if not any(want):         # the default path: the same node, the same launches
            # -> (probs, mean, std, speeds) for the mixtures; (actions, pred_speed) for PUNetExpert
            return EngineFn.apply(eng, args, *eng.flat_params)
        return EngineFn.apply(eng, args[:4] + (True,) + args[5:] + (want,), *eng.flat_params,
                              *[t for t, w in zip((images, speed, command), want) if w])


class BaseExpert(_Grouped):
    """``moe.py:50-101``: one expert.  Runs as a group of one when called on its own."""

    def __init__(self, params):
        super().__init__()
        self.speed_encoder = B.make_mlp(**params.speed_encoder)
        self.command_encoder = B.make_mlp(**params.command_encoder)
        if params.backbone.type != "rgb":
            raise NotImplementedError("backbone.type 'segmentation' (get_unet) is not built: the reference cannot run it either -- "
                                      "Sequential(entry_block, UNet(inter_repr=True)) returns a TUPLE (blocks/unet.py:92-95) that "
                                      "BaseExpert.forward's torch.cat rejects (model/moe.py:92-95); SURVEY.md section 2 #3")
        self.backbone = B.get_backbone(**{**params.backbone.rgb, "n_frames": params.backbone.n_frames})
        self.speed_pred = B.make_mlp(**params.speed_prediction)
        self.action_features = B.make_mlp(**params.action_head)
        width = params.action_head.dims[-1]
        self.alpha = B.Linear(width, 1)
        self.action_pred = B.Linear(width, 4)

    def _expert_list(self):
        return [self]

    def _alt(self):
        return False

    def _make_engine(self):
        eng = super()._make_engine()
        eng.raw_alpha = True        # a lone expert has no group to normalise over: the gate kernel hands back alpha itself
        return eng

    def forward(self, images, speed, command):
        """-> alpha [B,1], mean [B,2], std [B,2], pred_speed [B,1] (moe.py:74-101; BaseExpertAlt: moe.py:112-128).
        Runs as a group of ONE through the same engine the mixture uses (MixtureOfExperts builds its own grouped engine
        over all its experts and never calls this)."""
        alpha, mean, std, speeds = self._run(images, speed, command)
        return alpha, mean[:, 0], std[:, 0], speeds[:, 0]


class BaseExpertAlt(BaseExpert):
    """``moe.py:104-128``: alpha = MLP(1536 -> 512 -> 1) on the concatenated features, no ReLU."""

    def __init__(self, params):
        super().__init__(params)
        self.alpha = B._Seq(B.Linear(1536, 512), B.Activation("relu"), B.Linear(512, 1))

    def _alt(self):
        return True


class MixtureOfExperts(_Grouped):
    """``moe.py:131-177``."""

    def __init__(self, params):
        super().__init__()
        self.k = params.n_experts
        self._is_alt = params.type != "moe"
        base = BaseExpert if params.type == "moe" else BaseExpertAlt
        self.moe = nn.ModuleList([base(params) for _ in range(self.k)])

    def _expert_list(self):
        return list(self.moe)

    def _alt(self):
        return self._is_alt

    def mixture_params(self, images, speed, command):
        """probs [B,E], mean [B,E,2], std [B,E,2], speeds [B,E,1]: the deterministic tensors behind the
        distribution (gate softmax of moe.py:150-151 included)."""
        return self._run(images, speed, command)

    def forward(self, images, speed, command):
        probs, mean, std, speeds = self._run(images, speed, command)
        dist = MixtureDistribution(probs, mean, std)
        return dist, speeds

    def sample(self, images, speed, command):
        probs, mean, std, _ = self._run(images, speed, command)
        return MixtureDistribution(probs, mean, std).sample()


class MixtureOfExpertsShared(_Grouped):
    """``moe.py:180-265``: ONE trunk (encoders, backbone, speed / action-feature heads) whose last layer emits
    ``n_experts`` Gaussian components: ``action_pred = Linear(512, 4*n_experts)`` viewed as [B, n_experts, 4] and
    ``alpha = Linear(512, n_experts)`` (plain softmax).  ``forward`` returns (distribution, pred_speed [B,1])."""

    def __init__(self, params):
        super().__init__()
        self.speed_encoder = B.make_mlp(**params.speed_encoder)
        self.command_encoder = B.make_mlp(**params.command_encoder)
        if params.backbone.type != "rgb":
            raise NotImplementedError("backbone.type 'segmentation' (get_unet) is not built: the reference cannot run it either -- "
                                      "Sequential(entry_block, UNet(inter_repr=True)) returns a TUPLE (blocks/unet.py:92-95) that "
                                      "BaseExpert.forward's torch.cat rejects (model/moe.py:92-95); SURVEY.md section 2 #3")
        self.backbone = B.get_backbone(**{**params.backbone.rgb, "n_frames": params.backbone.n_frames})
        self.speed_pred = B.make_mlp(**params.speed_prediction)
        self.action_features = B.make_mlp(**params.action_head)
        width = params.action_head.dims[-1]
        self.n_experts = params.n_experts
        self.alpha = B.Linear(width, params.n_experts)
        self.action_pred = B.Linear(width, 4 * params.n_experts)

    def _expert_list(self):
        return [self]

    def _alt(self):
        return False

    def _shared_k(self):
        return self.n_experts

    def mixture_params(self, images, speed, command):
        """probs [B,K], mean [B,K,2], std [B,K,2], pred_speed [B,1]."""
        return self._run(images, speed, command)

    def forward(self, images, speed, command):
        probs, mean, std, speeds = self._run(images, speed, command)
        return MixtureDistribution(probs, mean, std), speeds

    def sample(self, images, speed, command):
        probs, mean, std, _ = self._run(images, speed, command)
        return MixtureDistribution(probs, mean, std).sample()


class PUNetExpert(_Grouped):
    """``moe.py:268-323``: frozen PU-Net (future segmentation masks) -> ResNet18-ECA backbone over the
    ``future_frames * num_classes`` mask channels -> ``tanh`` action head; ``punet_inter`` feeds the PU-Net bottleneck
    vector instead of a backbone.  Loads ``params.punet_path`` (key ``"model"``) exactly like the reference."""
    input_grads = False       # (limits: no gradient reaches the inputs of the PU-Net types)

    def __init__(self, params):
        super().__init__()
        self.return_inter = True if params.type == "punet_inter" else False
        params.punet.inter_repr = self.return_inter
        self.speed_encoder = B.make_mlp(**params.speed_encoder)
        self.command_encoder = B.make_mlp(**params.command_encoder)
        self.punet = PredictiveUnet(**params.punet)
        punet_weights = torch.load(params.punet_path, map_location=params.device)
        self.punet.load_state_dict(punet_weights["model"])
        self.punet = freeze(self.punet)
        self.backbone = None if self.return_inter else B.get_backbone(
            **{**params.backbone.rgb, "n_frames": params.punet.future_frames, "n_channels": params.punet.num_classes})
        self.speed_pred = B.make_mlp(**params.speed_prediction)
        self.action_pred = B._Seq(B.make_mlp(**params.action_head), B.Linear(params.action_head.dims[-1], 2))

    def _make_engine(self):
        from ..engine_punet import PUNetEngine
        return PUNetEngine(self)

    def forward(self, images, speed, command):
        """-> (actions [B,2] in (-1,1), pred_speed [B,1])."""
        return self._run(images, speed, command)

    def sample(self, images, speed, command):
        return self.forward(images, speed, command)[0]


class _BlendFn(torch.autograd.Function):
    """``tanh(cat(lat_weights([moe_x, punet_x]), long_weights([moe_y, punet_y])))`` (moe.py:353-356)."""

    @staticmethod
    def forward(ctx, moe_act, pu_act, lat_w, lat_b, long_w, long_b):
        Bsz = moe_act.shape[0]
        moe_act, pu_act = moe_act.contiguous().float(), pu_act.contiguous().float()
        out = torch.empty(Bsz, 2, dtype=torch.float32, device=moe_act.device)
        ops.blend_fwd(moe_act, pu_act, lat_w.contiguous(), lat_b.contiguous(), long_w.contiguous(), long_b.contiguous(),
                      out, Bsz)
        ctx.save_for_backward(moe_act, pu_act, lat_w, long_w, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        moe_act, pu_act, lat_w, long_w, out = ctx.saved_tensors
        Bsz = moe_act.shape[0]
        dlw, dgw = torch.empty_like(lat_w), torch.empty_like(long_w)
        dlb = torch.empty(1, dtype=torch.float32, device=out.device)
        dgb = torch.empty(1, dtype=torch.float32, device=out.device)
        dpu = torch.empty_like(pu_act) if ctx.needs_input_grad[1] else None
        ops.blend_bwd(moe_act, pu_act, lat_w.contiguous(), long_w.contiguous(), out, dout.contiguous().float(),
                      dlw, dlb, dgw, dgb, dpu, Bsz)
        return None, dpu, dlw, dlb, dgw, dgb


class PMoE(nn.Module):
    """``moe.py:326-363``: frozen mixture of experts + PU-Net expert, blended per axis by two ``Linear(2,1)``.
    ``forward`` returns ``(actions [B,2], -1)`` and is stochastic (``dists.sample()``), like the reference."""

    def __init__(self, params):
        super().__init__()
        assert params.pmoe.moe_dir is not None, "MoE weights should be provided"
        self.moe = MixtureOfExperts(params)
        # SWA checkpoints carry extra keys, therefore strict=False (moe.py:336-337)
        self.moe.load_state_dict(torch.load(params.pmoe.moe_dir, map_location="cpu"), strict=False)
        self.moe = freeze(self.moe, params.exclude_freeze, params.verbose)
        self.moe.input_grads = False      # (its actions are sampled: no gradient passes them, so nothing is taped for one)
        self.punet = PUNetExpert(params)
        if params.pmoe.punet_dir:
            self.punet.load_state_dict(torch.load(params.pmoe.punet_dir, map_location="cpu"), strict=False)
            self.punet = freeze(self.punet, params.exclude_freeze, params.verbose)
        self.lat_weights = B.Linear(2, 1)
        self.long_weights = B.Linear(2, 1)

    @property
    def compute_dtype(self):
        return self.moe.compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, dtype):
        self.moe.compute_dtype = dtype
        self.punet.compute_dtype = dtype

    def blend(self, moe_actions, punet_actions):
        """the deterministic tail of ``forward`` (moe.py:353-356) on given per-model actions."""
        return _BlendFn.apply(moe_actions, punet_actions, self.lat_weights.weight, self.lat_weights.bias,
                              self.long_weights.weight, self.long_weights.bias)

    def forward(self, images, speed, command):
        punet_actions, _ = self.punet(images, speed, command)
        dists, _ = self.moe(images, speed, command)
        moe_actions = dists.sample()
        # -1 is the reference's dummy speed prediction (interface consistency)
        return self.blend(moe_actions, punet_actions), -1

    def sample(self, images, speed, command):
        return self.forward(images, speed, command)[0]


class MixtureDistribution(D.MixtureSameFamily):
    """The very distribution ``moe.py:154-156`` builds; also keeps the raw parameter tensors so that
    ``pmoe_amd.loss.moe_loss`` can use the fused HIP loss kernel."""

    def __init__(self, probs, mean, std):
        self.hip_params = (probs, mean, std)
        super().__init__(D.Categorical(probs), D.Independent(D.Normal(mean, std), 1), validate_args=False)
