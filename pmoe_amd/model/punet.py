"""Drop-in parameter container for ``PMoE/model/punet.py`` (``PredictiveUnet``).

Same constructor arguments and ``state_dict`` keys (``unet.*``, ``entry_block.*``, ``pred_unet.*``); like the
reference it loads the stage-0 U-Net checkpoint ``torch.load(model_path)[model_name]`` with ``strict=False`` and
freezes it (punet.py:40-55).  Inside ``PUNetExpert`` the arithmetic is issued by ``pmoe_amd.engine_punet.PUNetEngine``
(stage 2: the whole PU-Net frozen).  Called on its own -- ``PredictiveUnet.forward(img_list)``, the stage-1 trainer's
``self.model(img)`` (trainer/train_1.py:131-134) -- it runs on ``PredictiveUnetEngine``: forward, and backward through the
autoregressive loop for ``entry_block`` / ``pred_unet``, as one autograd node.
"""
import torch

from . import blocks as B
from .host import EngineFn, EngineHost


class PredictiveUnet(EngineHost, B._Held):
    def __init__(self, past_frames=4, future_frames=4, in_features=3, num_classes=23, gamma=2, b=1, inter_repr=False,
                 unet_inter_repr=False, model_name="unet-swa", model_path="unet.pth"):
        super().__init__()
        self.n_past_frames = past_frames
        self.n_future_frames = future_frames
        self.inter_repr = inter_repr
        self.unet_inter_repr = unet_inter_repr
        self.in_features, self.num_classes = in_features, num_classes
        self.unet = B.UNet(in_features=in_features, out_features=num_classes, gamma=gamma, b=b, inter_repr=unet_inter_repr)
        checkpoint = torch.load(model_path, map_location="cpu")       # punet.py:40 (raises like the reference if absent)
        self.unet.load_state_dict(checkpoint[model_name], strict=False)
        for p in self.unet.parameters():
            p.requires_grad = False
        self.unet.eval()
        self.entry_block = B.EfficientConvBlock(in_ch=past_frames * num_classes, out_ch=in_features, gamma=gamma, b=b)
        self.pred_unet = B.UNet(in_features=in_features, out_features=num_classes, gamma=gamma, b=b, inter_repr=inter_repr)

    def _make_engine(self):
        from ..engine_punet import PredictiveUnetEngine
        return PredictiveUnetEngine(self)

    def forward(self, img_list):
        """``punet.py:75-120``: img_list [B,T,C,H,W] -> logits of the ``future_frames`` predicted masks [B,F,classes,H,W]
        (f32), or the bottleneck feature [B,512] when ``inter_repr`` (inference only)."""
        assert img_list.shape[-4] == self.n_past_frames, "Number of images should match number of past frames"
        eng, dtype, taping = self.resolve_engine()
        return EngineFn.apply(eng, (img_list, self.training, taping, dtype), *eng.flat_params)[0]
