"""``CharbonnierLoss`` (vsrlab ``src/core/losses.py:10-18``), fused value+gradient HIP kernel; ``AdversarialLoss``;
``PerceptualLoss`` (VGG19, ``src/core/losses.py:29-64``) on the HIP perceptual engine; ``OpticalFlowConsistency`` (RAFT-small,
``src/core/losses.py:79-98``) on the fused HIP correlation lookup; ``WL1Loss`` (``:20-27``) and ``rmse_loss`` (``:76-77``) on the fused pair
reductions of ``libvsrlab_losses.so``; ``LossPipeline`` (``:100-173``), which combines them by configuration."""
import os
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as VF
from . import pixel_ops
from .utils import resize
from ..optical_flow.models.raft.raft import RAFT


class CharbonnierLoss(nn.Module):
    def __init__(self, eps=1e-9):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        return VF.charbonnier_loss(x, y, self.eps)


class WL1Loss(nn.L1Loss):
    """``WL1Loss`` (``src/core/losses.py:20-27``): ``weight * mean |x - y|``, one fused value + gradient HIP pass, differentiable w.r.t.
    both arguments.  As in the reference, ``*args, **kwargs`` reach ``nn.L1Loss.__init__`` and ``forward`` ignores them:
    ``WL1Loss(2.0, reduction="sum")`` is twice the MEAN."""

    def __init__(self, weight=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.weight = weight

    def forward(self, x, y):
        return pixel_ops.l1_loss(x, y) * self.weight


def rmse_loss(yhat, y):
    """``rmse_loss`` (``src/core/losses.py:76-77``): ``sqrt(mean((yhat - y) ** 2))`` on the fused HIP pass.  No epsilon, as in the
    reference: equal operands give 0 and a NaN gradient."""
    return pixel_ops.rmse_loss(yhat, y)


class AdversarialLoss(nn.Module):
    """``AdversarialLoss`` (``src/core/losses.py:66-74``): BCE-with-logits against a constant target map; scaled by
    ``weight`` on the generator side only.  Fused value + gradient HIP kernel."""

    def __init__(self, weight=2e-5):
        super().__init__()
        self.weight = weight

    def forward(self, x, target, is_disc=False):
        loss = VF.bce_with_logits_const(x, target)
        return loss if is_disc else loss * self.weight


LAYER_WEIGHTS = dict(VF.PERCEPTUAL_LAYER_WEIGHTS)
VGG19_CHECKPOINT = "vgg19-dcbb9e9d.pth"          # torchvision's ImageNet weights, as models.vgg19(pretrained=True) caches them


def _vgg19_features(num_layers):
    """vgg19().features[:num_layers] (configuration 'E'): Conv2d 3x3 / ReLU(inplace=True) / MaxPool2d(2, 2), built locally."""
    layers, cin = [], 3
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"):
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)[:num_layers]


def _feature_state_dict(vgg_weights):
    """``vgg_weights`` (None, a path or a state dict; torchvision ``features.N.*`` or reference ``vgg.vgg_layers.N.*`` keys)
    -> {'N.weight': ..., 'N.bias': ...}.  Never downloads."""
    if vgg_weights is None:
        path = os.path.join(torch.hub.get_dir(), "checkpoints", VGG19_CHECKPOINT)
        if not os.path.isfile(path):
            raise FileNotFoundError(
                f"PerceptualLoss needs the VGG19 ImageNet weights and does not download them: {path} does not exist. Copy "
                f"torchvision's {VGG19_CHECKPOINT} there (torch.hub.get_dir() follows $TORCH_HOME), or pass vgg_weights= a path "
                "or a state dict (keys 'features.N.weight' or 'vgg.vgg_layers.N.weight').")
        vgg_weights = path
    if isinstance(vgg_weights, (str, os.PathLike)):
        vgg_weights = torch.load(vgg_weights, map_location="cpu", weights_only=True)
    out = {}
    for k, v in vgg_weights.items():
        for prefix in ("features.", "vgg.vgg_layers.", "vgg_layers."):
            if k.startswith(prefix):
                out[k[len(prefix):]] = v
                break
    return out


class PerceptualVGG(nn.Module):
    """``PerceptualVGG`` (``src/core/losses.py:29-45``): the frozen ``vgg19().features[:max+1]`` stack under ``vgg_layers``, so
    state_dict keys match the reference's.  Evaluated by the HIP engine inside ``PerceptualLoss``, not by ``forward``."""

    def __init__(self, layer_name_list, vgg_weights=None):
        super().__init__()
        self.layer_name_list = layer_name_list
        num_layers = max(map(int, self.layer_name_list)) + 1
        self.vgg_layers = _vgg19_features(num_layers)
        sd = _feature_state_dict(vgg_weights)
        self.vgg_layers.load_state_dict({k: sd[k] for k in self.vgg_layers.state_dict() if k in sd}, strict=True)
        for p in self.vgg_layers.parameters():
            p.requires_grad = False

    def params(self):
        return [t for m in self.vgg_layers if isinstance(m, nn.Conv2d) for t in (m.weight, m.bias)]


class PerceptualLoss(nn.Module):
    """``PerceptualLoss`` (``src/core/losses.py:47-64``): ``weight * sum_k LAYER_WEIGHTS[k] * l1(f_k(yhat), f_k(y))`` over VGG19
    taps 2, 7, 16, 25 (post-ReLU: the reference's taps are overwritten by ``ReLU(inplace=True)``) and 34 (pre-ReLU), on the HIP
    engine.  ``vgg_weights``: path or state dict; None = torchvision's cached checkpoint under ``torch.hub.get_dir()``
    (``FileNotFoundError`` if absent: nothing is downloaded).  ``max_workspace_bytes``: device workspace budget per call."""

    def __init__(self, weight=1, vgg_weights=None, max_workspace_bytes=None):
        super().__init__()
        self.weight = weight
        self.layer_weights = LAYER_WEIGHTS
        self.max_workspace_bytes = max_workspace_bytes
        self.vgg = PerceptualVGG(list(self.layer_weights.keys()), vgg_weights)

    def forward(self, yhat, y):
        return VF.perceptual_loss(yhat, y, self.vgg.params(), self.weight, max_workspace_bytes=self.max_workspace_bytes)


class OpticalFlowConsistency(nn.Module):
    """``OpticalFlowConsistency`` (``src/core/losses.py:79-98``): ``weight * l1(flow(sr), flow(hr))`` of frozen RAFT-small
    (``scale_factor=8``) between consecutive frames of (B, T, C, H, W) clips.  ``weights``: path or state dict; None = the
    checkpoint under ``$PROJECT_ROOT`` (``FileNotFoundError`` if absent: nothing is downloaded).  ``compute_dtype``: storage of
    the correlation pyramid.  The HR flow needs no gradient and is computed under ``no_grad`` (same values); the SR flow
    differentiates into ``sr``.  H and W: multiples of 8, at least 128."""

    def __init__(self, weight=1.0, weights=None, compute_dtype=None):
        super().__init__()
        self.of = RAFT(small=True, scale_factor=8, pretrained=True, weights=weights, compute_dtype=compute_dtype)
        self.weight = weight
        for p in self.of.parameters():
            p.requires_grad = False

    def forward(self, sr, hr):
        b, t, c, h, w = sr.shape
        flow_sr = self.of(sr[:, 1:].reshape(-1, c, h, w), sr[:, :-1].reshape(-1, c, h, w))
        with torch.no_grad():
            flow_hr = self.of(hr[:, 1:].reshape(-1, c, h, w), hr[:, :-1].reshape(-1, c, h, w))
        return F.l1_loss(flow_sr, flow_hr) * self.weight


class LossPipeline(nn.ModuleDict):
    """``LossPipeline`` (``src/core/losses.py:100-173``): named losses, evaluated as a list of terms on a dict of tensors.

    ``losses``: name -> ``nn.Module`` (registered in sorted-name order; anything else, or a name already present, is a
    ``ValueError``).  ``pipeline``: a list of ``{name: {'x': key, 'y': key}}`` terms.  ``forward(args)`` sets ``prefix + name +
    postfix`` to 0 for every loss and for ``'loss'``, then adds every term, in order, to its loss's key and to the total: a loss that
    the pipeline names twice accumulates into one key.  The dict that came in is the dict that is returned.

    A key that contains ``match`` is read without its ``match_`` prefix and resized (``core.utils.resize``: bilinear, on the HIP
    kernel, differentiable) to the (h, w) of the other operand; the ``x`` key is tested first and only one side is matched.

    Deviation: ``clone(prefix, postfix)`` raises ``NameError`` in the reference, which never imports ``deepcopy``.  Here
    it works: an independent deep copy under the new names."""

    def __init__(self, losses, pipeline, prefix=None, postfix=None):
        super().__init__()
        self.prefix = prefix
        self.postfix = postfix
        self.pipeline = pipeline
        self.losses = losses
        self.add_losses(losses)

    def add_losses(self, losses):
        for name in sorted(losses.keys()):
            loss = losses[name]
            if not isinstance(loss, nn.Module):
                raise ValueError(f"Value {loss} belonging to key {name} is not an instance of `nn.Module`")
            if name in self:
                raise ValueError(f"Encountered two losses both named {name}")
            self[name] = loss

    def _set_name(self, base):
        return ("" if self.prefix is None else self.prefix) + base + ("" if self.postfix is None else self.postfix)

    def set_keys(self, args):
        for name in list(self.losses.keys()) + ["loss"]:
            args[self._set_name(name)] = 0
        return args

    def clone(self, prefix=None, postfix=None):
        other = deepcopy(self)
        if prefix:
            other.prefix = prefix
        if postfix:
            other.postfix = postfix
        return other

    @staticmethod
    def match_shapes(matching, target):
        return resize(matching, tuple(target.shape[-2:])), target

    def get_loss(self, args, cfg):
        name, keys = list(cfg.items())[-1]                    # a term with several entries evaluates its last, as the reference's loop does
        x_key, y_key = keys["x"], keys["y"]
        if "match" in x_key:
            x, y = self.match_shapes(args[x_key.removeprefix("match_")], args[y_key])
        elif "match" in y_key:
            y, x = self.match_shapes(args[y_key.removeprefix("match_")], args[x_key])
        else:
            x, y = args[x_key], args[y_key]
        return self[name](x, y), name

    def forward(self, args: dict):
        args = self.set_keys(args)
        for cfg in self.pipeline:
            loss, name = self.get_loss(args, cfg)
            args[self._set_name(name)] += loss
            args[self._set_name("loss")] += loss
        return args
