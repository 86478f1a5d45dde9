"""``CharbonnierLoss`` (vsrlab ``src/core/losses.py:10-18``), fused value+gradient HIP kernel; ``AdversarialLoss``;
``PerceptualLoss`` (VGG19, ``src/core/losses.py:29-64``) on the HIP perceptual engine; ``OpticalFlowConsistency`` (RAFT-small,
``src/core/losses.py:79-98``) on the fused HIP correlation lookup."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as VF
from ..optical_flow.models.raft.raft import RAFT


class CharbonnierLoss(nn.Module):
    def __init__(self, eps=1e-9):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        return VF.charbonnier_loss(x, y, self.eps)


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
