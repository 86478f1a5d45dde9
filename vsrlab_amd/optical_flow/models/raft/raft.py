"""``RAFT`` (reference ``raft/raft.py``), the small model: the only one whose trained weights exist (``raft-small.pth``)."""
import logging
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from .... import functional as VF
from .extractor import SmallEncoder
from .update import SmallUpdateBlock
from .utils import coords_grid, upflow

pylogger = logging.getLogger(__name__)

WEIGHTS_RELPATH = os.path.join("src", "optical_flow", "weights", "raft-small.pth")


def default_weights_path():
    """``$PROJECT_ROOT/src/optical_flow/weights/raft-small.pth``; without the variable the reference's own rule, the parent of
    the working directory.  (The reference spells the directory ``src/vsrlab.optical_flow``, which does not exist.)"""
    root = os.environ.get("PROJECT_ROOT") or os.path.dirname(os.getcwd())
    return os.path.join(root, WEIGHTS_RELPATH)


def load_raft_state_dict(weights=None):
    """``weights``: None (the default path), a path, or a state dict.  A ``module.`` prefix (DataParallel checkpoints) is
    stripped.  Never downloads: a missing file is ``FileNotFoundError`` naming the path that was expected."""
    if weights is None:
        weights = default_weights_path()
    if isinstance(weights, (str, os.PathLike)):
        if not os.path.isfile(weights):
            raise FileNotFoundError(f"RAFT-small weights not found at {weights} (nothing is downloaded): set $PROJECT_ROOT so that "
                                    f"$PROJECT_ROOT/{WEIGHTS_RELPATH} exists, or pass weights= a path or a state dict")
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    return OrderedDict((k[len("module."):] if k.startswith("module.") else k, v) for k, v in weights.items())


class RAFT(nn.Module):
    """``RAFT(small=True, scale_factor=2, pretrained=True)``.  ``weights``: path or state dict used instead of the default
    checkpoint (implies loading).  ``compute_dtype``: storage of the correlation pyramid ('fp32' / 'bf16'; None = the package
    rule, ``functional.resolve_dtype``).  ``small=False`` is not offered: its weights do not exist and it needs radius 4."""

    def __init__(self, small: bool = True, scale_factor: int = 2, pretrained: bool = True, weights=None, compute_dtype=None):
        super().__init__()
        if not small:
            raise NotImplementedError("RAFT(small=False): only RAFT-small is on the HIP path (radius 3, 128 feature channels)")
        self.scale_factor = scale_factor
        self.compute_dtype = compute_dtype
        self.hidden_dim, self.context_dim = 96, 64
        self.corr_levels, self.corr_radius = 4, 3
        self.fnet = SmallEncoder(output_dim=128, norm_fn='instance')
        self.cnet = SmallEncoder(output_dim=self.hidden_dim + self.context_dim, norm_fn='none')
        self.update_block = SmallUpdateBlock(self.corr_levels, self.corr_radius, hidden_dim=self.hidden_dim)
        if pretrained or weights is not None:
            pylogger.info('Loading RAFT pretrained weights')
            self.load_state_dict(load_raft_state_dict(weights), strict=True)

    @staticmethod
    def initialize_flow(img):
        n, _, h, w = img.shape
        coords = coords_grid(n, h // 8, w // 8).to(img.device).type_as(img)
        return coords, coords.clone()

    @staticmethod
    def check_size(img):
        h, w = img.shape[-2:]
        if h % 8 or w % 8 or h < 128 or w < 128:
            raise ValueError(f"RAFT: height and width must be multiples of 8 and at least 128 (the coarsest correlation level "
                             f"must be 2 x 2 or larger); got {h} x {w}")

    def forward(self, ref, supp, iters=12):
        """flow (N, 2, H, W) x ``scale_factor`` from ``supp`` to ``ref``, after ``iters`` updates at 1/8 resolution."""
        supp, ref = supp.contiguous(), ref.contiguous()
        self.check_size(supp)
        fmap1, fmap2 = self.fnet([supp, ref])
        net, inp = torch.split(self.cnet(supp), [self.hidden_dim, self.context_dim], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        coords0, coords1 = self.initialize_flow(supp)
        pyramid = VF.raft_corr_pyramid(fmap1, fmap2, self.corr_levels, self.compute_dtype, radius=self.corr_radius)
        for _ in range(iters):
            coords1 = coords1.detach()
            corr = VF.raft_corr_lookup(pyramid, coords1)
            net, _, delta_flow = self.update_block(net, inp, corr, coords1 - coords0)
            coords1 = coords1 + delta_flow
        return upflow(coords1 - coords0, scale_factor=self.scale_factor)
