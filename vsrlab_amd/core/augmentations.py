"""The reference's low-resolution augmentations (core/augmentations.py) on the GPU: ``RandomJPEGCompression`` and ``Mirroring``.

``RandomJPEGCompression`` sends a clip through ``functional.jpeg_compress`` (csrc/jpeg_degrade.hip) where the reference sends
every frame through ``to_pil_image`` -> libjpeg -> ``to_tensor`` on a loader CPU; the two agree bit for bit.

``RandomVideoCompression`` is NOT provided.  It encodes the clip with an H.264 codec through PyAV (``av``), which is not a
dependency of this project, and an inter-frame video codec has no counterpart among the kernels here.  A configuration that
names it has to keep using the reference's class; the reference's helpers around it (``read_video``, ``compress_video`` ...)
are file utilities of the same dependency and are left out with it.
"""
from random import randint

import torch
import torch.nn as nn

from .. import functional as VF


class RandomJPEGCompression(nn.Module):
    """JPEG-compress a (3, H, W) frame or a (N, 3, H, W) clip at a quality drawn once, at construction.

    ``quality``: ``[lo, hi]`` draws ``random.randint(lo, hi)``; ``[q]`` or a plain int is that value.  (The reference calls
    ``len()`` on a plain int and fails; that defect is not reproduced.)"""

    def __init__(self, quality):
        super().__init__()
        if isinstance(quality, (list, tuple)):
            if len(quality) not in (1, 2):
                raise ValueError(f"RandomJPEGCompression: quality must be an int, [q] or [lo, hi]; got {quality!r}")
            self.q = randint(quality[0], quality[1]) if len(quality) == 2 else quality[0]
        else:
            self.q = quality
        self.q = int(self.q)

    def forward(self, in_batch):
        if in_batch.dim() not in (3, 4):
            raise ValueError(f"RandomJPEGCompression: expected (3, H, W) or (N, 3, H, W); got {tuple(in_batch.shape)}")
        # the kernel clamps to [0, 1] itself and returns the dtype it was given
        return VF.jpeg_compress(in_batch.detach(), self.q).type_as(in_batch)


class Mirroring(nn.Module):
    """The clip followed by itself reversed in time: (T, ...) -> (2 T, ...)."""

    def __init__(self) -> None:
        super().__init__()

    @staticmethod
    def forward(x):
        return torch.cat((x, x.flip(0)), 0)
