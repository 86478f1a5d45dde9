"""``EncoderDCT`` / ``DecoderIDCT`` (reference core/modules/dct_transforms.py) on the fused HIP block transform
(``core.token_ops.block_dct`` / ``block_idct``).

The reference runs an ``einops`` rearrange, a grouped stride-``ps`` convolution and a second rearrange; here one kernel reads the
planar frames and writes the token layout, and its adjoint goes back.  Constructors, ``generate_dct_matrix`` / ``build_filter``,
the ``.weight`` attribute and the ``state_dict`` keys (``dct_conv.weight``, ``reverse_dct.weight``: frozen parameters of shape
(3 ps^2, 1, ps, ps)) are the reference's, and the kernels read that parameter: a loaded checkpoint is honoured."""
import math

import numpy as np
import torch
import torch.nn as nn

from ..token_ops import block_dct, block_idct


class _FrozenWeight(nn.Module):
    """holds the transform's weight under the reference's key (``<name>.weight``), frozen as there"""

    def __init__(self, weight):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)


class _DCTBase(nn.Module):
    @staticmethod
    def build_filter(pos, freq, POS):
        """entry (freq, pos) of the orthonormal POS-point DCT-II matrix"""
        scale = math.sqrt((1.0 if freq == 0 else 2.0) / POS)
        return scale * math.cos(math.pi * freq * (2 * pos + 1) / (2 * POS))

    def generate_dct_matrix(self, ps=8):
        """(ps^2, ps, ps) in fp64: filter u ps + v is the outer product of rows u and v of the orthonormal DCT-II matrix"""
        rows = np.array([[self.build_filter(i, u, ps) for i in range(ps)] for u in range(ps)], dtype=np.float64)
        return np.einsum("ui,vj->uvij", rows, rows).reshape(ps * ps, ps, ps)

    def _basis(self, ps):
        self.ps = ps
        self.weight = torch.from_numpy(self.generate_dct_matrix(ps)).float().unsqueeze(1)
        return torch.cat([self.weight] * 3, dim=0)


class EncoderDCT(_DCTBase):
    """(b, t, 3, h, w) -> (b, t, (h // ps)(w // ps), 3 ps^2): the DCT coefficients of every ps x ps block of every colour plane"""

    def __init__(self, ps=4):
        super().__init__()
        self.dct_conv = _FrozenWeight(self._basis(ps))

    def forward(self, x):
        b, t, c, h, w = x.shape
        y = block_dct(x.reshape(b * t, c, h, w), self.dct_conv.weight, self.ps)
        return y.reshape(b, t, y.shape[1], y.shape[2])


class DecoderIDCT(_DCTBase):
    """(b, t, (h // ps)(w // ps), 3 ps^2) -> (b, t, 3, (h // ps) ps, (w // ps) ps)"""

    def __init__(self, out_ch, ps, h, w):
        super().__init__()
        if out_ch != 3:
            raise NotImplementedError(f"DecoderIDCT(out_ch={out_ch}): only out_ch = 3 is provided; the reference's out_ch in (1, 2) construct "
                                      "but mix coefficient channels across colour planes")
        self.reverse_dct = _FrozenWeight(self._basis(ps))
        self.h = h // ps
        self.w = w // ps

    def forward(self, x):
        b, t, p, c = x.shape
        if p != self.h * self.w:
            raise ValueError(f"DecoderIDCT built for {self.h} x {self.w} = {self.h * self.w} tokens got {p}")
        y = block_idct(x.reshape(b * t, p, c), self.reverse_dct.weight, self.ps, self.h * self.ps, self.w * self.ps)
        return y.reshape(b, t, *y.shape[1:])
