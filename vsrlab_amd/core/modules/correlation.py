"""``vsrlab.core.modules.correlation``: the local correlation of the reference's ``core/modules/correlation.py`` on one HIP
launch (``csrc/spatial_corr.hip``) instead of one pass over both maps per displacement."""
from typing import Tuple, Union

import torch
import torch.nn as nn

from ... import functional as VF

_IntOrPair = Union[int, Tuple[int, int]]


def iter_spatial_correlation_sample(input1: torch.Tensor, input2: torch.Tensor, kernel_size: _IntOrPair = 1, patch_size: _IntOrPair = 1,
                                    stride: _IntOrPair = 1, padding: _IntOrPair = 0, dilation: _IntOrPair = 1,
                                    dilation_patch: _IntOrPair = 1, compute_dtype=None) -> torch.Tensor:
    """(N, P_h, P_w, ceil(H' / s_h), ceil(W' / s_w)): the sum over channels of ``input1`` at every ``stride``-th position of the
    frame padded by ``padding`` times ``input2`` displaced by ``dilation_patch * (i, j) - max_displacement``.  The signature,
    the defaults and the three refusals are the reference's; what the kernel does not serve (patch above 9, stride or
    dilation_patch above 2, padding above the displacement) raises ``RuntimeError('... unsupported shape ...')``."""
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    if pair(kernel_size) != (1, 1):
        raise NotImplementedError("Only kernel_size=1 is supported.")
    if pair(dilation) != (1, 1):
        raise NotImplementedError("Only dilation=1 is supported.")
    if pair(patch_size)[0] % 2 == 0 or pair(patch_size)[1] % 2 == 0:
        raise NotImplementedError("Only odd patch sizes are supported.")
    return VF.spatial_correlation(input1, input2, patch_size, stride, padding, dilation_patch, compute_dtype=compute_dtype)


class SpatialCorrelationSampler(nn.Module):
    def __init__(self, kernel_size: _IntOrPair = 1, patch_size: _IntOrPair = 1, stride: _IntOrPair = 1, padding: _IntOrPair = 0,
                 dilation: _IntOrPair = 1, dilation_patch: _IntOrPair = 1) -> None:
        super().__init__()
        self.kernel_size, self.patch_size, self.stride = kernel_size, patch_size, stride
        self.padding, self.dilation, self.dilation_patch = padding, dilation, dilation_patch
        self.compute_dtype = None           # None: functional.resolve_dtype (bf16 under autocast, else fp32)

    def forward(self, input1: torch.Tensor, input2: torch.Tensor) -> torch.Tensor:
        return iter_spatial_correlation_sample(input1, input2, self.kernel_size, self.patch_size, self.stride, self.padding, self.dilation,
                                               self.dilation_patch, compute_dtype=self.compute_dtype)
