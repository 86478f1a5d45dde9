"""The front of ``VRT.forward`` (vsrlab ``src/vsr/models/VRT/vrt.py:145-150``) on the HIP path, as module-level functions that mirror
the reference's methods, for the ``VRT`` class to bind when it lands: ``get_flows`` (:189-208), ``get_aligned_image`` (:211-228) and
``aligned_input``, the ``cat([x, x_backward, x_forward], 2)`` of :150 in one launch (csrc/warp_taps.hip).
``Upsample`` (:13-39), the reconstruction tail's conv + PixelShuffle(2) + LeakyReLU(0.1) groups, runs one ``vsr_conv3d_fwd`` launch per
group (csrc/conv3d.hip).  ``Stage``, ``VRT`` and ``TinyVRT`` themselves are not provided (README)."""
import math

import torch.nn as nn

from .... import functional as VF
from ....core.conv3d_ops import conv3d
from .modules.spynet import flow_warp  # noqa: F401  (the reference imports it here, :9)

aligned_input = VF.aligned_input


def get_flows(optical_flow, x):
    """Flow between frames t and t+1 of ``x`` (B, D, C, H, W) at every level ``optical_flow`` returns (``VRT.get_flows`` with the
    network passed in place of ``self``): two lists of (B, D - 1, 2, H / 2^i, W / 2^i) views, backward then forward."""
    b, n, c, h, w = x.size()
    x_1 = x[:, :-1, :, :, :].reshape(-1, c, h, w)
    x_2 = x[:, 1:, :, :, :].reshape(-1, c, h, w)
    n_scales = len(optical_flow.return_levels)

    def views(flows):
        flows = flows if isinstance(flows, (list, tuple)) else [flows]      # SpyNet returns the tensor itself for one level
        return [flow.view(b, n - 1, 2, h // (2 ** i), w // (2 ** i)) for flow, i in zip(flows, range(n_scales))]

    flows_backward = views(optical_flow(x_1, x_2))
    flows_forward = views(optical_flow(x_2, x_1))
    return flows_backward, flows_forward


def get_aligned_image(x, flows_backward, flows_forward):
    """``VRT.get_aligned_image`` (static, :211-228): ``[x_backward, x_forward]``, each (B, D, 4 C, H, W): the 'nearest4' warps of the
    neighbouring frames and a zero block at the clip's end.  Both are channel slices of ``aligned_input``'s result: one launch, and
    nothing is copied."""
    c = x.size(2)
    out = aligned_input(x, flows_backward, flows_forward)
    return [out[:, :, c:5 * c], out[:, :, 5 * c:]]


class _Transpose_Dim12(nn.Module):
    """Transpose dim 1 and dim 2 of a tensor (a child of ``Upsample``, as in the reference)."""

    @staticmethod
    def forward(x):
        return x.transpose(1, 2)


class Upsample(nn.Sequential):
    """``Upsample(scale, num_feat)`` on (b, c, t, h, w)  (vrt.py:13-39): log2(scale) groups of Conv3d(1,3,3) C -> 4C, PixelShuffle(2) on
    the frames and LeakyReLU(0.1), then a Conv3d(1,3,3) C -> C.  The children are the reference's at the reference's indices (keys
    ``0.*``, ``5.*``, ``10.*`` for scale 4); ``forward`` runs each group as ONE launch -- the shuffle is the store pattern and the
    LeakyReLU, which commutes with it, the epilogue -- plus the last convolution."""

    def __init__(self, scale, num_feat):
        assert (scale & (scale - 1)) == 0, "Scale should be a power of 2"
        m = []
        for _ in range(int(math.log(scale, 2))):
            m.append(nn.Conv3d(num_feat, 4 * num_feat, kernel_size=(1, 3, 3), padding=(0, 1, 1)))
            m.append(_Transpose_Dim12())
            m.append(nn.PixelShuffle(2))
            m.append(_Transpose_Dim12())
            m.append(nn.LeakyReLU(negative_slope=0.1, inplace=True))
        m.append(nn.Conv3d(num_feat, num_feat, kernel_size=(1, 3, 3), padding=(0, 1, 1)))
        super().__init__(*m)

    def forward(self, x):
        convs = [c for c in self if isinstance(c, nn.Conv3d)]
        for c in convs[:-1]:
            x = conv3d(x, c.weight, c.bias, act="leaky_relu", slope=0.1, pixel_shuffle=2)
        return conv3d(x, convs[-1].weight, convs[-1].bias)
