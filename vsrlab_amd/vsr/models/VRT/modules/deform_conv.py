"""VRT's deformable alignment modules, HIP-backed.  Mirrors vsrlab ``src/vsr/models/VRT/modules/deform_conv.py``:
``ModulatedDeformConv`` (:8-48), ``ModulatedDeformConvPack`` (:50-85), ``DCNv2PackFlowGuided`` (:87-145) -- same constructors,
parameter names and initialisation, so checkpoints load strictly.  The deformable convolution itself and the tanh / flow / sigmoid
epilogue in front of it run in ``vsr_deform_conv_fwd`` / ``_bwd`` (there is no torchvision here); the four ``conv_offset``
convolutions stay library convolutions, as the Linear layers of ``TMSA`` stay library GEMMs."""
import math

import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair, _single

from ..... import functional as VF


def _check_supported(module):
    if module.kernel_size != (3, 3) or _pair(module.stride) != (1, 1) or _pair(module.padding) != (1, 1) or \
            _pair(module.dilation) != (1, 1) or module.groups != 1:
        raise NotImplementedError("HIP deformable convolution: kernel 3x3, stride 1, padding 1, dilation 1, groups 1 (what the reference "
                                  f"instantiates); got kernel {module.kernel_size}, stride {module.stride}, padding {module.padding}, "
                                  f"dilation {module.dilation}, groups {module.groups}")
    if module.in_channels % module.deformable_groups:
        # the reference's vrt.yaml pairs embed_dims 120 / 180 with deformable_groups 16; torchvision rejects that as well
        raise ValueError(f"deformable_groups ({module.deformable_groups}) must divide in_channels ({module.in_channels})")


class ModulatedDeformConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.with_bias = bias
        self.transposed = False
        self.output_padding = _single(0)
        _check_supported(self)
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.init_weights()

    def init_weights(self):
        n = self.in_channels
        for k in self.kernel_size:
            n *= k
        stdv = 1. / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return VF.deform_conv2d(x, offset, self.weight, self.bias, self.stride, self.padding, self.dilation, mask)


class ModulatedDeformConvPack(ModulatedDeformConv):
    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=_pair(self.stride), padding=_pair(self.padding),
                                     dilation=_pair(self.dilation), bias=True)
        self.init_weights()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, "conv_offset"):
            self.conv_offset.weight.data.zero_()
            self.conv_offset.bias.data.zero_()

    def forward(self, x):
        o1, o2, mask = torch.chunk(self.conv_offset(x).float(), 3, dim=1)
        return VF.deform_conv2d(x, torch.cat((o1, o2), dim=1), self.weight, self.bias, self.stride, self.padding, self.dilation,
                                torch.sigmoid(mask))


class DCNv2PackFlowGuided(ModulatedDeformConvPack):
    """Flow-guided deformable alignment (BasicVSR++): offsets = max_residue_magnitude * tanh(conv_offset(...)) + flow."""

    def __init__(self, *args, **kwargs):
        self.max_residue_magnitude = kwargs.pop("max_residue_magnitude", 10)
        self.pa_frames = kwargs.pop("pa_frames", 2)
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Sequential(
            nn.Conv2d((1 + self.pa_frames // 2) * self.in_channels + self.pa_frames, self.out_channels, 3, 1, 1),
            nn.LeakyReLU(negative_slope=0.1, inplace=True),
            nn.Conv2d(self.out_channels, self.out_channels, 3, 1, 1),
            nn.LeakyReLU(negative_slope=0.1, inplace=True),
            nn.Conv2d(self.out_channels, self.out_channels, 3, 1, 1),
            nn.LeakyReLU(negative_slope=0.1, inplace=True),
            nn.Conv2d(self.out_channels, 3 * 9 * self.deformable_groups, 3, 1, 1),
        )
        self.init_offset()

    def init_offset(self):
        ModulatedDeformConv.init_weights(self)
        if hasattr(self, "conv_offset"):
            self.conv_offset[-1].weight.data.zero_()
            self.conv_offset[-1].bias.data.zero_()

    def forward(self, x, x_flow_warpeds, x_current, flows):
        out = self.conv_offset(torch.cat(x_flow_warpeds + [x_current] + flows, dim=1))
        return VF.flow_guided_deform_conv(x, out.float(), flows[0], self.weight, self.bias, self.max_residue_magnitude)
