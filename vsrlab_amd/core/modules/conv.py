"""Shared conv blocks of the hot path, HIP-backed.  Mirrors vsrlab ``src/core/modules/conv.py``:
``ConvReLU`` (:15-22), ``ResidualConv`` (:82-92), ``ResidualBlock`` (:94-103) -- same constructor
arguments, same parameter names (``conv.0.weight``, ``res_block.{i}.conv1.weight`` ...), so
checkpoints load strictly.  Inside ``BasicVSR`` / ``Spynet`` / ``UNetDiscriminator`` the whole network runs in one engine
call and these modules are its parameter containers; called on their own they dispatch to the per-layer kernels
(all differentiable: ``ResidualConv`` through its fused forward/backward function, ``ConvReLU`` and the ``ResidualBlock`` stem through
``vsr_conv_layer_fwd`` / ``vsr_conv_layer_bwd``).  ``DeformConv`` / ``DeformBlock`` (:33-80) run their deformable convolution
in ``vsr_deform_conv_fwd`` / ``_bwd``.  ``ConvST`` / ``ConvSTBlock`` (:105-143) run their ``nn.Conv3d`` layers in ``vsr_conv3d_fwd`` /
``_bwd`` (``core.conv3d_ops``), on the (b, t, c, h, w) tensor as it lies: no rearrange."""
import math

import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from ... import functional as VF
from ..conv3d_ops import conv3d


class _SpectralConv2d(nn.Module):
    """The parameters / buffers ``torch.nn.utils.spectral_norm(nn.Conv2d(..., bias=False))`` registers
    (``weight_orig``, ``weight_u``, ``weight_v``: same names, shapes and initialisation), so reference checkpoints
    load strictly.  The normalisation itself (one power iteration per training forward) runs in
    ``vsr_spectral_norm`` inside the discriminator's HIP call."""

    def __init__(self, in_ch, out_ch, ks, stride, pad):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding = in_ch, out_ch, ks, stride, pad
        conv = nn.Conv2d(in_ch, out_ch, ks, stride, pad, bias=False)          # for its default initialisation
        self.weight_orig = nn.Parameter(conv.weight.detach().clone())
        with torch.no_grad():
            u = nn.functional.normalize(torch.randn(out_ch), dim=0, eps=1e-12)
            v = nn.functional.normalize(torch.randn(in_ch * ks * ks), dim=0, eps=1e-12)
        self.register_buffer("weight_u", u)
        self.register_buffer("weight_v", v)


class SpectralConv(nn.Module):
    """spectral_norm(Conv2d(in_ch, out_ch, ks, stride, pad, bias=False))  (conv.py:6-13).  A building block of
    ``UNetDiscriminator``, which runs all of its layers in one engine call; called on its own it is an ordinary differentiable
    module for the shape the per-layer kernels serve (64 -> 64, 3x3, stride 1, padding 1 = the class defaults at 64 channels):
    ``vsr_spectral_norm`` (one power iteration per training-mode forward, ``weight_u`` / ``weight_v`` updated in place) +
    ``vsr_conv_layer_fwd`` / ``_bwd``."""

    def __init__(self, in_ch, out_ch, ks=3, stride=1, pad=1):
        super().__init__()
        self.conv = _SpectralConv2d(in_ch, out_ch, ks, stride, pad)

    def forward(self, x):
        c = self.conv
        if (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding) != (64, 64, 3, 1, 1):
            raise NotImplementedError("standalone HIP SpectralConv: Conv2d(64, 64, 3, 1, 1); the wide and the 4x4 stride-2 layers run "
                                      "inside the UNetDiscriminator engine (vsr_disc_forward)")
        return VF.spectral_conv_forward(x, c.weight_orig, c.weight_u, c.weight_v, self.training)


class ConvReLU(nn.Module):
    """Conv2d + ReLU (SPyNet building block, conv.py:15-22)."""

    def __init__(self, in_ch, out_ch, *args, **kwargs):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_ch, out_ch, *args, **kwargs), nn.ReLU())

    def forward(self, x):
        conv = self.conv[0]
        if conv.stride != (1, 1) or conv.padding != (conv.kernel_size[0] // 2,) * 2:
            raise NotImplementedError("HIP ConvReLU: stride 1, 'same' padding")
        return VF.conv_relu_forward(x, conv.weight, conv.bias)


class ResidualConv(nn.Module):
    """x + conv2(relu(conv1(x)))  (conv.py:82-92)."""

    def __init__(self, filters=64):
        super().__init__()
        self.conv1 = nn.Conv2d(filters, filters, 3, 1, 1)
        self.conv2 = nn.Conv2d(filters, filters, 3, 1, 1)
        self.relu = nn.ReLU()

    def forward(self, x):
        return VF.residual_conv(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias)


class ResidualBlock(nn.Module):
    """conv3x3 + LeakyReLU(0.1), then ``blocks`` x ResidualConv  (conv.py:94-103)."""

    def __init__(self, in_ch, out_ch=64, blocks=30):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_ch, out_ch, 3, 1, 1), nn.LeakyReLU(0.1))
        self.res_block = nn.Sequential(*[ResidualConv(out_ch) for _ in range(blocks)])

    def forward(self, x):
        blocks = [(b.conv1.weight, b.conv1.bias, b.conv2.weight, b.conv2.bias) for b in self.res_block]
        return VF.residual_block_forward(x, self.conv[0].weight, self.conv[0].bias, blocks)


class DeformConv(nn.Module):
    """Deformable convolution pack (conv.py:33-65).  The reference inherits ``torchvision.ops.DeformConv2d``; this class carries the
    same attributes, parameter names (``weight``, ``bias``, ``conv_offset.*``) and initialisation (kaiming-uniform(a=sqrt 5) weight,
    fan-in bias, zero offset convolution) without torchvision.  No modulation mask."""

    def __init__(self, deformable_groups, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
        self.groups = groups
        self.deformable_groups = deformable_groups
        if (self.kernel_size, self.stride, self.padding, self.dilation, groups) != ((3, 3), (1, 1), (1, 1), (1, 1), 1):
            raise NotImplementedError("HIP DeformConv: kernel 3x3, stride 1, padding 1, dilation 1, groups 1 (what DeformBlock instantiates); "
                                      f"got kernel {kernel_size}, stride {stride}, padding {padding}, dilation {dilation}, groups {groups}")
        if in_channels % deformable_groups:
            raise ValueError(f"deformable_groups ({deformable_groups}) must divide in_channels ({in_channels})")
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.weight.shape[1] * self.kernel_size[0] * self.kernel_size[1])
            nn.init.uniform_(self.bias, -bound, bound)
        self.conv_offset = nn.Conv2d(in_channels, deformable_groups * 2 * self.kernel_size[0] * self.kernel_size[1], self.kernel_size,
                                     self.stride, self.padding, self.dilation, self.groups)
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def forward(self, x):
        offset = self.conv_offset(x).float()
        return VF.deform_conv2d(x, offset, self.weight, self.bias, stride=self.stride, padding=self.padding, dilation=self.dilation)


class DeformBlock(nn.Module):
    """conv3x3, ``blocks`` x DeformConv(deformable_groups=1), conv3x3  (conv.py:67-80)."""

    def __init__(self, in_channels, mid_channels, blocks):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, mid_channels, 3, 1, 1)
        self.dcblock = nn.Sequential(*[DeformConv(deformable_groups=1, in_channels=mid_channels, out_channels=mid_channels, kernel_size=3,
                                                  padding=1) for _ in range(blocks)])
        self.conv_out = nn.Conv2d(mid_channels, in_channels, 3, 1, 1)

    def forward(self, x):
        return self.conv_out(self.dcblock(self.conv_in(x)))


class ConvST(nn.Module):
    """A (1,3,3) convolution, then a (3,1,1) one, on (b, t, c, h, w)  (conv.py:105-130).  Two launches; the reference's two
    ``rearrange`` calls are the strides of the descriptor.  The parameters are the reference's ``nn.Conv3d`` children (``conv_xy``,
    ``conv_t``, no biases), so initialisation and checkpoints are the reference's."""

    def __init__(self, in_ch, out_ch, kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=(1, 1, 1)):
        super().__init__()
        kernel_size, stride, padding = (tuple(int(v) for v in a) for a in (kernel_size, stride, padding))
        if kernel_size != (3, 3, 3) or stride != (1, 1, 1) or padding != (1, 1, 1):
            raise NotImplementedError("HIP ConvST: kernel (3,3,3), stride 1, padding k // 2 (the class defaults, what ConvSTBlock and "
                                      f"PixelShufflePack3D instantiate); got kernel {kernel_size}, stride {stride}, padding {padding}")
        self.conv_xy = nn.Conv3d(in_ch, out_ch, (1, 3, 3), 1, (0, 1, 1), bias=False)
        self.conv_t = nn.Conv3d(out_ch, out_ch, (3, 1, 1), 1, (1, 0, 0), bias=False)

    def forward(self, x, pixel_shuffle=0):
        x = conv3d(x, self.conv_xy.weight, time_major=True)
        return conv3d(x, self.conv_t.weight, pixel_shuffle=pixel_shuffle, time_major=True)


class ConvSTBlock(nn.Module):
    """Conv3d(3,3,3) with bias, then ``blocks`` x ConvST, on (b, t, c, h, w)  (conv.py:132-143)."""

    def __init__(self, blocks, in_ch, out_ch):
        super().__init__()
        self.conv_in = nn.Conv3d(in_ch, out_ch, 3, 1, 1)
        self.block = nn.Sequential(*[ConvST(out_ch, out_ch) for _ in range(blocks)])

    def forward(self, x):
        return self.block(conv3d(x, self.conv_in.weight, self.conv_in.bias, time_major=True))
