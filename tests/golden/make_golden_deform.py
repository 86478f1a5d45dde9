"""Generate tests/golden/deform_conv.npz from the REAL reference modules (build container only; uses make_golden.py's stub
mechanism to import the reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deform.py

torchvision is not installed, so ``torchvision.ops.deform_conv2d`` is stubbed with the pure-torch restatement of
tests/deform_common.py (it agrees with an independent grid_sample(align_corners=True, zeros) formulation to 1.5e-15 relative
in fp64).  That makes the restatement the ONLY available oracle of the operator itself; what the reference contributes is
everything around it: DCNv2PackFlowGuided's offset stack, chunk order, tanh / flow flip / sigmoid epilogue, parameter names and
shapes, and DeformBlock's composition.  fp64, keyed weights; only seeds, shapes and the reference's outputs are stored."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import deform_common as DC  # noqa: E402
from helpers import BIG, grad_stats, sub_stride  # noqa: E402
from make_golden import import_reference  # noqa: E402


def check_exercised(offset, mask, tanh_in, H, W, tag):
    """the data must exercise the operator: some, not most, samples out of bounds; tanh and sigmoid not saturated"""
    py, px = DC.sample_positions(offset, H, W)
    oob = float(((py <= -1) | (py >= H) | (px <= -1) | (px >= W)).double().mean())
    sat = float((torch.tanh(tanh_in).abs() > 0.99).double().mean())
    print(f"{tag}: out of bounds {oob:.3f}, |tanh| > 0.99 {sat:.3f}, mask {float(mask.min()):.3f}..{float(mask.max()):.3f}")
    assert 0.05 <= oob <= 0.40, oob
    assert sat < 0.10, sat
    assert float(mask.min()) >= 0.02 and float(mask.max()) <= 0.98


def put(store, tag, key, g):
    if g.numel() <= BIG:
        store[f"{tag}__{key}"] = g.detach().numpy().astype(np.float64)
    else:                                    # every stride-th element in full precision, the whole through its statistics
        store[f"{tag}__sub__{key}"] = g.detach().flatten()[::sub_stride(g.numel())].numpy().astype(np.float64)
    store[f"{tag}__stats__{key}"] = grad_stats(f"{tag}.{key}", g).numpy()


def main():
    torch.set_num_threads(8)
    import_reference()
    import torchvision.ops as ops
    captured = {}

    def stub(x, offset, weight, bias, stride, padding, dilation, mask=None):
        captured["offset"], captured["mask"] = offset.detach(), None if mask is None else mask.detach()
        return DC.deform_conv2d_ref(x, offset, weight, bias, mask=mask)

    class DeformConv2d(nn.Module):           # plain holder of what torchvision's module registers
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
            super().__init__()
            from torch.nn.modules.utils import _pair
            self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
            self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
            self.weight = nn.Parameter(torch.zeros(out_channels, in_channels // groups, *self.kernel_size))
            self.bias = nn.Parameter(torch.zeros(out_channels))

    ops.deform_conv2d = stub
    ops.DeformConv2d = DeformConv2d
    import importlib
    from vsrlab.core.modules import conv as ref_conv
    ref_conv = importlib.reload(ref_conv)    # re-import with the stubs in place
    from vsrlab.vsr.models.VRT.modules import deform_conv as ref_dc
    ref_dc.torchvision.ops.deform_conv2d = stub
    store = {}
    for tag, c in DC.DCN_CASES.items():
        m = ref_dc.DCNv2PackFlowGuided(c["C"], c["C"], 3, padding=1, deformable_groups=c["dg"], max_residue_magnitude=10, pa_frames=2)
        store[f"{tag}__keys"] = np.asarray(list(m.state_dict().keys()))
        store[f"{tag}__shapes"] = np.asarray([";".join(map(str, v.shape)) for v in m.state_dict().values()])
        m = m.double()
        m.load_state_dict(DC.dcn_state_dict(m.state_dict(), tag), strict=True)
        x, warped, cur, flow, cot = DC.dcn_inputs(tag)
        leaves = [t.requires_grad_(True) for t in (x, warped, cur, flow)]
        y = m(x, [warped], cur, [flow])
        with torch.no_grad():
            raw = m.conv_offset(torch.cat([warped, cur, flow], dim=1))
        check_exercised(captured["offset"], captured["mask"], raw[:, :18 * c["dg"]], c["H"], c["W"], tag)
        (y * cot).sum().backward()
        put(store, tag, "y", y)
        for name, t in zip(("dx", "dwarped", "dcur", "dflow"), leaves):
            put(store, tag, name, t.grad)
        named = dict(m.named_parameters())
        for k in ("weight", "bias", "conv_offset.0.weight", "conv_offset.6.weight"):
            put(store, tag, "grad__" + k.replace(".", "_"), named[k].grad)
        store[f"{tag}__case"] = np.asarray([c[k] for k in ("C", "dg", "N", "H", "W", "seed")])
    # ModulatedDeformConv / Pack key lists (no forward in the reference)
    for name, mod in (("mdc", ref_dc.ModulatedDeformConv(32, 32, 3, padding=1, deformable_groups=4)),
                      ("mdcp", ref_dc.ModulatedDeformConvPack(32, 32, 3, padding=1, deformable_groups=4))):
        store[f"{name}__keys"] = np.asarray(list(mod.state_dict().keys()))
        store[f"{name}__shapes"] = np.asarray([";".join(map(str, v.shape)) for v in mod.state_dict().values()])
    c = DC.BLOCK_CASE
    blk = ref_conv.DeformBlock(c["cin"], c["mid"], c["blocks"])
    store["blk__keys"] = np.asarray(list(blk.state_dict().keys()))
    store["blk__shapes"] = np.asarray([";".join(map(str, v.shape)) for v in blk.state_dict().values()])
    blk = blk.double()
    blk.load_state_dict(DC.block_state_dict(blk.state_dict()), strict=True)
    x, cot = DC.block_inputs()
    x.requires_grad_(True)
    y = blk(x)
    py, px = DC.sample_positions(captured["offset"], c["H"], c["W"])
    oob = float(((py <= -1) | (py >= c["H"]) | (px <= -1) | (px >= c["W"])).double().mean())
    print(f"blk: last DeformConv out of bounds {oob:.3f}, |offset| max {float(captured['offset'].abs().max()):.2f}")
    assert 0.05 <= oob <= 0.40, oob
    (y * cot).sum().backward()
    put(store, "blk", "y", y)
    put(store, "blk", "dx", x.grad)
    for k, p in blk.named_parameters():
        put(store, "blk", "grad__" + k.replace(".", "_"), p.grad)
    np.savez_compressed(os.path.join(HERE, "deform_conv.npz"), **store)
    print("deform_conv.npz", len(store), "arrays,", os.path.getsize(os.path.join(HERE, "deform_conv.npz")) // 1024, "KiB")


if __name__ == "__main__":
    main()
