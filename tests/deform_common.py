"""Pure-torch restatement of deformable convolution (torchvision.ops.deform_conv2d semantics; 3x3, stride 1, padding 1,
dilation 1, groups 1) and of the flow-guided epilogue of VRT's DCNv2PackFlowGuided, in whatever dtype its inputs have (fp64 for
the oracles).  Explicit floor / four-corner gather with validity masks: no grid_sample, so no coordinate normalisation rounding.
torchvision is not installed anywhere this project is built or tested; this restatement is the only oracle of the operator.

``store``: where the bf16 build rounds -- x, the gathered columns, the weights, and the cotangent that enters the two
backward products -- the restatement rounds too (``bf16_store``); None = exact."""
import torch

from helpers import BIG, bf16_store, grad_stats, sub_stride  # noqa: F401  (the host tests read them here)


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_store(g)


def sample_positions(offset, H, W):
    """(py, px), each (N, dg, 9, H, W): py = y - 1 + i + dy, px = x - 1 + j + dx for tap k = 3 i + j."""
    N = offset.shape[0]
    dg = offset.shape[1] // 18
    off = offset.reshape(N, dg, 9, 2, H, W)
    k = torch.arange(9, device=offset.device)
    ys = torch.arange(H, device=offset.device, dtype=offset.dtype).view(1, 1, 1, H, 1)
    xs = torch.arange(W, device=offset.device, dtype=offset.dtype).view(1, 1, 1, 1, W)
    ki = (k // 3).to(offset.dtype).view(1, 1, 9, 1, 1)
    kj = (k % 3).to(offset.dtype).view(1, 1, 9, 1, 1)
    return ys - 1 + ki + off[:, :, :, 0], xs - 1 + kj + off[:, :, :, 1]


def deform_columns(x, offset, mask=None):
    """(N, Cin, 9, H*W): bilinear samples (a corner counts only inside the image) times the mask."""
    N, C, H, W = x.shape
    dg = offset.shape[1] // 18
    cpg = C // dg
    py, px = sample_positions(offset, H, W)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    xg = x.reshape(N, dg, cpg, H * W)

    def corner(yy, xx, wgt):
        valid = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().reshape(N, dg, 1, 9 * H * W).expand(-1, -1, cpg, -1)
        v = xg.gather(3, idx).reshape(N, dg, cpg, 9, H, W)
        return v * (wgt * valid.to(wgt.dtype)).unsqueeze(2)

    col = corner(y0, x0, (1 - ly) * (1 - lx)) + corner(y0, x0 + 1, (1 - ly) * lx) + \
        corner(y0 + 1, x0, ly * (1 - lx)) + corner(y0 + 1, x0 + 1, ly * lx)
    if mask is not None:
        col = col * mask.reshape(N, dg, 1, 9, H, W)
    return col.reshape(N, C, 9, H * W)


def deform_conv2d_ref(x, offset, weight, bias=None, stride=1, padding=1, dilation=1, mask=None, store=None):
    assert (stride, padding, dilation) in ((1, 1, 1), ((1, 1), (1, 1), (1, 1))) and tuple(weight.shape[2:]) == (3, 3)
    N, C, H, W = x.shape
    if store is not None:
        x, weight = store(x), store(weight)
    col = deform_columns(x, offset, mask)
    if store is not None:
        col = store(col)
    y = torch.einsum("ock,nckp->nop", weight.reshape(weight.shape[0], C, 9), col)
    if store is not None:
        y = _RoundGrad.apply(y)
    y = y.reshape(N, -1, H, W)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def flow_guided_offset_mask_ref(out, flow, max_residue_magnitude):
    """deform_conv.py:135-142: offset = mrm * tanh(cat(o1, o2)) + flow.flip(1) repeated, mask = sigmoid(third chunk)."""
    o1, o2, mask = torch.chunk(out, 3, dim=1)
    offset = max_residue_magnitude * torch.tanh(torch.cat((o1, o2), dim=1))
    offset = offset + flow.flip(1).repeat(1, offset.size(1) // 2, 1, 1)
    return offset, torch.sigmoid(mask)


def flow_guided_deform_conv_ref(x, out, flow, weight, bias, max_residue_magnitude, store=None):
    offset, mask = flow_guided_offset_mask_ref(out, flow, max_residue_magnitude)
    return deform_conv2d_ref(x, offset, weight, bias, mask=mask, store=store)


def near_integer(offset, H, W, tol=1e-4):
    """(N, dg, 9, H, W) bool: sample positions within tol px of an integer in y or x, where d offset has its kink."""
    py, px = sample_positions(offset, H, W)
    return ((py - torch.round(py)).abs() < tol) | ((px - torch.round(px)).abs() < tol)


def keyed(key, shape, scale=1.0, dtype=torch.float64):
    from oracle.basicvsr_oracle import keyed_tensor
    return (keyed_tensor(key, tuple(shape)) * scale).to(dtype)


# the golden cases of tests/golden/make_golden_deform.py: inputs are functions of these numbers alone
DCN_CASES = {"a": dict(C=32, dg=4, N=2, H=20, W=28, wscale=1.5, flow=4.0, seed=101),
             "b": dict(C=120, dg=8, N=1, H=32, W=40, wscale=1.5, flow=6.0, seed=111)}
BLOCK_CASE = dict(cin=3, mid=64, blocks=2, N=1, H=18, W=22, wscale=1.0, oscale=10.0, seed=121)


def dcn_inputs(case, dtype=torch.float64):
    c = DCN_CASES[case]
    g = torch.Generator().manual_seed(c["seed"])
    shp = (c["N"], c["C"], c["H"], c["W"])
    x, warped, cur, cot = (torch.randn(shp, generator=g, dtype=torch.float64) for _ in range(4))
    flow = (torch.rand((c["N"], 2, c["H"], c["W"]), generator=g, dtype=torch.float64) * 2 - 1) * c["flow"]
    return [t.to(dtype) for t in (x, warped, cur, flow, cot)]


def dcn_state_dict(module_sd, case, dtype=torch.float64):
    """keyed weights x wscale (biases as keyed), a function of the state_dict key"""
    s = DCN_CASES[case]["wscale"]
    return {k: keyed("dcn." + k, v.shape, 1.0 if k.endswith("bias") else s, dtype) for k, v in module_sd.items()}


def block_inputs(dtype=torch.float64):
    c = BLOCK_CASE
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randn((c["N"], c["cin"], c["H"], c["W"]), generator=g, dtype=torch.float64)
    cot = torch.randn((c["N"], c["cin"], c["H"], c["W"]), generator=g, dtype=torch.float64)
    return x.to(dtype), cot.to(dtype)


def block_state_dict(module_sd, dtype=torch.float64):
    c = BLOCK_CASE
    out = {}
    for k, v in module_sd.items():
        s = 1.0 if k.endswith("bias") else (c["oscale"] if "conv_offset" in k else c["wscale"])
        out[k] = keyed("dblock." + k, v.shape, s, dtype)
    return out
