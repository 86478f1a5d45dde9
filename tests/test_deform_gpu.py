"""GPU tests of the HIP deformable convolution (csrc/deform_conv.hip) against the golden (tests/golden/deform_conv.npz, the
reference modules run in fp64 on the restatement) and the fp64 restatement of tests/deform_common.py.

Bounds: fp32 1e-3 relative (y: max-rel, gradients: rel-L2).  d offset / d out / d flow have a kink where a sample position is an
integer; positions within 1e-4 px of one (decided in the fp64 oracle) are left out, at most 0.1 % of them.  bf16: the
project's noise-floor criterion, error <= 1.5 x max(error of the bf16-storage restatement, 1e-3).
Projections <g, r> of gradients pinned by statistics: r is a unit normal vector independent of the error, so the difference is
N(0, |dg|^2); the bound is 3 sigma = 3 x tol x |g|."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_common as DC
from helpers import GOLDEN, bf16_store, proj_vector, rel_err, rel_l2, sub_stride

pytestmark = pytest.mark.gpu
TOL32 = 1e-3
FLOOR16 = 1e-3


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _inputs(seed, N, C, Cout, H, W, dg, mode):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    d = dict(x=r(N, C, H, W), weight=r(Cout, C, 3, 3) / (C * 9) ** 0.5, bias=r(Cout) * 0.1, cot=r(N, Cout, H, W))
    if mode == "flow":
        d["out"] = r(N, 27 * dg, H, W) * 0.6
        d["flow"] = (torch.rand(N, 2, H, W, generator=g, dtype=torch.float64) * 2 - 1) * 4
    else:
        d["offset"] = r(N, 18 * dg, H, W) * 3
        if mode == "mask":
            d["mask"] = torch.rand(N, 9 * dg, H, W, generator=g, dtype=torch.float64)
    return d


_DIFF = {"plain": ("x", "offset", "weight", "bias"), "mask": ("x", "offset", "mask", "weight", "bias"),
         "flow": ("x", "out", "flow", "weight", "bias")}


def _call(fn_plain, fn_flow, d, mode, **kw):
    if mode == "flow":
        return fn_flow(d["x"], d["out"], d["flow"], d["weight"], d["bias"], 10.0, **kw)
    return fn_plain(d["x"], d["offset"], d["weight"], d["bias"], mask=d.get("mask"), **kw)


def _run(d, mode, fn_plain, fn_flow, dev, dtype, **kw):
    t = {k: v.detach().clone().to(device=dev, dtype=dtype) for k, v in d.items()}      # fresh leaves on every call
    for k in _DIFF[mode]:
        t[k].requires_grad_(True)
    y = _call(fn_plain, fn_flow, t, mode, **kw)
    (y * t["cot"]).sum().backward()
    return y.detach(), {k: t[k].grad.detach() for k in _DIFF[mode]}


def _hip(d, mode, dev, compute_dtype):
    from vsrlab_amd import functional as VF
    out = _run(d, mode, VF.deform_conv2d, VF.flow_guided_deform_conv, dev, torch.float32, compute_dtype=compute_dtype)
    torch.cuda.synchronize()
    return out


def _oracle(d, mode, store=None):
    return _run(d, mode, DC.deform_conv2d_ref, DC.flow_guided_deform_conv_ref, "cpu", torch.float64, store=store)


def _kink_keep(d, mode, H, W):
    """per (n, group, tap, pixel): True where the sample position is not within 1e-4 px of an integer"""
    off = DC.flow_guided_offset_mask_ref(d["out"], d["flow"], 10.0)[0] if mode == "flow" else d["offset"]
    near = DC.near_integer(off, H, W)
    assert float(near.double().mean()) <= 1e-3, float(near.double().mean())
    return ~near


def _errors(y, g, y_o, g_o, d, mode, H, W):
    keep = _kink_keep(d, mode, H, W)                   # (N, dg, 9, H, W)
    N, dg = keep.shape[:2]
    e = {"y": rel_err(y, y_o)}
    for k in g:
        a, b = g[k].double().cpu(), g_o[k]
        if k == "offset" or k == "out":
            m = keep.unsqueeze(3).expand(-1, -1, -1, 2, -1, -1).reshape(N, 18 * dg, H, W).to(a.dtype)
            if k == "out":                             # mask logits have no kink
                m = torch.cat([m, torch.ones(N, 9 * dg, H, W, dtype=a.dtype)], dim=1)
            a, b = a * m, b * m
        elif k == "flow":                              # a pixel's d flow sums every tap: leave out pixels with any kinked tap
            m = keep.all(dim=1).all(dim=1).unsqueeze(1).to(a.dtype)
            a, b = a * m, b * m
        e[k] = rel_l2(a, b)
    return e


SHAPES = [dict(N=2, C=32, Cout=32, H=13, W=37, dg=4), dict(N=1, C=120, Cout=120, H=11, W=21, dg=12),
          dict(N=1, C=64, Cout=64, H=9, W=19, dg=1), dict(N=2, C=9, Cout=8, H=13, W=37, dg=3)]


@pytest.mark.parametrize("mode", ["plain", "mask", "flow"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s['C']}dg{s['dg']}")
def test_fp32_matches_the_fp64_restatement(mode, shape):
    """odd shapes: W not a multiple of 32, H*W not a multiple of the 32- and 64-pixel tiles; cpg 8, 10 (padded to 16) and 64;
    C9dg3: groups of 3 in slots of 8, 24 packed channels in a staged row of 32, 8 outputs in an accumulator block of 32"""
    dev = _gpu()
    d = _inputs(7, mode=mode, **shape)
    y, g = _hip(d, mode, dev, "fp32")
    y_o, g_o = _oracle(d, mode)
    e = _errors(y, g, y_o, g_o, d, mode, shape["H"], shape["W"])
    print("fp32", mode, shape, e)
    assert all(v < TOL32 for v in e.values()), e


@pytest.mark.parametrize("mode", ["plain", "mask", "flow"])
def test_bf16_within_the_noise_floor(mode):
    """Measured on an MI355X (C 120, dg 8, 11x21): y 2.6e-3..3.1e-3 (restatement: the same to 4 digits), gradients 2.3e-3..2.9e-3
    (restatement 3.1e-3..3.4e-3), d bias 8e-8: the oracle error is above the 1e-3 floor everywhere but d bias."""
    dev = _gpu()
    shape = dict(N=1, C=120, Cout=120, H=11, W=21, dg=8)
    d = _inputs(9, mode=mode, **shape)
    y, g = _hip(d, mode, dev, "bf16")
    y_o, g_o = _oracle(d, mode)
    y_e, g_e = _oracle(d, mode, store=bf16_store)
    e = _errors(y, g, y_o, g_o, d, mode, shape["H"], shape["W"])
    e_emu = _errors(y_e, g_e, y_o, g_o, d, mode, shape["H"], shape["W"])
    print("bf16", mode, "hip", e, "restatement", e_emu)
    for k in e:
        assert e[k] <= 1.5 * max(e_emu[k], FLOOR16), (k, e[k], e_emu[k])


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_fused_flow_guided_equals_plain_on_formed_offsets(compute_dtype):
    from vsrlab_amd import functional as VF
    dev = _gpu()
    shape = dict(N=2, C=32, Cout=32, H=13, W=37, dg=4)
    d = _inputs(11, mode="flow", **shape)
    y, g = _hip(d, "flow", dev, compute_dtype)
    t = {k: v.to(device=dev, dtype=torch.float32) for k, v in d.items()}
    off, mask = VF.flow_guided_offset_mask(t["out"], t["flow"], 10.0)
    off.requires_grad_(True); mask.requires_grad_(True)
    x = t["x"].clone().requires_grad_(True)
    w = t["weight"].clone().requires_grad_(True)
    y2 = VF.deform_conv2d(x, off, w, t["bias"], mask=mask, compute_dtype=compute_dtype)
    assert torch.equal(y, y2.detach())
    (y2 * t["cot"]).sum().backward()
    # chain rule through the epilogue, in torch
    raw = t["out"].clone().requires_grad_(True)
    fl = t["flow"].clone().requires_grad_(True)
    o_t, m_t = DC.flow_guided_offset_mask_ref(raw, fl, 10.0)
    ((o_t * off.grad).sum() + (m_t * mask.grad).sum()).backward()
    assert rel_l2(g["out"], raw.grad) < 1e-5 and rel_l2(g["flow"], fl.grad) < 1e-5
    assert rel_l2(g["x"], x.grad) < 1e-5 and rel_l2(g["weight"], w.grad) < 1e-5


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_repeatability_and_no_grad_bits(compute_dtype):
    from vsrlab_amd import functional as VF
    dev = _gpu()
    shape = dict(N=2, C=120, Cout=120, H=13, W=37, dg=8)
    d = _inputs(13, mode="flow", **shape)
    y1, g1 = _hip(d, "flow", dev, compute_dtype)
    y2, g2 = _hip(d, "flow", dev, compute_dtype)
    assert torch.equal(y1, y2)
    for k in ("weight", "bias", "out", "flow"):
        assert torch.equal(g1[k], g2[k]), k
    assert rel_l2(g1["x"], g2["x"]) < 1e-6
    t = {k: v.to(device=dev, dtype=torch.float32) for k, v in d.items()}
    with torch.no_grad():
        y3 = VF.flow_guided_deform_conv(t["x"], t["out"], t["flow"], t["weight"], t["bias"], 10.0, compute_dtype=compute_dtype)
    assert torch.equal(y1, y3)


def test_autograd_contract():
    from vsrlab_amd import functional as VF
    dev = _gpu()
    d = _inputs(15, mode="plain", N=1, C=32, Cout=32, H=8, W=9, dg=4)
    t = {k: v.to(device=dev, dtype=torch.float32) for k, v in d.items()}
    x = t["x"].clone().requires_grad_(True)
    y = VF.deform_conv2d(x, t["offset"], t["weight"], t["bias"])
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        y.sum().backward()
    y = VF.deform_conv2d(x, t["offset"], t["weight"], t["bias"])
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(y.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        VF.deform_conv2d(torch.zeros(1, 256, 8, 8, device=dev), torch.zeros(1, 18, 8, 8, device=dev), torch.zeros(8, 256, 3, 3, device=dev))


def _z():
    return np.load(os.path.join(GOLDEN, "deform_conv.npz"), allow_pickle=False)


def _check_golden(z, tag, key, val, tol):
    val = val.detach().double().cpu()
    stats = torch.from_numpy(z[f"{tag}__stats__{key}"])
    if f"{tag}__{key}" in z.files:
        e = rel_l2(val, torch.from_numpy(z[f"{tag}__{key}"]))
    else:
        e = float((val.flatten()[::sub_stride(val.numel())] - torch.from_numpy(z[f"{tag}__sub__{key}"])).norm() / stats[1] *
                  sub_stride(val.numel()) ** 0.5)
    e_norm = abs(float(val.norm() / stats[1]) - 1)
    e_proj = abs(float((val * proj_vector(f"{tag}.{key}", tuple(val.shape))).sum() - stats[2])) / float(stats[1])
    print(tag, key, f"rel-L2 {e:.2e} norm {e_norm:.2e} proj {e_proj:.2e}")
    assert e < tol and e_norm < tol and e_proj < 3 * tol, (tag, key, e, e_norm, e_proj)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_dcnv2_flow_guided_module_matches_the_golden(tag):
    from vsrlab_amd.vsr.models.VRT.modules.deform_conv import DCNv2PackFlowGuided
    dev = _gpu()
    z = _z()
    c = DC.DCN_CASES[tag]
    m = DCNv2PackFlowGuided(c["C"], c["C"], 3, padding=1, deformable_groups=c["dg"], max_residue_magnitude=10, pa_frames=2)
    m.load_state_dict(DC.dcn_state_dict(m.state_dict(), tag, torch.float32), strict=True)
    m = m.to(dev)
    x, warped, cur, flow, cot = (t.to(dev).requires_grad_(True) for t in DC.dcn_inputs(tag, torch.float32))
    y = m(x, [warped], cur, [flow])
    (y * cot.detach()).sum().backward()
    torch.cuda.synchronize()
    _check_golden(z, tag, "y", y, TOL32)
    for name, t in (("dx", x), ("dwarped", warped), ("dcur", cur)):
        _check_golden(z, tag, name, t.grad, TOL32)
    named = dict(m.named_parameters())
    for k in ("weight", "bias", "conv_offset.0.weight", "conv_offset.6.weight"):
        _check_golden(z, tag, "grad__" + k.replace(".", "_"), named[k].grad, TOL32)
    # d flow: leave out the pixels with a kinked tap (fp64 positions from the restatement of the same wiring)
    sd = DC.dcn_state_dict(m.state_dict(), tag)
    xs = DC.dcn_inputs(tag)
    h = torch.cat([xs[1], xs[2], xs[3]], dim=1)
    for i in (0, 2, 4, 6):
        h = F.conv2d(h, sd[f"conv_offset.{i}.weight"], sd[f"conv_offset.{i}.bias"], padding=1)
        h = F.leaky_relu(h, 0.1) if i < 6 else h
    near = DC.near_integer(DC.flow_guided_offset_mask_ref(h, xs[3], 10.0)[0], c["H"], c["W"])
    assert float(near.double().mean()) <= 1e-3
    keep = (~near).all(dim=1).all(dim=1).unsqueeze(1).double()
    gold = torch.from_numpy(z[f"{tag}__dflow"])
    assert rel_l2(flow.grad.double().cpu() * keep, gold * keep) < TOL32


def test_deform_block_matches_the_golden():
    from vsrlab_amd.core.modules.conv import DeformBlock
    dev = _gpu()
    z = _z()
    c = DC.BLOCK_CASE
    m = DeformBlock(c["cin"], c["mid"], c["blocks"])
    m.load_state_dict(DC.block_state_dict(m.state_dict(), torch.float32), strict=True)
    m = m.to(dev)
    x, cot = (t.to(dev) for t in DC.block_inputs(torch.float32))
    x.requires_grad_(True)
    y = m(x)
    (y * cot).sum().backward()
    torch.cuda.synchronize()
    _check_golden(z, "blk", "y", y, TOL32)
    _check_golden(z, "blk", "dx", x.grad, TOL32)
    for k, p in m.named_parameters():
        _check_golden(z, "blk", "grad__" + k.replace(".", "_"), p.grad, TOL32)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k


def test_stage_call_pattern():
    """stage.py:109-129 on a 3-frame toy: warp the neighbour's features with the flow, align with pa_deform"""
    from vsrlab_amd.vsr.models.VRT.modules.deform_conv import DCNv2PackFlowGuided
    from vsrlab_amd.vsr.models.VRT.modules.spynet import flow_warp
    dev = _gpu()
    torch.manual_seed(0)
    C, H, W = 32, 16, 24
    pa = DCNv2PackFlowGuided(C, C, 3, padding=1, deformable_groups=4, max_residue_magnitude=10, pa_frames=2).to(dev)
    with torch.no_grad():
        pa.conv_offset[-1].weight.normal_(0, 0.02)
    x = torch.randn(1, 3, C, H, W, device=dev)
    flows = (torch.rand(1, 2, 2, H, W, device=dev) * 4 - 2).requires_grad_(True)
    feats = []
    for i in range(2, 0, -1):                          # backward direction: align frame i to frame i - 1
        flow = flows[:, i - 1]
        warped = flow_warp(x[:, i], flow.permute(0, 2, 3, 1), "bilinear")
        feats.append(pa(x[:, i], [warped], x[:, i - 1], [flow]))
    out = torch.stack(feats, 1)
    assert out.shape == (1, 2, C, H, W) and torch.isfinite(out).all()
    out.square().mean().backward()
    assert torch.isfinite(flows.grad).all() and float(flows.grad.abs().max()) > 0


def test_full_size_bf16():
    """config 5's first stage: 15 frame pairs of 120 channels at 184 x 320, 8 deformable groups"""
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    dev = _gpu()
    N, C, H, W, dg = 15, 120, 184, 320, 8
    g = torch.Generator(device="cpu").manual_seed(21)
    x = torch.randn(N, C, H, W, generator=g).to(dev)
    raw = (torch.randn(N, 27 * dg, H, W, generator=g) * 0.6).to(dev)
    flow = ((torch.rand(N, 2, H, W, generator=g) * 2 - 1) * 6).to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5).to(dev)
    b = (torch.randn(C, generator=g) * 0.1).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        y = VF.flow_guided_deform_conv(x, raw, flow, w, b, 10.0, compute_dtype="bf16")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ws = VF.deform_conv_workspace_bytes((N, C, H, W), C, dg, _lib.DT_BF16, False)
    assert peak <= ws + y.numel() * 4 + (64 << 20), (peak, ws, y.numel() * 4)      # 64 MiB: allocator block rounding
    assert torch.isfinite(y).all()
    e_hip = e_emu = 0.0
    for n in range(0, N, 5):                           # the restatement, one image at a time (3.8 GB of columns per 15)
        sl = slice(n, n + 1)
        y32 = DC.flow_guided_deform_conv_ref(x[sl], raw[sl], flow[sl], w, b, 10.0)
        y16 = DC.flow_guided_deform_conv_ref(x[sl], raw[sl], flow[sl], w, b, 10.0, store=bf16_store)
        e_hip, e_emu = max(e_hip, rel_err(y[sl], y32)), max(e_emu, rel_err(y16, y32))
    print(f"full size bf16: y max-rel {e_hip:.3e}, bf16-storage restatement {e_emu:.3e}")
    assert e_hip <= 1.5 * max(e_emu, FLOOR16)
    # and one backward at this size: finite everywhere
    xg, rg, fg, wg = (t.clone().requires_grad_(True) for t in (x, raw, flow, w))
    VF.flow_guided_deform_conv(xg, rg, fg, wg, b, 10.0, compute_dtype="bf16").mean().backward()
    torch.cuda.synchronize()
    for t in (xg, rg, fg, wg):
        assert torch.isfinite(t.grad).all() and float(t.grad.abs().max()) > 0
