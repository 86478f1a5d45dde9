"""GPU tests of the narrow widths (mid_channels 16 / 32: vsr_basicvsr_narrow_*, the pre-clean stack and the per-op layers at
C channels) against the reference's goldens and the fp64 oracle.  Criteria as in test_hip_parity.py: fp32 within 1e-3 of fp64
(_fp32_check), bf16 no worse than 1.5 x the error of the bf16-storage-emulating oracle (_floor_check)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import golden, rand, rel_err, rel_l2, realbasicvsr_oracle_grads, realbasicvsr_shapes

pytestmark = pytest.mark.gpu

from oracle import basicvsr_oracle as O  # noqa: E402  (checker only)

DTYPES = ["fp32", "bf16"]
BF16_FLOOR = 1e-3


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _floor_check(got, emu, ref, floor, glob_ratio=1.5, tensor_ratio=2.5):
    """got's error against `ref` <= ratio x the same-precision CPU evaluation's error `emu` (globally and per tensor)."""
    keys = sorted(ref)
    cat = lambda d: torch.cat([d[k].double().flatten() for k in keys])
    e_got, e_emu = rel_l2(cat(got), cat(ref)), rel_l2(cat(emu), cat(ref))
    assert e_got <= glob_ratio * max(e_emu, floor), ("global", e_got, e_emu)
    for k in keys:
        eg, ee = rel_l2(got[k], ref[k]), rel_l2(emu[k], ref[k])
        assert eg <= tensor_ratio * max(ee, floor), (k, eg, ee)


def _fp32_check(got, o32, ref):
    """fp32: within 1e-3 of the fp64 values globally (relative L2 over all tensors), or within 1.5 x the fp32 oracle's own error
    where that is larger (ReLU / LeakyReLU mask flips grow with the number of pixels); per tensor no worse than 2.5 x the fp32
    oracle's own error or 5e-3 (test_hip_parity.test_basicvsr_end_to_end_vs_golden)."""
    keys = sorted(ref)
    cat = lambda d: torch.cat([d[k].double().flatten() for k in keys])
    e_got, e_o32 = rel_l2(cat(got), cat(ref)), rel_l2(cat(o32), cat(ref))
    assert e_got < max(1e-3, 1.5 * e_o32), ("global", e_got, e_o32)
    for k in keys:
        eg, eo = rel_l2(got[k], ref[k]), rel_l2(o32[k], ref[k])
        assert eg <= max(2.5 * eo, 5e-3), (k, eg, eo)


def _model(mid, rb, up, dtype, dev, train_flow=False):
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    m = BasicVSR(mid, rb, up, False, train_flow)
    sd = O.keyed_state_dict(O.basicvsr_param_shapes(mid, rb, up))
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    m.compute_dtype = dtype
    return m, sd


def _fwd_bwd(m, lrs, cot, dev):
    m.zero_grad(set_to_none=True)
    sr = m(lrs.to(dev))
    torch.mean(sr * cot.to(dev)).backward()
    return sr.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}


def _check_vs_oracle(dtype, sd, lrs, cot, sr, grads):
    sr_x, _, g_x = O.fwd_bwd({k: v.double() for k, v in sd.items()}, lrs.double(), torch.zeros_like(cot).double(), cot=cot.double())
    if dtype == "fp32":
        sr_o, _, g_o = O.fwd_bwd(sd, lrs, torch.zeros_like(cot), cot=cot)
        assert rel_err(sr, sr_x) < 1e-3
        _fp32_check(grads, g_o, g_x)
    else:
        with O.emulate_bf16():
            sr_e, _, g_e = O.fwd_bwd(sd, lrs, torch.zeros_like(cot), cot=cot)
        assert rel_err(sr, sr_x) <= 1.5 * max(rel_err(sr_e, sr_x), BF16_FLOOR)
        _floor_check(grads, g_e, g_x, BF16_FLOOR)


# ---- per op --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mid", [16, 32])
def test_narrow_modules_forward_and_backward_vs_oracle(dtype, mid):
    """ResidualConv(C), ResidualBlock(3 + C, C, 2) on cat([lr, feat]), ResidualBlock(3, C, 2) and PixelShufflePack(C, C, 2):
    output, input gradient and every parameter gradient against autograd on the oracle's restatements."""
    dev = _gpu()
    from vsrlab_amd.core.modules.conv import ResidualBlock, ResidualConv
    from vsrlab_amd.core.modules.upsampling import PixelShufflePack
    os.environ["VSRLAB_AMD_DTYPE"] = dtype

    def check(name, mod, ref_fn, x, seed):
        sd = O.keyed_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items()})
        mod.load_state_dict(sd, strict=True)
        mod = mod.to(dev)
        xg = x.clone().to(dev).requires_grad_(True)
        y = mod(xg)
        cot = rand(seed, *y.shape, lo=-1, hi=1)
        (y * cot.to(dev)).sum().backward()
        got = {"x": xg.grad.cpu(), **{k: p.grad.cpu() for k, p in mod.named_parameters()}}
        leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xr = x.double().requires_grad_(True)
        yr = ref_fn(leaves, xr)
        (yr * cot.double()).sum().backward()
        want = {"x": xr.grad, **{k: v.grad for k, v in leaves.items()}}
        assert tuple(y.shape) == tuple(yr.shape), name
        if dtype == "fp32":
            assert rel_err(y.detach(), yr.detach()) < 1e-3, name
            for k in want:
                assert rel_l2(got[k], want[k]) < 1e-3, (name, k, rel_l2(got[k], want[k]))
        else:
            with O.emulate_bf16():
                l32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
                x32 = x.clone().requires_grad_(True)
                ye = ref_fn(l32, x32)
                (ye * cot).sum().backward()
            emu = {"x": x32.grad, **{k: v.grad for k, v in l32.items()}}
            assert rel_err(y.detach(), yr.detach()) <= 1.5 * max(rel_err(ye.detach(), yr.detach()), 2e-2), name
            for k in want:
                assert rel_l2(got[k], want[k]) <= 1.5 * max(rel_l2(emu[k], want[k]), 2e-2), (name, k, rel_l2(got[k], want[k]), rel_l2(emu[k], want[k]))

    try:
        check("ResidualConv", ResidualConv(mid), lambda sd, x: O.residual_conv(sd, "", O._q(x)), rand(80 + mid, 2, mid, 13, 37, lo=-1, hi=1), 81)
        for cin in (3 + mid, 3):
            check(f"ResidualBlock{cin}", ResidualBlock(cin, mid, 2), lambda sd, x: O.residual_block(sd, "", O._q(x), 2),
                  rand(61 + cin, 2, cin, 13, 37, lo=-1, hi=1), 71)
        check("PixelShufflePack", PixelShufflePack(mid, mid, 2), lambda sd, x: O.pixel_shuffle_pack(sd, "", O._q(x)),
              rand(62, 2, mid, 7, 9, lo=-1, hi=1), 72)
    finally:
        del os.environ["VSRLAB_AMD_DTYPE"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mid", [16, 32])
def test_narrow_flow_warp_and_gather_adjoint(dtype, mid):
    """flow_warp at C channels against the oracle, and the engine's gather-form adjoint at C channels
    (vsr_debug_warp_bwd_gather_c) against the scatter form on flows with far sources; S comes back all-zero."""
    dev = _gpu()
    from vsrlab_amd import _lib, functional as VF
    lib = _lib.load()
    dt = VF.resolve_dtype(dtype)
    n, h, w = 2, 37, 70
    x = rand(1400 + mid, n, mid, h, w, lo=-1, hi=1)
    flow = rand(1401, n, 2, h, w, lo=-3, hi=3)
    flow[:, 0, :, 20:45] += 7.0                                       # a band of far sources (|dx| > 4)
    os.environ["VSRLAB_AMD_DTYPE"] = dtype
    try:
        out = VF.flow_warp(x.to(dev), flow.permute(0, 2, 3, 1).to(dev))
    finally:
        del os.environ["VSRLAB_AMD_DTYPE"]
    xin = x if dtype == "fp32" else x.to(torch.bfloat16).float()
    assert rel_err(out, O.flow_warp(xin, flow, "zeros")) < (1e-5 if dtype == "fp32" else 1e-2)
    fn = lib.vsr_debug_warp_bwd_gather_c
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    fl = flow.to(dev).contiguous()
    cot = rand(1402, n, mid, h, w, lo=-1, hi=1).to(dev)
    top = rand(1403, n, mid, h, w, lo=-1, hi=1).to(dev)
    g, t = VF.to_pixel_major(cot, dt), VF.to_pixel_major(top, dt)
    o = torch.empty_like(g)
    S = torch.zeros(n * h * w * mid, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    assert fn(dt, VF._ptr(g), VF._ptr(fl), VF._ptr(t), VF._ptr(S), VF._ptr(cnt), VF._ptr(o), n, h, w, mid, VF._stream()) == 0
    o.pm_w = w
    got = VF.from_pixel_major(o, mid)
    far = int(cnt.item())
    assert far & 0x3fffffff > 0 and not (far & 0x40000000) and int(S.abs().max()) == 0
    acc = torch.zeros((n, h, w, mid), dtype=torch.float32, device=dev)
    assert lib.vsr_flow_warp_bwd_ex(dt, VF._ptr(g), VF._ptr(fl), VF._ptr(acc), n, h, w, mid, 0, VF._stream()) == 0
    want = acc.permute(0, 3, 1, 2) + VF.from_pixel_major(t, mid)
    assert rel_err(got, want) < (1e-5 if dtype == "fp32" else 1e-2)


# ---- end to end against the reference's goldens ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_basicvsr_m16_vs_reference_golden(dtype):
    """BasicVSR(16, 2) at (1,3,3,32,32): sr, the Charbonnier loss, both flows (vsr_basicvsr_narrow_get_flows) and the 11 stored
    parameter gradients against the reference's own fp64 values."""
    dev = _gpu()
    import vsrlab_amd
    from vsrlab_amd import functional as VF
    from vsrlab_amd._order import basicvsr_keys
    g = golden("basicvsr_m16_rb2")
    shape = (1, 3, 3, 32, 32)
    m, sd = _model(16, 2, 4, dtype, dev)
    lrs = rand(int(g["seed_lr"]), *shape)
    hr = rand(int(g["seed_hr"]), 1, 3, 3, 128, 128)
    cot = rand(int(g["seed_cot"]), 1, 3, 3, 128, 128, lo=-1, hi=1)
    sr, grads = _fwd_bwd(m, lrs, cot, dev)
    ref = {k[len("grad__"):].replace("__", "."): v for k, v in g.items() if k.startswith("grad__")}
    assert len(ref) == 11
    loss = O.charbonnier(sr.double(), hr.double())
    if dtype == "fp32":
        assert rel_err(sr, g["sr"]) < 1e-3
        assert abs(float(loss) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
        _, _, g32 = O.fwd_bwd(sd, lrs, hr, cot=cot)
        _fp32_check(grads, g32, ref)
    else:
        with O.emulate_bf16():
            sr_e, _, g_e = O.fwd_bwd(sd, lrs, hr, cot=cot)
        assert rel_err(sr, g["sr"]) <= 1.5 * max(rel_err(sr_e, g["sr"]), BF16_FLOOR)
        assert abs(float(loss) - float(g["loss"])) < 2e-2 * abs(float(g["loss"]))
        _floor_check(grads, g_e, ref, BF16_FLOOR)
    lib = vsrlab_amd._lib.load()
    keys, _ = basicvsr_keys(2)
    ps = [sd[k].to(dev).contiguous() for k in keys]
    dt = VF.resolve_dtype(dtype)
    desc = vsrlab_amd._lib.BasicVSRDesc(1, 3, 32, 32, 16, 2, 4, dt)
    assert lib.vsr_basicvsr_workspace_bytes(ctypes.byref(desc), 0) == 0
    nbytes = lib.vsr_basicvsr_narrow_workspace_bytes(ctypes.byref(desc), 0)
    ws = VF.Workspace(nbytes, dev)
    sr2 = torch.empty(1, 3, 3, 128, 128, device=dev)
    assert lib.vsr_basicvsr_narrow_forward(ctypes.byref(desc), VF._ptr_array(ps), len(ps), VF._ptr(lrs.to(dev)), VF._ptr(sr2),
                                           VF._ptr(ws.buf), nbytes, 0, VF._stream()) == 0
    ff, fb = VF.basicvsr_flows(shape, 16, 2, 4, ws, dt, dev)
    t = (1e-3, 1e-3) if dtype == "fp32" else (1e-2, 5e-2)
    assert rel_err(sr2, g["sr"]) < t[0]
    assert rel_err(ff.reshape(-1, 2, 32, 32).cpu(), g["flow_forward"]) < t[1]
    assert rel_err(fb.reshape(-1, 2, 32, 32).cpu(), g["flow_backward"]) < t[1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_realbasicvsr_m16_inference_vs_reference_golden(dtype):
    dev = _gpu()
    from vsrlab_amd.vsr.models.RealBasicVSR.realbasicvsr import RealBasicVSR
    g = golden("realbasicvsr_m16")
    m = RealBasicVSR(2, mid_channels=16, upscale=4, res_blocks=2, pretrained_flow=False, train_flow=False)
    m.load_state_dict(O.keyed_state_dict(realbasicvsr_shapes(16, 2, 2)), strict=True)
    m = m.to(dev).eval()
    m.basicvsr.compute_dtype = dtype
    lrs = rand(g["seed_lr"], 1, 3, 3, 32, 32).to(dev)
    os.environ["VSRLAB_AMD_DTYPE"] = dtype
    try:
        with torch.no_grad():
            sr, lq = m(lrs)
    finally:
        del os.environ["VSRLAB_AMD_DTYPE"]
    assert rel_err(lq, g["lq"]) < (1e-3 if dtype == "fp32" else 2e-2)
    assert rel_err(sr, g["sr"]) < (1e-3 if dtype == "fp32" else 3e-2)


# ---- against the fp64 oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up", [4, 2])
def test_basicvsr_mid32_ragged_vs_oracle(dtype, up):
    """mid 32, 3 blocks, (2,3,3,24,40): every trainable gradient, upscale 4 and 2."""
    dev = _gpu()
    m, sd = _model(32, 3, up, dtype, dev)
    lrs = rand(301, 2, 3, 3, 24, 40)
    cot = rand(302, 2, 3, 3, up * 24, up * 40, lo=-1, hi=1)
    sr, grads = _fwd_bwd(m, lrs, cot, dev)
    assert len(grads) == len([k for k in sd if "spynet" not in k])
    _check_vs_oracle(dtype, sd, lrs, cot, sr, grads)


def test_basicvsr_mid16_train_flow_and_input_gradient_vs_oracle():
    """train_flow=True with the gradient into the clip (need_backward = 2), fp32: the 60 SPyNet gradients and lrs.grad."""
    dev = _gpu()
    m, sd = _model(16, 2, 4, "fp32", dev, train_flow=True)
    lrs = rand(311, 1, 3, 3, 32, 32)
    cot = rand(312, 1, 3, 3, 128, 128, lo=-1, hi=1)
    lg = lrs.clone().to(dev).requires_grad_(True)
    torch.mean(m(lg) * cot.to(dev)).backward()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    leaves = {k: v.double().requires_grad_(not k.endswith(("mean", "std"))) for k, v in sd.items()}
    lo = lrs.double().requires_grad_(True)
    torch.mean(O.basicvsr_forward(leaves, lo) * cot.double()).backward()
    ref = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    spy = [k for k in ref if k.startswith("spynet")]
    assert len(spy) == 60 and set(grads) == set(ref)
    # (fp32 ReLU-mask noise of SPyNet's coarse-to-fine recursion: test_hip_parity.test_basicvsr_train_flow_vs_golden's bounds)
    g = torch.cat([grads[k].double().flatten() for k in spy])
    r = torch.cat([ref[k].double().flatten() for k in spy])
    assert rel_l2(g, r) < 1.5e-2
    assert float(torch.dot(g, r) / (g.norm() * r.norm())) > 0.9999
    assert rel_l2(lg.grad, lo.grad) < 2e-2
    assert rel_l2(grads["conv_last.2.weight"], ref["conv_last.2.weight"]) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mid", [16, 32])
def test_realbasicvsr_narrow_training_vs_oracle(dtype, mid):
    """sr, lq = RealBasicVSR(lr) at mid 16 / 32 with a two-term loss: every trainable gradient, the pre-clean stack's
    backward through the narrow cleaner entries fed by d lq from the narrow BasicVSR engine."""
    dev = _gpu()
    from vsrlab_amd.vsr.models.RealBasicVSR.realbasicvsr import RealBasicVSR
    sd32 = O.keyed_state_dict(realbasicvsr_shapes(mid, 2, 2))
    m = RealBasicVSR(2, mid_channels=mid, upscale=4, res_blocks=2, pretrained_flow=False, train_flow=False)
    m.load_state_dict(sd32, strict=True)
    m = m.to(dev)
    m.basicvsr.compute_dtype = dtype
    shape = (1, 3, 3, 24, 40)
    n, t, _, h, w = shape
    lr = rand(14, *shape)
    cot_sr = rand(15, n, t, 3, 4 * h, 4 * w, lo=-1, hi=1)
    cot_lq = rand(16, n, t, 3, h, w, lo=-1, hi=1)
    os.environ["VSRLAB_AMD_DTYPE"] = dtype
    try:
        sr, lq = m(lr.to(dev))
        (torch.mean(sr * cot_sr.to(dev)) + torch.mean(lq * cot_lq.to(dev))).backward()
    finally:
        del os.environ["VSRLAB_AMD_DTYPE"]
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    sr_o, lq_o, ref = realbasicvsr_oracle_grads({k: v.double() for k, v in sd32.items()}, lr.double(), cot_sr.double(), cot_lq.double())
    assert set(grads) == set(ref)
    if dtype == "fp32":
        assert rel_err(lq, lq_o) < 1e-4 and rel_err(sr, sr_o) < 1e-3
        _, _, g32 = realbasicvsr_oracle_grads(sd32, lr, cot_sr, cot_lq)
        _fp32_check(grads, g32, ref)
    else:
        with O.emulate_bf16():
            sr_e, lq_e, g_e = realbasicvsr_oracle_grads(sd32, lr, cot_sr, cot_lq)
        assert rel_err(lq, lq_o) <= 1.5 * max(rel_err(lq_e, lq_o), BF16_FLOOR)
        assert rel_err(sr, sr_o) <= 1.5 * max(rel_err(sr_e, sr_o), BF16_FLOOR)
        _floor_check(grads, g_e, ref, BF16_FLOOR)


def test_basicvsr_mid32_moderate_shape_vs_oracle():
    """mid 32, 5 blocks, (1,7,3,180,320), fp32: many workgroups and tiles per launch, all frames per weight-gradient launch."""
    dev = _gpu()
    m, sd = _model(32, 5, 4, "fp32", dev)
    lrs = rand(321, 1, 7, 3, 180, 320)
    cot = rand(322, 1, 7, 3, 720, 1280, lo=-1, hi=1)
    sr, grads = _fwd_bwd(m, lrs, cot, dev)
    _check_vs_oracle("fp32", sd, lrs, cot, sr, grads)


# ---- schedule invariants --------------------------------------------------------------------------
def test_mid32_bf16_arenas_repeatability_inference_and_optimizer():
    dev = _gpu()
    from vsrlab_amd import functional as VF
    from vsrlab_amd.optim import FusedAdam
    m, _ = _model(32, 3, 4, "bf16", dev)
    lrs = rand(331, 1, 10, 3, 24, 40)
    cot = rand(332, 1, 10, 3, 96, 160, lo=-1, hi=1)
    out = {}
    for mode in ("full", "diet"):
        VF.set_arena_mode(mode)
        try:
            out[mode] = _fwd_bwd(m, lrs, cot, dev)
        finally:
            VF.set_arena_mode(None)
    assert torch.equal(out["full"][0], out["diet"][0])
    for k, v in out["full"][1].items():
        assert rel_l2(out["diet"][1][k], v) < 1e-5, (k, rel_l2(out["diet"][1][k], v))
    again = _fwd_bwd(m, lrs, cot, dev)
    assert torch.equal(again[0], out["full"][0])
    assert all(torch.equal(again[1][k], v) for k, v in out["full"][1].items())
    with torch.no_grad():                                               # t = 32, inference
        sr = m(rand(333, 1, 32, 3, 24, 40).to(dev))
    assert sr.shape == (1, 32, 3, 96, 160) and bool(torch.isfinite(sr).all())
    m16, _ = _model(16, 2, 4, "bf16", dev)
    before = [p.detach().clone() for p in m16.parameters() if p.requires_grad]
    opt = FusedAdam(m16.parameters(), lr=1e-3, max_grad_norm=1.0)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss = VF.charbonnier_loss(m16(lrs[:, :3].to(dev)), rand(334, 1, 3, 3, 96, 160).to(dev))
        loss.backward()
        opt.step()
    assert bool(torch.isfinite(loss))
    after = [p.detach() for p in m16.parameters() if p.requires_grad]
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
