"""The fused PSNR / SSIM kernel and the metric surface over it on the GPU, against the fp64 restatement of tests/metrics_common.py
(the only oracle there is: see that file's docstring).

The kernel works on 64 x 256 tiles of SSIM outputs, so the shapes below include one that is two tiles plus
one pixel in both directions, (139, 523), and the tile-corner case of the locality test uses a 96 x 300 image whose output has
an interior tile corner at (64, 256); the 48 x 80 image of the other positions is a single tile of this kernel."""
import pytest
import torch

import metrics_common as MC
from helpers import rand

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _pair(seed, shape):
    """sr in [-0.2, 1.2] (so the clamp matters), hr in [0, 1]"""
    return rand(seed, *shape, lo=-0.2, hi=1.2), rand(seed + 1, *shape)


def _gpu_metrics(sr, hr, dev, clamp=(0.0, 1.0), **kw):
    """(psnr, ssim) per image in fp64 on the CPU, from one fused call"""
    from vsrlab_amd import functional as VF
    res = VF.psnr_ssim(sr.to(dev), hr.to(dev), clamp=clamp, **kw)
    vr = kw.get("value_range", 1.0)
    return (10 * torch.log10(vr ** 2 / (res.mse + 1e-8))).cpu(), res.ssim.cpu()


def _check_parity(sr, hr, dev, what, **kw):
    p64, s64 = MC.reference(sr, hr, **kw)
    p32, s32 = MC.reference(sr, hr, dtype=torch.float32, **kw)
    pg, sg = _gpu_metrics(sr, hr, dev, **kw)
    for name, got, r64, r32 in (("psnr", pg, p64, p32), ("ssim", sg, s64, s32)):
        e32 = float((r32.double() - r64).abs().max())
        err = float((got - r64).abs().max())
        bound = MC.precision_bound(e32, r64.abs().max())
        print(f"{what} {name}: gpu deviation {err:.3e}, fp32 CPU deviation e32 {e32:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, name, err, e32, bound)


PARITY_CASES = [
    ((2, 3, 11, 11), {}),                                 # one output pixel
    ((3, 3, 37, 70), {}),                                 # ragged, W not a multiple of 4: scalar loads
    ((2, 3, 75, 141), {}),                                # two tile rows
    ((1, 2, 139, 523), {}),                               # 2 tiles + 1 pixel in both directions (129 x 513 outputs), scalar loads
    ((1, 1, 139, 524), {}),                               # the same tiling through the 16-byte loads
    ((1, 1, 12, 300), {}),                                # thin strips
    ((1, 1, 300, 12), {}),
    ((2, 3, 33, 40), dict(window_size=7, sigma=1.0)),
]


@pytest.mark.parametrize("shape,kw", PARITY_CASES, ids=["x".join(map(str, s)) + ("_w7" if k else "") for s, k in PARITY_CASES])
def test_parity_with_the_fp64_restatement(shape, kw):
    dev = _gpu()
    sr, hr = _pair(100 + shape[-1], shape)
    _check_parity(sr, hr, dev, str(shape), **kw)


def _deficit_case(dev, hr, pos, delta):
    from vsrlab_amd import functional as VF
    sr = hr.clone()
    sr[0, 1, pos[0], pos[1]] += delta
    assert 0.0 <= float(sr.min()) and float(sr.max()) <= 1.3
    n_out = 3 * (hr.shape[-2] - 10) * (hr.shape[-1] - 10)
    want = n_out - float(MC.ssim_map(sr.double(), hr.double()).sum())
    res = VF.psnr_ssim(sr.to(dev), hr.to(dev))
    got = n_out - float(res.ss_sum[0].cpu())
    print(f"pixel {pos} {delta:+}: deficit {got:.6f}, restatement {want:.6f}, relative deviation {abs(got / want - 1):.2e}")
    assert want > 1.0 and abs(got / want - 1) < 1e-3, (pos, got, want)
    assert abs(float(res.sq_err_sum[0].cpu()) - delta * delta) < 1e-6


@pytest.mark.parametrize("pos", [(20, 5), (31, 63), (32, 64)])
def test_one_moved_pixel_costs_what_the_restatement_says(pos):
    """locality and halos: every SSIM output within 5 pixels of the moved pixel changes, and nothing else does"""
    dev = _gpu()
    hr = MC.smooth_pair(48, 80)
    _deficit_case(dev, hr, pos, 0.5 if float(hr[0, 1, pos[0], pos[1]]) < 0.5 else -0.5)


@pytest.mark.parametrize("pos", [(63, 255), (63, 256), (64, 255), (64, 256), (68, 260)])
def test_one_moved_pixel_at_a_tile_corner(pos):
    """The four pixels around the interior corner of the kernel's 64 x 256 output tiles, and one a few pixels past it.  The outputs
    a pixel (r, c) touches are rows r-10..r, columns c-10..c: (63, 255) changes outputs of tile (0, 0) alone, (63, 256) and
    (64, 255) straddle one seam each with a single column / row beyond it, (64, 256) has one row and one column in the other
    three tiles, and (68, 260) has five rows and five columns on the far side and six on the near side of both seams."""
    dev = _gpu()
    hr = MC.smooth_pair(96, 300)
    _deficit_case(dev, hr, pos, 0.5 if float(hr[0, 1, pos[0], pos[1]]) < 0.5 else -0.5)


def test_exactness_cases():
    from vsrlab_amd import functional as VF
    dev = _gpu()
    c1 = 0.01 ** 2
    for a, b in ((0.3, 0.7), (1.0, 0.0), (0.25, 0.25)):
        x, y = torch.full((2, 3, 40, 50), a), torch.full((2, 3, 40, 50), b)
        _check_parity(x, y, dev, f"constant {a}/{b}")
        pg, sg = _gpu_metrics(x, y, dev)
        x64, y64 = float(x[0, 0, 0, 0].double()), float(y[0, 0, 0, 0].double())          # the fp32 values the kernel saw
        want = (2 * x64 * y64 + c1) / (x64 * x64 + y64 * y64 + c1)
        assert float((sg - want).abs().max()) <= MC.precision_bound(0.0, want)
    hr = rand(7, 2, 3, 45, 67)
    pg, sg = _gpu_metrics(hr, hr, dev)
    print(f"sr is hr: ssim - 1 = {float((sg - 1).abs().max()):.3e}, psnr - 80 = {float((pg - 80).abs().max()):.3e}")
    assert float((sg - 1).abs().max()) <= 1e-6 and float((pg - 80).abs().max()) <= 1e-4
    sr = rand(8, 2, 3, 45, 67)
    a, b = VF.psnr_ssim(sr.to(dev), hr.to(dev), clamp=None), VF.psnr_ssim(sr.to(dev), hr.to(dev), clamp=(0.0, 1.0))
    assert torch.equal(a.mse, b.mse) and torch.equal(a.ssim, b.ssim)


def test_determinism_and_batch_independence():
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core.metrics import PSNR, SSIM, MetricCollection
    dev = _gpu()
    sr, hr = _pair(31, (5, 3, 40, 72))
    sr, hr = sr.to(dev), hr.to(dev)
    a, b = VF.psnr_ssim(sr, hr, clamp=(0.0, 1.0)), VF.psnr_ssim(sr, hr, clamp=(0.0, 1.0))
    assert torch.equal(a.mse, b.mse) and torch.equal(a.ssim, b.ssim)
    for i in range(5):
        one = VF.psnr_ssim(sr[i:i + 1], hr[i:i + 1], clamp=(0.0, 1.0))
        assert torch.equal(one.mse[0], a.mse[i]) and torch.equal(one.ssim[0], a.ssim[i])
    out = MetricCollection({"PSNR": PSNR(), "SSIM": SSIM()})(sr, hr, clamp=(0.0, 1.0))
    assert out["SSIM"] == a.ssim.mean().float().item()
    assert out["PSNR"] == (10 * torch.log10(1 / (a.mse + 1e-8))).mean().float().item()


def test_many_planes():
    """70 002 planes: more than a grid's y or z dimension holds"""
    dev = _gpu()
    sr, hr = _pair(41, (23334, 3, 11, 11))
    pg, sg = _gpu_metrics(sr, hr, dev)
    assert bool(torch.isfinite(pg).all()) and bool(torch.isfinite(sg).all())
    pick = [0, 1, 23333]
    p64, s64 = MC.reference(sr[pick], hr[pick])
    p32, s32 = MC.reference(sr[pick], hr[pick], dtype=torch.float32)
    for got, r64, r32 in ((pg[pick], p64, p32), (sg[pick], s64, s32)):
        assert float((got - r64).abs().max()) <= MC.precision_bound(float((r32.double() - r64).abs().max()), r64.abs().max())


def test_collection_fast_path_equals_the_modules():
    from vsrlab_amd.core.metrics import PSNR, SSIM, MetricCollection
    dev = _gpu()
    sr, hr = _pair(51, (3, 3, 30, 44))
    x, y = sr.clamp(0, 1).to(dev), hr.to(dev)
    both = MetricCollection({"SSIM": SSIM(), "PSNR": PSNR()}, prefix="val/")(x, y)
    assert list(both) == ["val/PSNR", "val/SSIM"] and all(type(v) is float for v in both.values())
    assert both["val/PSNR"] == PSNR()(x, y).item() and both["val/SSIM"] == SSIM()(x, y).item()
    assert tuple(SSIM(reduction="none")(x, y).shape) == (3,) and SSIM()(x, y).device == x.device and SSIM()(x, y).dim() == 0
    assert PSNR(reduction="sum")(x, y).item() == pytest.approx(3 * both["val/PSNR"], rel=1e-6)
    # a different value_range, or a third metric: every module is called on its own
    slow = MetricCollection({"PSNR": PSNR(value_range=2.), "SSIM": SSIM()})(x, y)
    assert slow["SSIM"] == both["val/SSIM"] and slow["PSNR"] == PSNR(value_range=2.)(x, y).item()
    with pytest.raises(ValueError):
        SSIM()(x[:, :, :10], y[:, :, :10])


def test_compute_metric_and_strided_input():
    from vsrlab_amd.core.metrics import PSNR, SSIM, MetricCollection
    from vsrlab_amd.core.utils import compute_metric, running_metrics
    dev = _gpu()
    metric = MetricCollection({"PSNR": PSNR(), "SSIM": SSIM()})
    sr, hr = _pair(61, (2, 3, 3, 24, 40))
    p64, s64 = MC.reference(sr.reshape(6, 3, 24, 40), hr.reshape(6, 3, 24, 40))
    p32, s32 = MC.reference(sr.reshape(6, 3, 24, 40), hr.reshape(6, 3, 24, 40), dtype=torch.float32)
    out = compute_metric(metric, sr.to(dev).requires_grad_(True), hr.to(dev))
    # the collection returns fp32 means: one more rounding to fp32 on top of the kernel's bound
    for k, r64, r32 in (("PSNR", p64, p32), ("SSIM", s64, s32)):
        want = float(r64.mean())
        bound = MC.precision_bound(float((r32.double() - r64).abs().max()), want) + 2.0 ** -24 * max(1.0, abs(want))
        assert abs(out[k] - want) <= bound, (k, out[k], want, bound)
    total = running_metrics({"PSNR": 1.0, "SSIM": 2.0, "other": 0.0}, metric, sr.to(dev), hr.to(dev))
    assert total == {"PSNR": 1.0 + out["PSNR"], "SSIM": 2.0 + out["SSIM"]}
    # a slice along t is not contiguous: it is copied, and gives what its copy gives
    big_sr, big_hr = _pair(63, (2, 5, 3, 24, 40))
    big_sr, big_hr = big_sr.to(dev), big_hr.to(dev)
    view_sr, view_hr = big_sr[:, 1:4], big_hr[:, 1:4]
    assert not view_sr.is_contiguous()
    assert compute_metric(metric, view_sr, view_hr) == compute_metric(metric, view_sr.contiguous(), view_hr.contiguous())


def test_evaluate_video_with_the_hip_model():
    from oracle import basicvsr_oracle as O
    from vsrlab_amd.core.metrics import PSNR, SSIM, MetricCollection
    from vsrlab_amd.core.utils import compute_metric
    from vsrlab_amd.evaluate import evaluate_video
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    dev = _gpu()
    m = BasicVSR(64, 2, 4, False, False)
    m.load_state_dict(O.keyed_state_dict(O.basicvsr_param_shapes(64, 2, 4)), strict=True)
    m = m.to(dev)
    lr, hr = rand(81, 1, 5, 3, 16, 24).to(dev), rand(82, 1, 5, 3, 64, 96).to(dev)
    metric = MetricCollection({"PSNR": PSNR(), "SSIM": SSIM()})
    calls = []
    hook = m.register_forward_hook(lambda mod, args, out: calls.append(args[0].shape[1]))
    sr, out = evaluate_video(m, lr, hr, metric, window_size=2)
    hook.remove()
    assert calls == [2, 2, 1] and tuple(sr.shape) == (1, 5, 3, 64, 96) and not m.training
    per = []
    with torch.no_grad():
        for i in (0, 2, 4):
            w = m(lr[:, i:i + 2])
            assert torch.equal(w, sr[:, i:i + 2])
            per.append(compute_metric(metric, w, hr[:, i:i + 2]))
    for k in ("PSNR", "SSIM"):
        assert out[k] == (per[0][k] + per[1][k] + per[2][k]) / 3
