"""CPU-side checks of the metric surface: the restatement of tests/metrics_common.py against closed forms, MetricCollection's
behaviour, the descriptor checks of the C ABI, the opt-in piqa alias and evaluate_video's windowing."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import metrics_common as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (0.0, 1.0), (0.5, 0.5)])
def test_restatement_matches_the_closed_form_on_constant_images(a, b):
    x, y = torch.full((2, 3, 16, 19), a, dtype=torch.float64), torch.full((2, 3, 16, 19), b, dtype=torch.float64)
    c1 = 0.01 ** 2
    assert float((MC.ssim(x, y) - (2 * a * b + c1) / (a * a + b * b + c1)).abs().max()) < 1e-12
    assert float((MC.psnr(x, y) - 10 * math.log10(1 / ((a - b) ** 2 + 1e-8))).abs().max()) < 1e-12


def test_restatement_on_identical_images():
    x = torch.rand(2, 3, 20, 23, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    assert float((MC.ssim(x, x) - 1).abs().max()) < 1e-12
    assert float((MC.psnr(x, x) - 80).abs().max()) < 1e-12
    assert abs(float(MC.gaussian_taps().sum()) - 1) < 1e-15 and tuple(MC.ssim_map(x, x).shape) == (2, 3, 10, 13)


class _L1(nn.Module):
    def forward(self, x, y):
        return (x - y).abs().mean()


class _MaxErr(nn.Module):
    def forward(self, x, y):
        return (x - y).abs().max()


def test_metric_collection_names_sorting_and_clone():
    from vsrlab_amd.core.metrics import MetricCollection
    mc = MetricCollection({"zeta": _L1(), "alpha": _MaxErr()}, prefix="val/")
    assert list(mc.keys()) == ["alpha", "zeta"]
    x, y = torch.zeros(2, 3, 4, 4), torch.full((2, 3, 4, 4), 0.25)
    y[0, 0, 0, 0] = 0.5
    out = mc(x, y)
    assert list(out) == ["val/alpha", "val/zeta"] and all(type(v) is float for v in out.values())
    assert out["val/alpha"] == 0.5 and abs(out["val/zeta"] - float((x - y).abs().mean())) < 1e-7
    test = mc.clone(prefix="test/", postfix="_db")
    assert list(test(x, y)) == ["test/alpha_db", "test/zeta_db"] and list(mc(x, y)) == ["val/alpha", "val/zeta"]
    assert test["alpha"] is not mc["alpha"]
    assert list(mc.clone()(x, y)) == ["val/alpha", "val/zeta"]
    assert list(MetricCollection({"m": _L1()}, postfix="@1")(x, y)) == ["m@1"]
    # the slow path clamps the prediction when asked to
    assert mc(x - 1, y, clamp=(0, 1)) == out


def test_metric_collection_rejects_non_modules_and_duplicates():
    from vsrlab_amd.core.metrics import MetricCollection
    with pytest.raises(ValueError):
        MetricCollection({"a": _L1(), "b": lambda x, y: 0})
    mc = MetricCollection({"a": _L1()})
    with pytest.raises(ValueError):
        mc.register("a", _MaxErr())
    with pytest.raises(ValueError):
        mc.register("b", 3.0)
    mc.register("b", _MaxErr())
    assert list(mc.keys()) == ["a", "b"]


def test_psnr_and_ssim_take_piqa_keywords_and_have_no_cpu_fallback():
    from vsrlab_amd.core.metrics import PSNR, SSIM, MetricCollection
    p = PSNR(epsilon=1e-8, value_range=1., reduction="mean")
    s = SSIM(window_size=11, sigma=1.5, n_channels=3, value_range=1., k1=0.01, k2=0.03, reduction="none")
    assert isinstance(p, nn.Module) and isinstance(s, nn.Module)
    with pytest.raises(ValueError):
        PSNR(reduction="median")
    x = torch.rand(2, 3, 16, 16)
    for call in (lambda: p(x, x), lambda: s(x, x), lambda: MetricCollection({"PSNR": p, "SSIM": SSIM()})(x, x, clamp=(0, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_functional_validation():
    from vsrlab_amd import functional as VF
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError):
        VF.psnr_ssim(x, torch.zeros(1, 3, 16, 17))
    with pytest.raises(RuntimeError):
        VF.psnr_ssim(x, x)


def _desc(H=32, W=32, ws=11, planes=6, C=3):
    from vsrlab_amd import _lib
    return _lib.MetricsDesc(planes, C, H, W, ws, 1.5, 1e-4, 9e-4, 1, 0.0, 1.0)


def test_scratch_query_rejects_unsupported_descriptors():
    from vsrlab_amd import _lib
    lib = _lib.load()
    for name in ("vsr_metrics_scratch_bytes", "vsr_psnr_ssim"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.vsr_abi_version() == 4
    q = lambda d: int(lib.vsr_metrics_scratch_bytes(ctypes.byref(d)))
    assert q(_desc()) > 0 and q(_desc(H=11, W=11)) > 0
    assert q(_desc(H=10)) == 0
    assert q(_desc(W=10)) == 0
    assert q(_desc(ws=10)) == 0
    assert q(_desc(ws=17)) == 0
    assert q(_desc(planes=7)) == 0                        # not whole images
    # one fp64 pair per tile of every plane; more tiles for a larger image
    assert q(_desc(H=2160, W=3840, planes=42)) > q(_desc(H=1080, W=1920, planes=42)) > 0
    assert q(_desc(H=2160, W=3840, planes=42)) < (1 << 20)
    # a failing call on the CPU box: the descriptor is checked before anything is launched
    assert lib.vsr_psnr_ssim(ctypes.byref(_desc(ws=10)), None, None, None, None, 0, None) == -2


def test_piqa_alias_is_opt_in_and_resolves_when_piqa_is_absent():
    code = (
        "import importlib.util, sys\n"
        "real = importlib.util.find_spec('piqa') is not None\n"
        "import vsrlab_amd, vsrlab_amd.compat as C, vsrlab_amd.core.metrics as M\n"
        "assert real or 'piqa' not in sys.modules\n"
        "done = C.install_metrics_as_piqa()\n"
        "assert done == (not real)\n"
        "if done:\n"
        "    m = C.instantiate({'_target_': 'piqa.PSNR'}); s = C.instantiate({'_target_': 'piqa.SSIM'})\n"
        "    import piqa\n"
        "    assert piqa.PSNR is M.PSNR and piqa.SSIM is M.SSIM and type(m) is M.PSNR and type(s) is M.SSIM\n"
        "    assert C.install_metrics_as_piqa()\n"
        "print('ok', done)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


class _Nearest4(nn.Module):
    """stub model: x4 nearest upsampling plus the index of the call, returned as RealBasicVSR returns (sr, lq)"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, lr):
        assert not self.training and not torch.is_grad_enabled()
        self.calls.append(lr.shape[1])
        b, t, c, h, w = lr.shape
        sr = torch.nn.functional.interpolate(lr.reshape(b * t, c, h, w), scale_factor=4, mode="nearest").reshape(b, t, c, 4 * h, 4 * w)
        return sr + 0.1 * (len(self.calls) - 1), lr


def test_evaluate_video_windows_average_and_concatenate():
    from vsrlab_amd.core.metrics import MetricCollection
    from vsrlab_amd.core.utils import compute_metric
    from vsrlab_amd.evaluate import evaluate_video
    g = torch.Generator().manual_seed(11)
    lr, hr = torch.rand(1, 70, 3, 4, 6, generator=g), torch.rand(1, 70, 3, 16, 24, generator=g)
    metric = MetricCollection({"L1": _L1(), "Max": _MaxErr()})
    model = _Nearest4().train()
    sr, out = evaluate_video(model, lr, hr, metric, window_size=32)
    assert model.calls == [32, 32, 6] and tuple(sr.shape) == (1, 70, 3, 16, 24)
    windows = [(0, 32), (32, 64), (64, 70)]
    up = lambda a: torch.nn.functional.interpolate(a.reshape(-1, 3, 4, 6), scale_factor=4, mode="nearest").reshape(1, -1, 3, 16, 24)
    per = []
    for k, (i, j) in enumerate(windows):
        want = up(lr[:, i:j]) + 0.1 * k
        assert torch.equal(sr[:, i:j], want)
        per.append(compute_metric(metric, want, hr[:, i:j]))
    for k in ("L1", "Max"):
        assert out[k] == pytest.approx(sum(p[k] for p in per) / 3, rel=1e-12)
    # every window weighs the same: the frame-weighted mean is a different number
    frames = sum(p["L1"] * (j - i) for p, (i, j) in zip(per, windows)) / 70
    assert abs(out["L1"] - frames) > 1e-4
    # any callable works as the metric, as in the reference: it gets the clamped prediction
    bare = compute_metric(lambda x, y: {"n": float(x.max()), "shape": tuple(x.shape)}, torch.full((1, 2, 3, 4, 4), 1.5), torch.ones(1, 2, 3, 4, 4))
    assert bare == {"n": 1.0, "shape": (2, 3, 4, 4)}
    # compute_metric clamps the prediction and not the target
    x5 = torch.full((1, 2, 3, 4, 4), 1.5)
    assert compute_metric(metric, x5, torch.ones(1, 2, 3, 4, 4))["L1"] == 0.0
    assert compute_metric(metric, torch.ones(1, 2, 3, 4, 4), x5)["L1"] == 0.5
