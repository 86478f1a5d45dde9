"""The definition of PSNR and SSIM that the metric kernel is held to, restated in plain torch (``F.conv2d`` with groups, no
padding) and able to run in fp64.

piqa, whose defaults the reference's YAML uses, is not a dependency of this repository and no golden recorded from it can exist,
so parity of ``vsrlab_amd.functional.psnr_ssim`` / ``vsrlab_amd.core.metrics`` is pinned by this restatement ALONE.  The
restatement itself is checked against closed forms in tests/test_metrics_host.py."""
import torch
import torch.nn.functional as F


def gaussian_taps(window_size=11, sigma=1.5, dtype=torch.float64, device=None):
    i = torch.arange(window_size, dtype=dtype, device=device)
    g = torch.exp(-(i - (window_size - 1) / 2) ** 2 / (2 * sigma ** 2))
    return g / g.sum()


def _blur(t, g):
    c = t.shape[1]
    t = F.conv2d(t, g.reshape(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)
    return F.conv2d(t, g.reshape(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)


def ssim_map(x, y, window_size=11, sigma=1.5, value_range=1.0, k1=0.01, k2=0.03):
    """ss of shape (N, C, H - ws + 1, W - ws + 1), in the dtype of x."""
    g = gaussian_taps(window_size, sigma, x.dtype, x.device)
    c1, c2 = (k1 * value_range) ** 2, (k2 * value_range) ** 2
    mx, my = _blur(x, g), _blur(y, g)
    sxx, syy, sxy = _blur(x * x, g) - mx * mx, _blur(y * y, g) - my * my, _blur(x * y, g) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    return (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs


def ssim(x, y, **kw):
    """per image, shape (N,)"""
    return ssim_map(x, y, **kw).mean(dim=(1, 2, 3))


def psnr(x, y, value_range=1.0, epsilon=1e-8):
    """per image, shape (N,)"""
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    return 10 * torch.log10(value_range ** 2 / (mse + epsilon))


def reference(sr, hr, clamp=(0.0, 1.0), dtype=torch.float64, **kw):
    """(psnr, ssim) per image of compute_metric's inputs: sr clamped, hr as it is, evaluated in `dtype`."""
    x, y = sr.to(dtype), hr.to(dtype)
    if clamp is not None:
        x = x.clamp(clamp[0], clamp[1])
    return psnr(x, y, value_range=kw.get("value_range", 1.0)), ssim(x, y, **kw)


def precision_bound(e32, value):
    """The parity bound of the GPU tests: 4 x max(deviation of the fp32 CPU evaluation of this restatement, 16 ulp of fp32 at the
    value's magnitude)."""
    return 4 * max(float(e32), 16 * 2.0 ** -24 * max(1.0, abs(float(value))))


def smooth_pair(h=48, w=80, seed=71):
    """hr: a smooth (1, 3, h, w) image in [0.2, 0.8] (bilinear upsampling of a random 6 x 10 one)."""
    g = torch.Generator().manual_seed(seed)
    small = torch.rand(1, 3, 6, 10, generator=g)
    return (0.2 + 0.6 * F.interpolate(small, size=(h, w), mode="bilinear", align_corners=False)).contiguous()
