"""Keyed VGG19 weights and a pure-torch restatement of PerceptualLoss (core/losses.py:29-64), shared by the perceptual tests and
tests/golden/make_golden_perceptual.py.  Weights are never stored: both sides regenerate them from the state_dict key."""
import zlib

import torch
import torch.nn.functional as F

LAYER_WEIGHTS = {'2': 0.1, '7': 0.1, '16': 0.8, '25': 0.9, '34': 1.0}
CONVS = ((0, 64, 3), (2, 64, 64), (5, 128, 64), (7, 128, 128), (10, 256, 128), (12, 256, 256), (14, 256, 256), (16, 256, 256),
         (19, 512, 256), (21, 512, 512), (23, 512, 512), (25, 512, 512), (28, 512, 512), (30, 512, 512), (32, 512, 512),
         (34, 512, 512))
POOL_AFTER = (2, 7, 16, 25)            # a MaxPool2d(2, 2) follows the ReLU of these convs


def keyed_vgg_state_dict(prefix="vgg.vgg_layers.", dtype=torch.float32):
    """He-scaled keyed weights: randn seeded by crc32(key) * sqrt(2 / (9 cin)); biases randn * 0.01."""
    sd = {}
    for idx, co, ci in CONVS:
        for name, shape, s in (("weight", (co, ci, 3, 3), (2.0 / (9 * ci)) ** 0.5), ("bias", (co,), 0.01)):
            key = f"{prefix}{idx}.{name}"
            g = torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7fffffff)
            sd[key] = (torch.randn(*shape, generator=g, dtype=torch.float64) * s).to(dtype)
    return sd


def param_list(sd, prefix="vgg.vgg_layers."):
    return [sd[f"{prefix}{idx}.{n}"] for idx, _, _ in CONVS for n in ("weight", "bias")]


def vgg_taps(x, params, store=None):
    """The five taps of features[:35] as the reference stores them: 2, 7, 16, 25 post-ReLU, 34 pre-ReLU.  ``store``: optional
    rounding applied where the bf16 build stores a tensor (conv outputs after the activation, pool outputs)."""
    st = store or (lambda t: t)
    taps = []
    for j, (idx, _, _) in enumerate(CONVS):
        x = F.conv2d(x, params[2 * j], params[2 * j + 1], padding=1)
        if idx != 34:
            x = st(F.relu(x))
        else:
            x = st(x)
        if str(idx) in LAYER_WEIGHTS:
            taps.append(x)
        if idx in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return taps


def perceptual_terms(sr, hr, params, weight=1.0, store=None):
    """The five weighted terms weight * LAYER_WEIGHTS[k] * l1_loss(f_k(sr), f_k(hr)) (sr, hr: (..., 3, h, w))."""
    h, w = hr.shape[-2:]
    fs = vgg_taps(sr.reshape(-1, 3, h, w), params, store)
    with torch.no_grad():
        fh = vgg_taps(hr.reshape(-1, 3, h, w), params, store)
    return torch.stack([weight * lw * F.l1_loss(a, b) for lw, a, b in zip(LAYER_WEIGHTS.values(), fs, fh)])
