"""The reference's metric side (``src/core/metrics.py`` + the ``piqa.PSNR`` / ``piqa.SSIM`` its YAML instantiates,
conf/train/default.yaml:8-14) on the HIP path.

``PSNR`` and ``SSIM`` take piqa's constructor keywords and compute piqa's defaults' definition; both run
``vsrlab_amd.functional.psnr_ssim``, one kernel pass that yields both numbers, and have no CPU fallback.  ``MetricCollection``
behaves as the reference's; when it holds exactly one ``PSNR`` and one ``SSIM`` of this module with the same ``value_range`` it
makes one kernel call and one device-to-host copy for both numbers.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from ..functional import psnr_ssim

_REDUCTIONS = ("mean", "sum", "none")


def _reduce(v: torch.Tensor, reduction: str) -> torch.Tensor:
    if reduction == "mean":
        return v.mean()
    return v.sum() if reduction == "sum" else v


def _psnr_from_mse(mse: torch.Tensor, value_range: float, epsilon: float) -> torch.Tensor:
    return 10.0 * torch.log10(value_range ** 2 / (mse + epsilon))


class _Metric(nn.Module):
    def __init__(self, value_range: float, reduction: str):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
        self.value_range = float(value_range)
        self.reduction = reduction

    @staticmethod
    def _check(x: torch.Tensor, y: torch.Tensor) -> None:
        if x.dim() != 4 or x.shape != y.shape:
            raise ValueError(f"expected two (N, C, H, W) tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")


class PSNR(_Metric):
    """``piqa.PSNR``: 10 log10(value_range^2 / (mse + epsilon)) per image, mse over (C, H, W).

    Called on its own it still runs the fused pass (the squared error is summed where the SSIM tiles are staged), with the largest
    odd window up to 11 that fits the image.  So, unlike piqa's PSNR, it needs images of at least 3 x 3 and raises ``ValueError``
    below that."""

    def __init__(self, epsilon: float = 1e-8, value_range: float = 1., reduction: str = "mean"):
        super().__init__(value_range, reduction)
        self.epsilon = float(epsilon)

    def _from(self, res) -> torch.Tensor:
        return _reduce(_psnr_from_mse(res.mse, self.value_range, self.epsilon), self.reduction).to(torch.float32)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        self._check(x, y)
        ws = min(11, int(min(x.shape[-2:])))                    # the pass computes an SSIM too: its window only has to fit
        return self._from(psnr_ssim(x, y, window_size=ws - (ws % 2 == 0), value_range=self.value_range))


class SSIM(_Metric):
    """``piqa.SSIM`` with its defaults' definition: Gaussian window, no padding, mean of the map over (C, H', W') per image."""

    def __init__(self, window_size: int = 11, sigma: float = 1.5, n_channels: int = 3, value_range: float = 1., k1: float = 0.01,
                 k2: float = 0.03, reduction: str = "mean"):
        super().__init__(value_range, reduction)
        self.window_size, self.sigma, self.n_channels, self.k1, self.k2 = int(window_size), float(sigma), int(n_channels), float(k1), float(k2)

    def _kwargs(self) -> dict:
        return dict(window_size=self.window_size, sigma=self.sigma, value_range=self.value_range, k1=self.k1, k2=self.k2)

    def _from(self, res) -> torch.Tensor:
        return _reduce(res.ssim, self.reduction).to(torch.float32)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        self._check(x, y)
        if x.shape[1] != self.n_channels:
            raise ValueError(f"SSIM was built for {self.n_channels} channels, got {x.shape[1]}")
        return self._from(psnr_ssim(x, y, **self._kwargs()))


class MetricCollection(nn.ModuleDict):
    """A dictionary of metric modules that is called like one metric, with the behaviour of the reference's collection
    (core/metrics.py): the entries are kept in the order of their sorted keys, every value must be an ``nn.Module`` and every key
    new (``ValueError`` otherwise), ``clone`` gives an independent copy under another prefix / postfix, and a call returns
    ``{prefix + key + postfix: float}``.

    ``forward(*args, clamp=(lo, hi))`` clamps the first argument (the prediction): inside the kernel on the fused path, with
    ``Tensor.clamp`` otherwise."""

    def __init__(self, metrics, prefix=None, postfix=None):
        super().__init__()
        self.prefix, self.postfix = prefix, postfix
        for key in sorted(metrics):
            self.register(key, metrics[key])

    def register(self, key: str, module: nn.Module) -> None:
        """Add one metric under a key the collection does not have yet."""
        if key in self:
            raise ValueError(f"the collection already has a metric named {key!r}")
        if not isinstance(module, nn.Module):
            raise ValueError(f"metric {key!r} must be an nn.Module, got {type(module).__name__}")
        self[key] = module

    def clone(self, prefix=None, postfix=None):
        """A deep copy; a prefix / postfix that is given (and not empty) replaces the copy's own."""
        twin = copy.deepcopy(self)
        twin.prefix = prefix or self.prefix
        twin.postfix = postfix or self.postfix
        return twin

    def _named(self, values: dict) -> dict:
        head, tail = self.prefix or "", self.postfix or ""
        return {head + key + tail: values[key] for key in self.keys()}

    def _fused_pair(self):
        """(key of the PSNR, key of the SSIM) when one pass serves the whole collection, else None."""
        if len(self) != 2:
            return None
        by_type = {type(m): k for k, m in self.items()}
        if set(by_type) != {PSNR, SSIM} or self[by_type[PSNR]].value_range != self[by_type[SSIM]].value_range:
            return None
        return by_type[PSNR], by_type[SSIM]

    def forward(self, *args, clamp=None):
        pair = self._fused_pair()
        if pair is not None and len(args) == 2:
            psnr, ssim = self[pair[0]], self[pair[1]]
            x, y = args
            ssim._check(x, y)
            if x.shape[1] != ssim.n_channels:
                raise ValueError(f"SSIM was built for {ssim.n_channels} channels, got {x.shape[1]}")
            res = psnr_ssim(x, y, clamp=clamp, **ssim._kwargs())
            both = torch.stack([psnr._from(res).double().reshape(-1), ssim._from(res).double().reshape(-1)]).cpu()   # the one copy
            return self._named({pair[0]: both[0].item(), pair[1]: both[1].item()})
        if clamp is not None:
            args = (args[0].clamp(float(clamp[0]), float(clamp[1])),) + tuple(args[1:])
        return self._named({key: module(*args).item() for key, module in self.items()})
