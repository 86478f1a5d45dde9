"""What the tests of LossPipeline, WL1Loss, rmse_loss and the differentiable resize share with tests/golden/make_golden_losses.py:
the case of tests/golden/loss_pipeline.npz (inputs, configuration) and its restatement in plain torch, which the host test pins to
the reference's recorded fp64 results and the GPU tests use as their checker at other shapes and dtypes."""
import torch
import torch.nn.functional as F

from helpers import rand

PREFIX, POSTFIX = "train/", "_g"
L1_WEIGHT = 0.5
CHARB_EPS = 1e-9
# charb on the prediction, L1 of the pre-cleaned frames against the down-sampled target, RMSE of the up-sampled pre-cleaned frames
# against the target, and L1 once more: `l1` is named twice and accumulates into one key
PIPELINE = [{"charb": {"x": "sr", "y": "hr"}}, {"l1": {"x": "lq", "y": "match_hr"}}, {"rmse": {"x": "match_lq", "y": "hr"}},
            {"l1": {"x": "sr", "y": "hr"}}]
PIPELINE_ORDER = [name for cfg in PIPELINE for name in cfg]
OUTPUT_KEYS = [PREFIX + name + POSTFIX for name in ("charb", "l1", "rmse", "loss")]
SINGLE_L1_WEIGHT = 2.0


def pipeline_inputs():
    """sr, hr (1, 2, 3, 16, 24) and lq (1, 2, 3, 5, 7), fp32 values in [0, 1)."""
    return rand(701, 1, 2, 3, 16, 24), rand(702, 1, 2, 3, 16, 24), rand(703, 1, 2, 3, 5, 7)


def single_inputs():
    """the ragged pair of the single-loss records"""
    return rand(704, 1, 2, 3, 5, 7), rand(705, 1, 2, 3, 5, 7)


def interp(x, size):
    """kornia.geometry.transform.resize(x, size) with its defaults = bilinear F.interpolate(align_corners=False) over the flattened
    leading dimensions (tests/test_training_glue.py::test_resize_matches_interpolate)"""
    H, W = x.shape[-2:]
    return F.interpolate(x.reshape(-1, 1, H, W), size=tuple(size), mode="bilinear", align_corners=False).reshape(*x.shape[:-2], *size)


def charbonnier(x, y, eps=CHARB_EPS):
    d = x - y
    return torch.mean(torch.sqrt(d * d + eps))


def l1(x, y):
    return torch.mean(torch.abs(x - y))


def rmse(x, y):
    return torch.sqrt(torch.mean((x - y) ** 2))


def restate_pipeline(sr, hr, lq, prefix=PREFIX, postfix=POSTFIX):
    """PIPELINE on the three tensors, in their dtype (the checker calls it in fp64): every output key, accumulated in pipeline order"""
    terms = [("charb", charbonnier(sr, hr)), ("l1", L1_WEIGHT * l1(lq, interp(hr, lq.shape[-2:]))),
             ("rmse", rmse(interp(lq, hr.shape[-2:]), hr)), ("l1", L1_WEIGHT * l1(sr, hr))]
    out = {prefix + k + postfix: 0 for k in ("charb", "l1", "rmse", "loss")}
    for name, v in terms:
        out[prefix + name + postfix] = out[prefix + name + postfix] + v
        out[prefix + "loss" + postfix] = out[prefix + "loss" + postfix] + v
    return out
