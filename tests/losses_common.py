"""What the tests of LossPipeline, WL1Loss, rmse_loss and the differentiable resize share with tests/golden/make_golden_losses.py:
the case of tests/golden/loss_pipeline.npz (inputs, configuration) and its restatement in plain torch, which the host test pins to
the reference's recorded fp64 results and the GPU tests use as their checker at other shapes and dtypes; and the summation order of
vsr_pixel_loss_fwd_bwd (csrc/pixel_losses.hip on csrc/reduce.h), restated in numpy fp32, which the order tests pin bit for bit."""
import numpy as np
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


# ---- the summation order of vsr_pixel_loss_fwd_bwd ------------------------------------------------------------------------------
ORDER_BLOCK, ORDER_BLOCKS, ORDER_VEC = 256, 1024, 8
ORDER_SIZES = (1, 7, 8, 2051, 12293, 2107395)      # 7: tail only; 2051: one workgroup, 4 live waves, a tail; the last: > 1024 * 256 * 8
ORDER_SEED = 755                                   # one at which both wrong orders of emulate_pair_loss_order give other bits, for L1 and MSE


def order_operands(n, seed=ORDER_SEED):
    """x, y: n fp32 values each, bf16-representable, uniform in (-1, 1)"""
    return tuple(rand(seed + k, n, lo=-1.0, hi=1.0).bfloat16().float() for k in (0, 1))


def pair_loss_terms(x, y, kind):
    """the fp32 terms |x - y| ("l1") or (x - y)^2 ("mse") as the kernel forms them: one rounding each"""
    d = np.asarray(x, dtype=np.float32) - np.asarray(y, dtype=np.float32)
    return np.abs(d) if kind == "l1" else d * d


def pair_loss_launch(n, aligned=True):
    """(blocks, elements per lane and trip, trips of the grid-stride loop) of the entry for n elements"""
    vec = ORDER_VEC if aligned else 1
    items = n // vec
    blocks = min(max(-(-items // ORDER_BLOCK), 1), ORDER_BLOCKS)
    return blocks, vec, max(-(-items // (blocks * ORDER_BLOCK)), 1)


def emulate_pair_loss_order(x, y, kind, combine="pairwise", final="tree", aligned=True):
    """The fp32 value vsr_pixel_loss_fwd_bwd returns for the flat fp32 operands x, y, addition by addition as the entry is written
    (csrc/pixel_losses.hip, csrc/reduce.h):
      * 16-byte aligned pointers: a lane adds 8 consecutive elements per trip, blocks = clamp(ceil((n // 8) / 256), 1, 1024)
        workgroups of 256 lanes, grid stride blocks * 256, and the n % 8 tail elements on the first lanes of workgroup 0;
        otherwise (`aligned=False`) one element per trip, blocks from ceil(n / 256), no tail;
      * the 64-lane shuffle tree (offsets 32 ... 1), the pairwise combiner (r0 + r1) + (r2 + r3) of the four wave sums, times
        fp32(1 / n): one partial per workgroup;
      * one workgroup of 256: thread t adds partials t, t + 256, ..., then the halving tree from 128 down.
    combine="inorder" (((0 + r0) + r1) + r2) + r3 and final="inorder" (one running sum over the partials) are deliberately WRONG
    orders: the order tests require that they give other bits."""
    f32 = np.float32
    t = pair_loss_terms(x, y, kind)
    n = t.size
    blocks, vec, trips = pair_loss_launch(n, aligned)
    lanes = blocks * ORDER_BLOCK
    body = (n // vec) * vec
    grid = np.zeros(trips * lanes * vec, dtype=f32)               # adding the +0 of a lane that has no element changes nothing
    grid[:body] = t[:body]
    grid = grid.reshape(trips, lanes, vec)
    local = np.zeros(lanes, dtype=f32)
    for k in range(trips):
        for j in range(vec):
            local = local + grid[k, :, j]
    local[:n - body] = local[:n - body] + t[body:]                # the tail: workgroup 0, lanes 0 .. n % 8 - 1
    v = local.reshape(blocks, ORDER_BLOCK // 64, 64).copy()
    o = 32
    while o:                                                      # lane l += lane l + o; only lanes below o matter from here on
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    r = v[..., 0]
    if combine == "pairwise":
        s = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    else:
        assert combine == "inorder"
        s = (((f32(0) + r[:, 0]) + r[:, 1]) + r[:, 2]) + r[:, 3]
    partial = s * (f32(1.0) / f32(n))
    if final == "inorder":
        total = f32(0)
        for p in partial:
            total = total + p
        return f32(total)
    assert final == "tree"
    rounds = -(-blocks // ORDER_BLOCK)
    pad = np.zeros(rounds * ORDER_BLOCK, dtype=f32)
    pad[:blocks] = partial
    red = np.zeros(ORDER_BLOCK, dtype=f32)
    for k in range(rounds):
        red = red + pad[k * ORDER_BLOCK:(k + 1) * ORDER_BLOCK]
    o = ORDER_BLOCK // 2
    while o:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return f32(red[0])
