"""Case table and CPU oracle of the integer-tap warps (csrc/warp_taps.hip): ``flow_warp(..., 'nearest' / 'nearest4')`` and VRT's
aligned input.  The oracle restates the specification of DESIGN section 11h in numpy -- one fp32 add per coordinate, floor / ceil /
rint, a range test on the float, a gather; gradients as a scatter in fp64 -- and tests/test_warp_taps_host.py pins it to the
reference's recorded results (tests/golden/warp_taps.npz) bit for bit.  Shared by the host test, the GPU test and the golden maker."""
import zlib

import numpy as np
import torch

# name -> (x shape, what the flow is); what each case catches:
#   tiny     smallest legal extent, every border at once
#   odd      about 60 % of the taps out of frame; batch stride
#   wide     two columns past a 64-lane row; width not a multiple of 4
#   chan     C != 3; odd width, so rows are not 16-byte aligned
#   feat     flow_warp on a feature map: the channel loop
#   integer  floor == ceil: four equal taps; the backward adds four times to one pixel
#   edge     positions exactly -1, -0.5, 0, W-1, W-0.5, W (likewise for rows): the <= W-1 test and -0.0 (ceil(-0.5))
#   far      +-1e6 and +-3e9: the range test is made in float, beyond int32
#   vec      a width that is a multiple of 8 (every row 16-byte aligned in both dtypes), more than one block, batch stride
CASES = {
    "tiny": ((1, 1, 2, 2), ("uniform", 2.0)),
    "odd": ((2, 3, 5, 7), ("uniform", 4.0)),
    "wide": ((1, 3, 9, 66), ("uniform", 4.0)),
    "chan": ((2, 5, 17, 33), ("uniform", 4.0)),
    "feat": ((1, 64, 8, 12), ("uniform", 3.0)),
    "integer": ((1, 3, 6, 10), ("integer", 3)),
    "edge": ((1, 3, 6, 10), ("edge", None)),
    "far": ((1, 3, 4, 6), ("far", None)),
    "vec": ((2, 3, 10, 72), ("uniform", 4.0)),
}
BORDER_GOLDEN = ("tiny", "odd", "integer", "edge", "far")       # cases whose 'border' outputs are recorded from the reference
# (B, D) by frame shape (C, H, W) of the aligned input; D = 2 is the smallest: one pair, both zero blocks adjacent
CLIP_CASES = [(b, d, f) for f in ((3, 6, 10), (3, 9, 66)) for b, d in ((1, 2), (2, 3), (1, 6))]
CLIP_GOLDEN = [(1, 2, (3, 6, 10)), (2, 3, (3, 6, 10)), (1, 6, (3, 6, 10)), (1, 2, (3, 9, 66))]   # recorded from the reference


def clip_name(b, d, f):
    return "clip_b%d_d%d_%dx%dx%d" % ((b, d) + tuple(f))


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7fffffff)


def case_x(name, dtype=torch.float32, shape=None):
    """the seeded input in [-1, 1); for bf16 it is rounded first (the op is a gather: the output is then exact)"""
    shape = shape or CASES[name][0]
    return (torch.rand(shape, generator=_gen("x:" + name)) * 2 - 1).to(dtype)


def _uniform_flow(key, n, h, w, amp):
    return (torch.rand(n, 2, h, w, generator=_gen("flow:" + key)) * 2 - 1) * amp


def case_flow(name, taps=4):
    """planar (N, 2, H, W) fp32 flow, plane 0 horizontal.  For taps = 1 ('nearest') every flow is an integer plus a fraction in
    [0.05, 0.45] or [0.55, 0.95]: the reference finds the tap through a normalise / un-normalise round trip in fp32 that can move a
    position within an ulp of .5 to the other side; with these fractions no case depends on it and nothing is exempted."""
    (n, _, h, w), (kind, arg) = CASES[name]
    g = _gen("flow:" + name)
    if kind == "uniform":
        flow = _uniform_flow(name, n, h, w, arg)
    elif kind == "integer":
        flow = torch.randint(-arg, arg + 1, (n, 2, h, w), generator=g).to(torch.float32)
    elif kind == "edge":
        xs = torch.tensor([-1.0, -0.5, 0.0, w - 1.0, w - 0.5, float(w)])
        ys = torch.tensor([-1.0, -0.5, 0.0, h - 1.0, h - 0.5, float(h)])
        r, c = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        pos = torch.stack([xs[c % 6], ys[(r + c // 6) % 6]])                    # every (x, y) pair of the six positions occurs
        flow = (pos - torch.stack([c, r]).to(torch.float32))[None].repeat(n, 1, 1, 1)
        assert torch.equal(flow[0] + torch.stack([c, r]).to(torch.float32), pos)
    elif kind == "far":
        vals = torch.tensor([1e6, -1e6, 3e9, -3e9, 0.5, -0.25, 1.75, -1.0])
        flow = vals[torch.randint(0, len(vals), (n, 2, h, w), generator=g)]
    else:
        raise KeyError(kind)
    if taps == 1:
        frac = torch.rand(n, 2, h, w, generator=_gen("frac:" + name)) * 0.4 + 0.05
        frac = frac + 0.5 * (torch.rand(n, 2, h, w, generator=_gen("half:" + name)) < 0.5)
        flow = torch.floor(flow) + frac
    return flow.to(torch.float32).contiguous()


def clip_inputs(b, d, f, dtype=torch.float32):
    """x (B, D, C, H, W), flows_backward and flows_forward (B, D - 1, 2, H, W), +-4 px sub-pixel"""
    c, h, w = f
    name = clip_name(b, d, f)
    x = case_x(name, dtype, (b, d, c, h, w))
    fb = _uniform_flow(name + ":b", b * (d - 1), h, w, 4.0).view(b, d - 1, 2, h, w)
    ff = _uniform_flow(name + ":f", b * (d - 1), h, w, 4.0).view(b, d - 1, 2, h, w)
    return x, fb, ff


def grid_cotangent(key, shape):
    """small integers in [-2, 2]: every partial sum is exact in fp32 (and in bf16) in any order"""
    return torch.randint(-2, 3, shape, generator=_gen("cot:" + key)).to(torch.float32)


def random_cotangent(key, shape):
    return torch.randn(shape, generator=_gen("rcot:" + key))


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def tap_indices(flow, taps, border=False):
    """per tap: (valid (N, H, W) bool, iy, ix int64) from the planar fp32 flow, as the specification states it"""
    flow = np.asarray(flow, dtype=np.float32)
    n, _, h, w = flow.shape
    with np.errstate(invalid="ignore", over="ignore"):
        px = np.arange(w, dtype=np.float32)[None, None, :] + flow[:, 0]              # one fp32 add
        py = np.arange(h, dtype=np.float32)[None, :, None] + flow[:, 1]
        assert px.dtype == np.float32 and py.dtype == np.float32
        if taps == 4:
            pairs = [(np.floor(px), np.floor(py)), (np.floor(px), np.ceil(py)), (np.ceil(px), np.floor(py)), (np.ceil(px), np.ceil(py))]
        elif taps == 1:
            pairs = [(np.rint(px), np.rint(py))]                                      # ties to even
        else:
            raise ValueError(taps)
        out = []
        for tx, ty in pairs:
            if border:
                tx = np.fmin(np.fmax(tx, np.float32(0)), np.float32(w - 1))
                ty = np.fmin(np.fmax(ty, np.float32(0)), np.float32(h - 1))
            valid = (tx >= 0) & (tx <= np.float32(w - 1)) & (ty >= 0) & (ty <= np.float32(h - 1))       # on the float; NaN fails
            ix = np.where(valid, tx, 0).astype(np.int64)
            iy = np.where(valid, ty, 0).astype(np.int64)
            out.append((valid, iy, ix))
    return out


def warp(x, flow, taps, border=False):
    """x (N, C, H, W) torch (any float dtype), flow planar -> (N, taps C, H, W) of x's dtype: a gather, exact"""
    xn = x.to(torch.float32).numpy() if x.dtype == torch.bfloat16 else x.numpy()
    n = xn.shape[0]
    nn = np.arange(n)[:, None, None]
    outs = []
    for valid, iy, ix in tap_indices(flow, taps, border):
        got = xn[nn, :, iy, ix]                                                       # (N, H, W, C)
        outs.append(np.where(valid[..., None], got, 0).transpose(0, 3, 1, 2))
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(outs, 1))).to(x.dtype)


def warp_grad(gout, flow, taps, border=False, stats=False):
    """fp64 gradient w.r.t. x of <warp(x), gout>: every in-frame tap adds its cotangent to its source pixel.  With stats: also the
    number of contributions per source value and the sum of their magnitudes."""
    g = gout.to(torch.float64).numpy()
    n, tc, h, w = g.shape
    c = tc // taps
    gx = np.zeros((n, h, w, c))
    cnt = np.zeros((n, h, w, c))
    mag = np.zeros((n, h, w, c))
    nn = np.broadcast_to(np.arange(n)[:, None, None], (n, h, w))
    for k, (valid, iy, ix) in enumerate(tap_indices(flow, taps, border)):
        gk = g[:, k * c:(k + 1) * c].transpose(0, 2, 3, 1)[valid]
        idx = (nn[valid], iy[valid], ix[valid])
        np.add.at(gx, idx, gk)
        np.add.at(cnt, idx, 1.0)
        np.add.at(mag, idx, np.abs(gk))
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))
    return (to(gx), to(cnt), to(mag)) if stats else to(gx)


def aligned_input(x, fb, ff):
    """cat([x, x_backward, x_forward], 2) of vrt.py:149-150 from the pair oracle"""
    b, d, c, h, w = x.shape
    zero = torch.zeros(b, 4 * c, h, w, dtype=x.dtype)
    xb = [warp(x[:, i], fb[:, i - 1], 4) for i in range(1, d)] + [zero]
    xf = [zero] + [warp(x[:, i], ff[:, i], 4) for i in range(0, d - 1)]
    return torch.cat([x, torch.stack(xb, 1), torch.stack(xf, 1)], 2)


def aligned_input_grad(gout, fb, ff, stats=False):
    """fp64 gradient w.r.t. x: the identity part plus both scatters (and, with stats, contribution counts and magnitude sums)"""
    b, d, c9, h, w = gout.shape
    c = c9 // 9
    g = gout.to(torch.float64)
    parts = [g[:, :, :c].clone(), torch.ones(b, d, c, h, w, dtype=torch.float64), g[:, :, :c].abs().clone()]
    for i in range(1, d):
        for p, q in zip(parts, warp_grad(g[:, i - 1, c:5 * c], fb[:, i - 1], 4, stats=True)):
            p[:, i] += q
    for i in range(0, d - 1):
        for p, q in zip(parts, warp_grad(g[:, i + 1, 5 * c:], ff[:, i], 4, stats=True)):
            p[:, i] += q
    return tuple(parts) if stats else parts[0]


def to_channels_last(flow):
    """planar (N, 2, H, W) -> the (N, H, W, 2) view the reference's callers pass (``flow.permute(0, 2, 3, 1)``): non-contiguous"""
    return flow.permute(0, 2, 3, 1)
