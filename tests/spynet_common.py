"""Shared by test_spynet_host.py and test_spynet_gpu.py: SPyNet's launches (the five 7x7 layers, their data and weight gradients, and the
ten planar launches around them: resize + normalise, 2x2 average pool, the per-level warp + concat + flow upsample, the flow resize,
the last layer's ReLU mask, the fp32 add, and four adjoints) restated in fp64, the elementwise bound of tests/hr_tail_common.py and
tests/trunk_common.py, and the driver of the ``vsr_debug_spy_*`` hooks (csrc/spynet_hooks.hip).  Case, Guarded, Planar, PmOutput,
pm_input, draw, draw_grid, draw_aux, mask_factor, measure_against / check_against and same_bits are used as they are.

* ``reference(case)``: the 7x7 operations from ``F.conv2d``; the planar ones from index arithmetic on the kernels' own formulas evaluated
  in fp64 (test_spynet_host.py pins them at 1e-10 to torch fp64 autograd on ``F.interpolate``, ``F.grid_sample`` / the oracle's
  ``flow_warp``, ``F.avg_pool2d`` and the ConvReLU stack).  Each output comes with ``A = sum |a_k b_k|`` from the same code on the
  operands' magnitudes and its term count K (``terms``).  For the scattering adjoints K and A come from the same scatter applied to
  ones and to magnitudes.
* the arithmetic bound is the project's (profiles/trunk_parity.md): a bf16 output |err| <= u |r| + 2 K 2^-24 A, an fp32 output
  |err| <= 2 K 2^-24 A, no element exempt; a bias, ``pres`` and a pre-filled gradient each count as one term; what a launch must leave
  alone, or only copies, has the bound 0.
* the coordinate term.  resize_norm, flow_out, spynet_prepare and their adjoints compute a sample coordinate in fp32.  A coordinate that
  is off by delta moves a bilinear value by at most delta (|dv/dx| + |dv/dy|) -- the interpolant is continuous, so this also holds when
  ``floor`` lands in the neighbouring cell; the partials are taken from the fp64 taps as the largest slope of the sample's cell and its
  two neighbours along that axis.  For an adjoint, the weight of a tap moves by at most delta times the other axis' weight.  delta is
  the count of roundings in the kernel's formula, each 2^-24 of the magnitude it rounds:
    src_index, align_corners=False:  s = (d + 0.5) * scale - 0.5 -- the quotient ``scale``, the product and the difference: 3 roundings of
      at most (d + 0.5) scale each (d + 0.5 is exact; the clamp at 0 and ``s - i0`` are exact).     delta = 3 2^-24 (d + 0.5) scale
    src_index, align_corners=True:   s = d * scale -- the quotient and the product.                   delta = 2 2^-24 d scale
    warp_coord: g = 2 (base + flow) / d - 1, p = (g + 1) 0.5 (dim - 1) with m = |base + flow| -- the sum, the quotient, ``g + 1`` and the
      last product round a value of magnitude m (in pixels; the factors 2 and 0.5 are exact), ``- 1`` one of |m - d/2|: 5 roundings.
                                                                                                        delta = 2^-24 (5 m + d/2)
      plus, in spynet_prepare, the error of the fp32 ``flow_up`` the coordinate is made of (its own bound, both terms); the clamp to
      [0, dim - 1] is 1-Lipschitz.  dim = 1: the coordinate is (g + 1) 0.5 * 0 = 0 in any precision, and every slope is 0.
* the flow gradient of spynet_prepare_bwd is discontinuous where a sample coordinate is an integer and at the clip limits 0 and dim - 1:
  ``flow_up`` of those cases is drawn so that every fp64 coordinate has a fractional part in [1/8, 7/8] and is inside the limits by at
  least 1/8 or outside by at least 1/8, one eighth of the samples (at least one) outside on each side of each axis.  ``_prepare_bwd`` asserts it.
* two input families for the three 7x7 hooks, as in the trunk: ``rand`` and ``grid`` ({-1, -1/2, 0, 1/2, 1}, ReLU or no activation;
  A < 2^22 asserted: an fp32 evaluation in any order is exact, an fp32 output has to equal the fp64 reference and a bf16 output its
  round-to-nearest-even, bit for bit).  For the deep shape the grid reference is an fp32 CPU ``F.conv2d``: every partial sum is exact in
  any order, so it IS the fp64 value, at a third of the time (``_values`` says where).
* masks: the data gradient's ``aux`` from ``draw_aux``; spynet_dres's planar ``res`` carries +0, -0, +2^-133 and -2^-133 on its first and
  last column.  ``> 0`` passes (the positive subnormal too), everything else is zeroed to +0.
* ``emulate(case, mut)``: fp32 -- the 7x7 operations with the reduction axes reversed, the planar ones with every coordinate computed in
  fp32 by the kernel's formula -- rounded to bf16 where the bf16 build stores; ``mut`` is one of MUTATIONS.
* ``run_hip(case, dev)``: one hook call; inputs with NaN padding pixels in NaN-banded buffers, outputs between sentinel bands, the status
  checked before anything reads an output."""
import functools

import torch
import torch.nn.functional as F

import hr_tail_common as T
from hr_tail_common import Case, EPS, SENTINEL, SUBNORMAL, U, bf16_round, draw, draw_aux, mask_factor, same_bits, sid  # noqa: F401
from trunk_common import case, draw_grid  # noqa: F401

CI, CO = (8, 32, 64, 32, 16), (32, 64, 32, 16, 2)
CIP, CD, DK = (16, 32, 64, 32, 16), (32, 64, 32, 16, 0), (32, 64, 32, 16, 16)

COARSE = [(1, 1, 1), (1, 2, 2), (1, 4, 4), (2, 8, 16)]                          # the engine's own coarse levels at hu = wu = 32 (and 64)
RAGGED = [(1, 8, 32), (2, 13, 37), (1, 3, 66), (1, 9, 31), (1, 17, 100)]        # the tail's list
SMALL = COARSE + RAGGED
BIG = (3, 80, 352)                   # 330 tiles on 256 workgroups: a QTileIter crosses an image boundary
DEEP = (4, 200, 330)                 # 1100 tiles: more than four per workgroup; grid family, bf16, forward and masked data gradient
WG_MANY = (3, 72, 200)               # the weight gradient's several-tiles case; grid family, accumulate
CONV_HOOKS = ("conv", "dgrad", "wgrad")
PLANAR_OPS = ("resize_norm", "resize_norm_bwd", "avgpool2", "avgpool2_bwd", "flow_out", "flow_out_bwd", "add")
LEVEL0 = [(1, 1), (3, 5)]
LEVELS = [(2, 2), (2, 6), (6, 2), (4, 4), (8, 16), (26, 74), (64, 96)]
PAIRS = [dict(pair_mode=0, n=1, t=2), dict(pair_mode=0, n=2, t=3), dict(pair_mode=1, P=1), dict(pair_mode=1, P=3)]
RESIZES = [((1, 1), (32, 32)), ((13, 37), (32, 64)), ((31, 33), (32, 64)), ((32, 64), (32, 64)), ((40, 72), (64, 96))]
MUTATIONS = ("tap_mirrored", "halo_cut_to_2", "drop_last_column", "eighth_tap_leaks", "passes_swapped", "pres_dropped", "relu_on_last_layer",
             "mask_ge", "accumulate_overwrites", "clip_mask_ignored", "flow_up_2x_missing", "align_corners_false", "pair_swapped", "uv_scales_swapped")


def npairs(c: Case):
    return c.o("P") if c.o("pair_mode", 1) else 2 * c.o("n") * (c.o("t") - 1)


def nframes(c: Case):
    return 2 * c.o("P") if c.o("pair_mode", 1) else c.o("n") * c.o("t")


# --------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def _specials_on_border(t, seed):
    """+0, -0, +-2^-133 on the first and the last column of a planar tensor (P, 2, h, w) and sprinkled over ~3 % of the rest."""
    g = torch.Generator().manual_seed(int(seed))
    special = torch.tensor([0.0, -0.0, SUBNORMAL, -SUBNORMAL])
    kind = torch.randint(0, 4, t.shape, generator=g)
    t = torch.where(torch.rand(t.shape, generator=g) < 0.03, special[kind], t)
    for col in (0, t.shape[-1] - 1):
        t[..., col] = special[(torch.arange(t.shape[-2]).view(-1) + torch.arange(t.shape[0] * t.shape[1]).view(-1, 1)).view(t.shape[0], t.shape[1], -1) % 4]
    return t


def _conditioned_flow(seed, P, h, w):
    """flow_up (P, 2, h, w) whose sample coordinates base + flow are integer + fraction, fraction in [3/16, 13/16]; per axis one eighth of
    the samples in [-2, 0), one eighth in [dim - 1, dim + 1), the rest inside [0, dim - 1) (dim = 1: there is no inside)."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for base, dim in ((torch.arange(w).view(1, 1, w), w), (torch.arange(h).view(1, h, 1), h)):
        where = (torch.randperm(P * h * w, generator=g).view(P, h, w).float() + 0.5) / (P * h * w)      # a fixed share on each side: numel // 8, at least one
        frac = 3 / 16 + torch.rand(P, h, w, generator=g) * 10 / 16
        inside = torch.randint(0, max(dim - 1, 1), (P, h, w), generator=g)
        below = torch.randint(-2, 0, (P, h, w), generator=g)
        above = torch.randint(dim - 1, dim + 1, (P, h, w), generator=g)
        nb = max(P * h * w // 8, 1) / (P * h * w)
        lo, hi = (0.5, 0.5) if dim == 1 else (nb, 2 * nb)
        cell = torch.where(where < lo, below, torch.where(where < hi, above, inside))
        out.append((cell + frac - base).float())
    return torch.stack(out, 1)


@functools.lru_cache(maxsize=4)
def make_inputs(hook, shape, key):
    """CPU fp32 tensors of one (hook, shape); key: the options that change the operands."""
    o = dict(key)
    b, h, w = shape
    hooks = CONV_HOOKS + PLANAR_OPS + ("prepare", "prepare_bwd", "dres")
    s = 11000 + 131 * h + 17 * w + b + 1000 * hooks.index(hook) + 7 * o.get("j", 0)
    if hook in CONV_HOOKS:
        j, grid = o["j"], o.get("family", "rand") == "grid"
        d = draw_grid if grid else draw
        fl = draw_grid if grid else _randn                  # fp32 operands: bias, pres, pre-filled gradients
        if hook == "conv":
            return dict(x=d(s, b, CI[j], h, w), w=d(s + 1, CO[j], CI[j], 7, 7), bias=fl(s + 2, CO[j]), pres=fl(s + 3, b, 2, h, w))
        if hook == "dgrad":
            aux = draw_aux(s + 2, b, h, w, CI[j])
            return dict(dy=d(s, b, CO[j], h, w), w=d(s + 1, CO[j], CI[j], 7, 7), aux=aux)
        return dict(x=d(s, b, CI[j], h, w), dy=d(s + 1, b, CO[j], h, w), gw0=fl(s + 2, CO[j], CI[j], 7, 7), gb0=fl(s + 3, CO[j]))
    if hook in PLANAR_OPS:
        hu, wu = o.get("hu", h), o.get("wu", w)
        ms = dict(mean=torch.tensor([0.485, 0.456, 0.406]), std=torch.tensor([0.229, 0.224, 0.225]))
        if hook == "resize_norm":
            return dict(x=torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(s)), **ms)
        if hook == "resize_norm_bwd":
            return dict(d=_randn(s, b, 3, hu, wu), out0=_randn(s + 1, b, 3, h, w), **ms)
        if hook == "avgpool2":
            return dict(x=_randn(s, b, h, w))
        if hook == "avgpool2_bwd":
            return dict(d=_randn(s, b, h // 2, w // 2), out0=_randn(s + 1, b, h, w))
        if hook == "flow_out":
            return dict(x=_randn(s, b, 2, hu, wu) * 4)
        if hook == "flow_out_bwd":
            return dict(d=_randn(s, b, 2, h, w), out0=_randn(s + 1, b, 2, hu, wu))
        return dict(a=_randn(s, b, h, w), b=_randn(s + 1, b, h, w))
    P = b
    Fr = 2 * P if o.get("pair_mode", 1) else o["n"] * o["t"]
    if hook == "dres":
        return dict(d=_randn(s, P, 2, h, w), res=_specials_on_border(_randn(s + 1, P, 2, h, w), s + 2))
    if hook == "prepare":
        return dict(frames=_randn(s, Fr, 3, h, w), flow_prev=_randn(s + 1, P, 2, max(h // 2, 1), max(w // 2, 1)) * 1.5)
    if hook == "prepare_bwd":
        return dict(frames=_randn(s, Fr, 3, h, w), flow_up=_conditioned_flow(s + 1, P, h, w), dx16=draw(s + 2, P, 8, h, w), dflow_l=_randn(s + 3, P, 2, h, w),
                    dprev0=_randn(s + 4, P, 2, max(h // 2, 1), max(w // 2, 1)), dframes0=_randn(s + 5, Fr, 3, h, w))
    raise KeyError(hook)


_OPERAND_OPTS = ("j", "family", "hu", "wu", "pair_mode", "n", "t", "P")


def inputs_of(c: Case):
    return make_inputs(c.hook, c.shape, tuple((k, v) for k, v in c.opts if k in _OPERAND_OPTS))


# --------------------------------------------------------------------------------------------------------------------
# the 7x7 operations, in the dtype of their operands.  rev: the reduction axes reversed; mut: one of MUTATIONS
# --------------------------------------------------------------------------------------------------------------------
def _conv7(x, w, mut=None, rev=False):
    """'same' 7x7 convolution of x (N, Ci, H, W) with w (Co, Ci, 7, 7)."""
    if mut == "tap_mirrored":                              # taps (3, 2) and (3, 4) change places
        w = w.clone()
        w[:, :, 3, 2], w[:, :, 3, 4] = w[:, :, 3, 4].clone(), w[:, :, 3, 2].clone()
    if mut == "halo_cut_to_2":                             # the outermost ring of the halo reads as zero where it lies inside the image too
        w = w.clone()
        w[:, :, 0], w[:, :, 6], w[:, :, :, 0], w[:, :, :, 6] = 0, 0, 0, 0
    if mut == "passes_swapped" and x.shape[1] == 64:       # the second 32-channel pass meets the first pass' weights
        x = torch.cat([x[:, 32:], x[:, :32]], 1)
    if rev:
        x, w = x.flip(1), w.flip(1)
    y = F.conv2d(x, w, padding=3)
    if mut == "eighth_tap_leaks" and x.shape[1] <= 16:     # tap pairs: the eighth tap of a row has a weight after all, and reads the pixel at + 4
        y = y + F.conv2d(F.pad(x, (0, 4, 3, 3))[..., 4:], 0.5 * w[..., 6:7])
    return y


def _dgrad_w(w):
    return w.transpose(0, 1).flip(2, 3)


def _wgrad7(x, dy, mut=None, rev=False):
    """gw[co][ci][ky][kx] = sum_p dy[co][p] x[ci][p + (ky - 3, kx - 3)], gb[co] = sum_p dy[co][p]."""
    if mut == "drop_last_column":
        dy = dy.clone()
        dy[..., -1] = 0
    if rev:
        x, dy = x.flip(0, 3), dy.flip(0, 3)
    gw = F.conv2d(F.pad(x, (3, 3, 3, 3)).transpose(0, 1), dy.transpose(0, 1)).transpose(0, 1)
    if rev:
        gw = gw.flip(3)
    if mut == "tap_mirrored":
        gw = gw.clone()
        gw[:, :, 3, 2], gw[:, :, 3, 4] = gw[:, :, 3, 4].clone(), gw[:, :, 3, 2].clone()
    if mut == "passes_swapped" and x.shape[1] == 64:       # the two 32-channel halves land in each other's place
        gw = torch.cat([gw[:, 32:], gw[:, :32]], 1)
    return gw, dy.sum(dim=(0, 2, 3))


def _ops7(c: Case, t, mut=None, rev=False):
    j = c.o("j")
    if c.hook == "conv":
        y = _conv7(t["x"], t["w"], mut, rev) + t["bias"].view(1, -1, 1, 1)
        if c.o("act", 1) or (mut == "relu_on_last_layer" and j == 4):
            y = torch.relu(y)
        if c.o("pres", 0) and mut != "pres_dropped":
            y = y + t["pres"]
        return dict(y=y)
    if c.hook == "dgrad":
        dx = _conv7(t["dy"], _dgrad_w(t["w"]), mut, rev)
        if c.o("aux", 0):
            dx = dx * mask_factor(t["aux"], 0.0, mut)
        return dict(dx=dx)
    gw, gb = _wgrad7(t["x"], t["dy"], mut, rev)
    keep = c.o("accumulate", 0) and mut != "accumulate_overwrites"
    out = dict(gw=(t["gw0"] + gw) if keep else gw)
    if c.o("gb", True):
        out["gb"] = (t["gb0"] + gb) if keep else gb
    return out


# --------------------------------------------------------------------------------------------------------------------
# the planar operations: the kernels' formulas, every coordinate in the dtype of the operands
# --------------------------------------------------------------------------------------------------------------------
def _src_index(dsize, in_size, num, den, align, dt):
    """src_index for d = 0 .. dsize - 1 at scale num / den: (i0, i1, l1, delta); delta: the docstring's count, on the values at hand."""
    d = torch.arange(dsize, dtype=dt)
    scale = (torch.tensor(float(num), dtype=dt) / torch.tensor(float(den), dtype=dt)) if den else torch.zeros((), dtype=dt)
    if align:
        s = d * scale
        delta = 2 * EPS * s
    else:
        s = ((d + 0.5) * scale - 0.5).clamp_min(0)
        delta = 3 * EPS * (d + 0.5) * scale
    i0 = s.floor().long().clamp_max(in_size - 1)
    i1 = i0 + (i0 < in_size - 1).long()
    return i0, i1, s - i0.to(dt), delta


def _matrix(idx, in_size, dt, kind="w"):
    """(dsize, in_size): row d holds 1 - l1 at i0 and l1 at i1 (w), 1 at both (count), or delta at i0 - 1, i0, i1 and i1 + 1, clamped (delta:
    a coordinate that is off by delta moves at most delta of the weight between neighbouring taps, the next cell's included)."""
    i0, i1, l1, delta = idx
    m = torch.zeros(len(i0), in_size, dtype=dt)
    rows = torch.arange(len(i0))
    if kind == "delta":
        for i in ((i0 - 1).clamp_min(0), i0, i1, (i1 + 1).clamp_max(in_size - 1)):
            m.index_put_((rows, i), delta.to(dt), accumulate=True)
        return m
    a, b = (1 - l1, l1) if kind == "w" else (torch.ones_like(l1), torch.ones_like(l1))
    m.index_put_((rows, i0), a.to(dt), accumulate=True)
    m.index_put_((rows, i1), b.to(dt), accumulate=True)
    return m


def _resize(p, yi, xi):
    """Bilinear resize of p (..., H, W) by the index sets of _src_index."""
    return _matrix(yi, p.shape[-2], p.dtype) @ p @ _matrix(xi, p.shape[-1], p.dtype).transpose(0, 1)


def _resize_t(d, yi, xi, hin, win, kind_y="w", kind_x="w"):
    """The adjoint: (..., Ho, Wo) -> (..., hin, win)."""
    return _matrix(yi, hin, d.dtype, kind_y).transpose(0, 1) @ d @ _matrix(xi, win, d.dtype, kind_x)


def _slopes(p, yi, xi):
    """(|dv/dy|, |dv/dx|) of the resize at every output element: the largest over the sample's cell and its two neighbours."""
    H, W = p.shape[-2:]
    My, Mx = _matrix(yi, H, p.dtype), _matrix(xi, W, p.dtype)
    best = []
    for axis, (i0, size) in enumerate(((yi[0], H), (xi[0], W))):
        top = None
        for s in (-1, 0, 1):
            a = (i0 + s).clamp(0, size - 1)
            b = (a + 1).clamp_max(size - 1)
            D = torch.zeros(len(i0), size, dtype=p.dtype)
            D[torch.arange(len(i0)), b] += 1
            D[torch.arange(len(i0)), a] -= 1
            v = (D @ p @ Mx.transpose(0, 1)) if axis == 0 else (My @ p @ D.transpose(0, 1))
            top = v.abs() if top is None else torch.maximum(top, v.abs())
        best.append(top)
    return best


def _pairs(c: Case, mut=None):
    """(fref, fsup): the frame of each pair (spynet_prepare_kernel)."""
    P = npairs(c)
    if c.o("pair_mode", 1):
        return list(range(P)), list(range(P, 2 * P))
    t, half = c.o("t"), P // 2
    fref, fsup = [], []
    for p in range(P):
        q = p if p < half else p - half
        b, i = q // (t - 1), q % (t - 1)
        first = p < half or mut == "pair_swapped"
        fref.append(b * t + i if first else b * t + i + 1)
        fsup.append(b * t + i + 1 if first else b * t + i)
    return fref, fsup


def _warp_coord(base, flow, dim):
    d = float(max(dim - 1, 1))
    g = 2.0 * (base + flow) / d - 1.0
    return (g + 1.0) * 0.5 * float(dim - 1)


def _warp_delta(base, flow, dim):
    m = (base + flow).abs()
    return EPS * (5 * m + max(dim - 1, 1) / 2) if dim > 1 else torch.zeros_like(m)


def _warp_setup(fu, h, w):
    """Clamped coordinates, corner indices and weights of the border-mode warp at flow fu (P, 2, h, w)."""
    dt = fu.dtype
    xs, ys = torch.arange(w, dtype=dt).view(1, 1, w), torch.arange(h, dtype=dt).view(1, h, 1)
    ux, uy = _warp_coord(xs, fu[:, 0], w), _warp_coord(ys, fu[:, 1], h)
    px, py = ux.clamp(0, w - 1), uy.clamp(0, h - 1)
    x0, y0 = px.floor(), py.floor()
    wx1, wy1 = px - x0, py - y0
    x0, y0 = x0.long(), y0.long()
    return dict(ux=ux, uy=uy, x0=x0, y0=y0, x1=(x0 + 1).clamp_max(w - 1), y1=(y0 + 1).clamp_max(h - 1), wx1=wx1, wy1=wy1, wx0=1 - wx1, wy0=1 - wy1,
                dx=_warp_delta(xs, fu[:, 0], w), dy=_warp_delta(ys, fu[:, 1], h))


def _tap(img, yy, xx):
    """img (P, C, h, w) at per-pixel positions (P, h, w) -> (P, C, h, w)."""
    P, C, h, w = img.shape
    idx = (yy * w + xx).view(P, 1, h * w).expand(P, C, h * w)
    return torch.gather(img.reshape(P, C, h * w), 2, idx).view(P, C, h, w)


def _warp(img, g):
    u = lambda v: v.unsqueeze(1)
    return u(g["wy0"]) * (u(g["wx0"]) * _tap(img, g["y0"], g["x0"]) + u(g["wx1"]) * _tap(img, g["y0"], g["x1"])) + \
        u(g["wy1"]) * (u(g["wx0"]) * _tap(img, g["y1"], g["x0"]) + u(g["wx1"]) * _tap(img, g["y1"], g["x1"]))


def _warp_slopes(img, g):
    """(|dv/dx|, |dv/dy|) of the warp's value (P, C, h, w): the largest over the sample's cell and its neighbours along the axis."""
    h, w = img.shape[-2:]
    u = lambda v: v.unsqueeze(1)
    bx = by = None
    for s in (-1, 0, 1):
        a = (g["x0"] + s).clamp(0, w - 1)
        b = (a + 1).clamp_max(w - 1)
        v = (u(g["wy0"]) * (_tap(img, g["y0"], b) - _tap(img, g["y0"], a)) + u(g["wy1"]) * (_tap(img, g["y1"], b) - _tap(img, g["y1"], a))).abs()
        bx = v if bx is None else torch.maximum(bx, v)
        a = (g["y0"] + s).clamp(0, h - 1)
        b = (a + 1).clamp_max(h - 1)
        v = (u(g["wx0"]) * (_tap(img, b, g["x0"]) - _tap(img, a, g["x0"])) + u(g["wx1"]) * (_tap(img, b, g["x1"]) - _tap(img, a, g["x1"]))).abs()
        by = v if by is None else torch.maximum(by, v)
    return bx, by


def _scatter(out, frame_of_pair, yy, xx, val):
    """out (F, 3, h, w)[frame of pair p, :, yy[p], xx[p]] += val (P, 3, h, w)."""
    Fr, C, h, w = out.shape
    flat = out.view(Fr, C, h * w)
    idx = yy * w + xx
    for p, f in enumerate(frame_of_pair):
        flat[f].scatter_add_(1, idx[p].view(1, -1).expand(C, -1), val[p].reshape(C, -1))
    return out


def _scatter_warp(out, frame_of_pair, g, val, wsel):
    """out += the warp's adjoint of val (P, 3, h, w); wsel(ky, kx) gives the (P, h, w) factor of tap (ky, kx)."""
    for ky in (0, 1):
        for kx in (0, 1):
            _scatter(out, frame_of_pair, g["y1" if ky else "y0"], g["x1" if kx else "x0"], val * wsel(ky, kx).unsqueeze(1))
    return out


def _scatter_warp_delta(out, frame_of_pair, g, mag):
    """The coordinate term of the warp's adjoint: a coordinate off by delta moves at most delta x (the other axis' weight) x |value| between
    neighbouring taps along its axis, the next cell's included (a sample on a cell boundary, as every sample of level 0 is)."""
    h, w = out.shape[-2:]
    for k in (0, 1):
        for o in (-1, 0, 1, 2):
            _scatter(out, frame_of_pair, g["y1" if k else "y0"], (g["x0"] + o).clamp(0, w - 1), mag * (g["dx"] * g["wy1" if k else "wy0"]).unsqueeze(1))
            _scatter(out, frame_of_pair, (g["y0"] + o).clamp(0, h - 1), g["x1" if k else "x0"], mag * (g["dy"] * g["wx1" if k else "wx0"]).unsqueeze(1))
    return out


def _up_index(c: Case, dt, mut=None):
    h, w = c.shape[1:]
    hp, wp = h // 2, w // 2
    if mut == "align_corners_false":
        return _src_index(h, hp, hp, h, False, dt), _src_index(w, wp, wp, w, False, dt)
    return _src_index(h, hp, hp - 1 if hp > 1 else 0, h - 1, True, dt), _src_index(w, wp, wp - 1 if wp > 1 else 0, w - 1, True, dt)


def _prepare(c: Case, t, mut=None, want_bound=False):
    """flow_up (P, 2, h, w) and x16 (P, 16, h, w) = [ref | warp(supp, flow_up, border) | flow_up | 0 x 8].  want_bound: also (A, coordinate
    term) per output, from the same taps."""
    P, h, w = c.shape
    fr = t["frames"]
    dt = fr.dtype
    fref, fsup = _pairs(c, mut)
    zero = torch.zeros(P, 2, h, w, dtype=dt)
    a_fu = c_fu = zero
    if c.o("level0", 0):
        fu = zero
    else:
        yi, xi = _up_index(c, dt, mut)
        fu = _resize(t["flow_prev"], yi, xi) * (1.0 if mut == "flow_up_2x_missing" else 2.0)
        if want_bound:
            sy, sx = _slopes(t["flow_prev"], yi, xi)
            a_fu = 2 * _resize(t["flow_prev"].abs(), yi, xi)
            c_fu = 2 * (sy * yi[3].view(-1, 1) + sx * xi[3].view(1, -1))
    g = _warp_setup(fu, h, w)
    sup = fr[fsup]
    x16 = torch.cat([fr[fref], _warp(sup, g), fu, torch.zeros(P, 8, h, w, dtype=dt)], 1)
    out = dict(flow_up=fu, x16=x16)
    if not want_bound:
        return out
    e_fu = 2 * 4 * EPS * a_fu + c_fu                       # what the fp32 flow_up may be off by: part of the warp's coordinate error
    bx, by = _warp_slopes(sup, g)
    c_warp = (g["dx"] + e_fu[:, 0]).unsqueeze(1) * bx + (g["dy"] + e_fu[:, 1]).unsqueeze(1) * by
    z3, z8 = torch.zeros(P, 3, h, w, dtype=dt), torch.zeros(P, 8, h, w, dtype=dt)
    A = dict(flow_up=a_fu, x16=torch.cat([z3, _warp(sup.abs(), g), a_fu, z8], 1))       # the reference frame and the zeros are copies: bound 0
    Cd = dict(flow_up=c_fu, x16=torch.cat([z3, c_warp, c_fu, z8], 1))
    return out, A, Cd


def _prepare_bwd(c: Case, t, mut=None, want_bound=False):
    """dflow_prev (P, 2, h/2, w/2) and dframes (F, 3, h, w), each ADDED to its pre-filled value, from dx16 (P, 8, h, w), the level's flow
    gradient dflow_l, the frames and flow_up."""
    P, h, w = c.shape
    fr, d = t["frames"], t["dx16"]
    dt = fr.dtype
    fref, fsup = _pairs(c, mut)
    level0 = bool(c.o("level0", 0))
    fu = torch.zeros(P, 2, h, w, dtype=dt) if level0 else t["flow_up"]
    g = _warp_setup(fu, h, w)
    if want_bound and not level0:                          # (the reference:) the condition on the inputs that makes the flow gradient continuous around them
        for u_, dim in ((g["ux"], w), (g["uy"], h)):
            if dim > 1:
                frac = u_ - u_.floor()
                assert bool(((frac >= 0.125) & (frac <= 0.875)).all()), c.name
                assert bool((((u_ >= 0.125) & (u_ <= dim - 1 - 0.125)) | (u_ <= -0.125) | (u_ >= dim - 1 + 0.125)).all()), c.name
                assert int((u_ < 0).sum()) == int((u_ > dim - 1).sum()) == max(u_.numel() // 8, 1), c.name
    sup = fr[fsup]
    u = lambda v: v.unsqueeze(1)
    v00, v01, v10, v11 = _tap(sup, g["y0"], g["x0"]), _tap(sup, g["y0"], g["x1"]), _tap(sup, g["y1"], g["x0"]), _tap(sup, g["y1"], g["x1"])
    out, A, Cd, K = {}, {}, {}, {}
    if c.o("dframes", 1):
        df = t["dframes0"].clone()
        for p, f in enumerate(fref):
            df[f] += d[p, 0:3]
        wsel = lambda ky, kx: g["wy1" if ky else "wy0"] * g["wx1" if kx else "wx0"]
        out["dframes"] = _scatter_warp(df, fsup, g, d[:, 3:6], wsel)
        if want_bound:
            a = t["dframes0"].abs()
            k = torch.ones_like(a)
            for p, f in enumerate(fref):
                a[f] += d[p, 0:3].abs()
                k[f] += 1
            A["dframes"] = _scatter_warp(a, fsup, g, d[:, 3:6].abs(), wsel)
            K["dframes"] = _scatter_warp(k, fsup, g, torch.ones_like(d[:, 3:6]), lambda ky, kx: torch.ones_like(g["wx0"])) + 3
            Cd["dframes"] = _scatter_warp_delta(torch.zeros_like(a), fsup, g, d[:, 3:6].abs())
    if level0:
        return (out, A, Cd, K) if want_bound else out
    d3 = d[:, 3:6]
    mx = ((g["ux"] > 0) & (g["ux"] < w - 1)).to(dt) if mut != "clip_mask_ignored" else torch.ones_like(g["ux"])
    my = ((g["uy"] > 0) & (g["uy"] < h - 1)).to(dt) if mut != "clip_mask_ignored" else torch.ones_like(g["uy"])
    gx = (d3 * (u(g["wy0"]) * (v01 - v00) + u(g["wy1"]) * (v11 - v10))).sum(1) * mx
    gy = (d3 * (u(g["wx0"]) * (v10 - v00) + u(g["wx1"]) * (v11 - v01))).sum(1) * my
    gg = torch.stack([d[:, 6] + gx, d[:, 7] + gy], 1) + t["dflow_l"]
    yi, xi = _up_index(c, dt, mut)
    hp, wp = h // 2, w // 2
    out["dflow_prev"] = t["dprev0"] + (1.0 if mut == "flow_up_2x_missing" else 2.0) * _resize_t(gg, yi, xi, hp, wp)
    if want_bound:
        ax = (d3.abs() * (u(g["wy0"]) * (v01.abs() + v00.abs()) + u(g["wy1"]) * (v11.abs() + v10.abs()))).sum(1) * mx
        ay = (d3.abs() * (u(g["wx0"]) * (v10.abs() + v00.abs()) + u(g["wx1"]) * (v11.abs() + v01.abs()))).sum(1) * my
        ag = torch.stack([d[:, 6].abs() + ax, d[:, 7].abs() + ay], 1) + t["dflow_l"].abs()
        cross = (d3 * ((v11 - v10) - (v01 - v00))).sum(1).abs()      # d gx / d py = d gy / d px
        cg = torch.stack([cross * g["dy"] * mx, cross * g["dx"] * my], 1)
        A["dflow_prev"] = t["dprev0"].abs() + 2 * _resize_t(ag, yi, xi, hp, wp)
        K["dflow_prev"] = _resize_t(torch.ones_like(gg), yi, xi, hp, wp, "count", "count") + 18
        Cd["dflow_prev"] = 2 * (_resize_t(cg, yi, xi, hp, wp) + _resize_t(gg.abs(), yi, xi, hp, wp, "delta", "w") + _resize_t(gg.abs(), yi, xi, hp, wp, "w", "delta"))
    return (out, A, Cd, K) if want_bound else out


def _ops_planar(c: Case, t, mut=None, want_bound=False):
    """dict output -> tensor; want_bound: (out, A, coordinate term, K) -- K a number or, for the scattering adjoints, a tensor."""
    b, h, w = c.shape
    hu, wu = c.o("hu", h), c.o("wu", w)
    dt = next(iter(t.values())).dtype
    zero = lambda v: torch.zeros_like(v)
    if c.hook == "prepare":
        if not want_bound:
            return _prepare(c, t, mut)
        out, A, Cd = _prepare(c, t, None, True)
        return out, A, Cd, dict(flow_up=4, x16=4)
    if c.hook == "prepare_bwd":
        return _prepare_bwd(c, t, mut, want_bound)
    if c.hook == "dres":
        m = mask_factor(t["res"], 0.0, mut) if c.o("res", 1) else torch.ones_like(t["d"])
        y = torch.cat([t["d"] * m, torch.zeros(b, 14, h, w, dtype=dt)], 1)
        return (dict(y=y), dict(y=zero(y)), dict(y=zero(y)), dict(y=1)) if want_bound else dict(y=y)
    if c.hook == "add":
        y = t["a"] + t["b"]
        return (dict(y=y), dict(y=t["a"].abs() + t["b"].abs()), dict(y=zero(y)), dict(y=2)) if want_bound else dict(y=y)
    if c.hook == "avgpool2":
        x = t["x"]
        pool = lambda v: 0.25 * (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2])
        y = pool(x)
        return (dict(y=y), dict(y=pool(x.abs())), dict(y=zero(y)), dict(y=4)) if want_bound else dict(y=y)
    if c.hook == "avgpool2_bwd":
        up = lambda v: 0.25 * v.repeat_interleave(2, -2).repeat_interleave(2, -1)
        y = t["out0"] + up(t["d"])
        return (dict(y=y), dict(y=t["out0"].abs() + up(t["d"].abs())), dict(y=zero(y)), dict(y=2)) if want_bound else dict(y=y)
    if c.hook in ("resize_norm", "resize_norm_bwd"):       # (b, 3, h, w) <-> (b, 3, hu, wu)
        yi, xi = _src_index(hu, h, h, hu, False, dt), _src_index(wu, w, w, wu, False, dt)
        mean, std = t["mean"].view(1, 3, 1, 1), t["std"].view(1, 3, 1, 1)
        if c.hook == "resize_norm":
            y = (_resize(t["x"], yi, xi) - mean) / std
            if not want_bound:
                return dict(y=y)
            sy, sx = _slopes(t["x"], yi, xi)
            return dict(y=y), dict(y=(_resize(t["x"].abs(), yi, xi) + mean.abs()) / std), dict(y=(sy * yi[3].view(-1, 1) + sx * xi[3].view(1, -1)) / std), dict(y=6)
        v = t["d"] / std
        y = t["out0"] + _resize_t(v, yi, xi, h, w)
    else:                                                  # flow_out: (b, 2, hu, wu) <-> (b, 2, h, w)
        yi, xi = _src_index(h, hu, hu, h, False, dt), _src_index(w, wu, wu, w, False, dt)
        fx = torch.tensor(float(w), dtype=dt) / torch.tensor(float(wu), dtype=dt)
        fy = torch.tensor(float(h), dtype=dt) / torch.tensor(float(hu), dtype=dt)
        sc = torch.stack([fy, fx] if mut == "uv_scales_swapped" else [fx, fy]).view(1, 2, 1, 1)
        if c.hook == "flow_out":
            y = _resize(t["x"], yi, xi) * sc
            if not want_bound:
                return dict(y=y)
            sy, sx = _slopes(t["x"], yi, xi)
            return dict(y=y), dict(y=_resize(t["x"].abs(), yi, xi) * sc), dict(y=(sy * yi[3].view(-1, 1) + sx * xi[3].view(1, -1)) * sc), dict(y=6)
        v = t["d"] * sc
        y = t["out0"] + _resize_t(v, yi, xi, hu, wu)
        h, w = hu, wu
    if not want_bound:
        return dict(y=y)
    return (dict(y=y), dict(y=t["out0"].abs() + _resize_t(v.abs(), yi, xi, h, w)),
            dict(y=_resize_t(v.abs(), yi, xi, h, w, "delta", "w") + _resize_t(v.abs(), yi, xi, h, w, "w", "delta")),
            dict(y=_resize_t(torch.ones_like(v), yi, xi, h, w, "count", "count") + 4))


# --------------------------------------------------------------------------------------------------------------------
# terms, bounds, the criterion
# --------------------------------------------------------------------------------------------------------------------
def terms(c: Case):
    """K of the 7x7 hooks: the products summed into one element, plus a bias, ``pres`` and a pre-filled gradient as one term each.  (The
    planar operations return theirs with the values: 4 taps of a bilinear value, + 2 for the further operations of resize_norm --
    mean, std -- and flow_out -- the scale's quotient, its product; an adjoint's scattered contributions + the pre-filled value + 3
    factors of a contribution, spynet_prepare_bwd's flow gradient + the 14 terms of g on top.)"""
    n, h, w = c.shape
    j = c.o("j")
    if c.hook == "conv":
        return dict(y=49 * CI[j] + 2)
    if c.hook == "dgrad":
        return dict(dx=49 * CO[j])
    return dict(gw=n * h * w + 1, gb=n * h * w + 1)


def bf16_outputs(c: Case):
    if c.dtype != "bf16":
        return ()
    if c.hook == "conv":
        return ("y",) if c.o("j") < 4 else ()
    return {"dgrad": ("dx",), "prepare": ("x16",), "dres": ("y",)}.get(c.hook, ())


def _core(c: Case):
    return Case(c.hook, c.shape, "any", c.opts)


def _linear(c: Case):
    o = dict(c.opts)
    if c.hook == "conv":
        o["act"] = 0                                       # ReLU is 1-Lipschitz: the bound of its argument passes
    return Case(c.hook, c.shape, c.dtype, tuple(sorted(o.items())))


@functools.lru_cache(maxsize=8)
def _values(c: Case):
    """(r, A, coordinate term, K) per output name, fp64."""
    t32 = inputs_of(c)
    if c.hook not in CONV_HOOKS:
        return _ops_planar(c, {k: v.double() for k, v in t32.items()}, None, True)
    grid = c.o("family", "rand") == "grid"
    # grid family at the deep shape: fp32 F.conv2d on the CPU IS exact (every product and partial sum a multiple of 1/4 below 2^22, in any
    # order; asserted below on A), so it stands in for the fp64 evaluation at a third of its time
    fast = grid and c.shape == DEEP
    inp = t32 if fast else {k: v.double() for k, v in t32.items()}
    r = _ops7(c, inp)
    mag = {k: v.abs() for k, v in inp.items()}
    if "aux" in inp:
        mag["aux"] = inp["aux"]
    a = _ops7(_linear(c), mag)
    if grid:
        for k, v in a.items():
            assert float(v.max()) < 2.0 ** 22, (c.name, k, float(v.max()))
    r, a = {k: v.double() for k, v in r.items()}, {k: v.double() for k, v in a.items()}
    return r, a, {k: torch.zeros_like(v) for k, v in r.items()}, terms(c)


def reference(c: Case):
    return _values(_core(c))


def bounds(c: Case):
    """name -> (accumulation term, rounding + coordinate terms)."""
    r, a, cd, kk = reference(c)
    grid = c.o("family", "rand") == "grid"
    out = {}
    for k in r:
        acc = torch.zeros_like(a[k]) if grid else 2 * kk[k] * EPS * a[k]
        rnd = (U * r[k].abs() if (k in bf16_outputs(c) and not grid) else torch.zeros_like(acc)) + cd[k]
        out[k] = (acc, rnd)
    return out


def expected(c: Case):
    r = reference(c)[0]
    if c.o("family", "rand") == "grid":
        return {k: (bf16_round(v.float()).double() if k in bf16_outputs(c) else v) for k, v in r.items()}
    return r


def emulate(c: Case, mut=None):
    inp = {k: v.float() for k, v in inputs_of(c).items()}
    out = _ops7(c, inp, mut, True) if c.hook in CONV_HOOKS else _ops_planar(c, inp, mut)
    return {k: (bf16_round(v) if k in bf16_outputs(c) else v) for k, v in out.items()}


def measure(c: Case, got):
    return T.measure_against(c.name, got, expected(c), bounds(c))


def check(c: Case, got, label="hip"):
    """Every element of every output inside its bound (grid family: equal).  One SPY_RATIO line per output: the worst err / bound, the
    worst share of the accumulation term, the worst share of the coordinate term (err beyond the other two terms, over it), and for a
    grid output how many elements equal the reference."""
    want, bnd = expected(c), bounds(c)
    m = T.measure_against(c.name, got, want, bnd)
    cd = reference(c)[2]
    grid = c.o("family", "rand") == "grid"
    for k, (ratio, acc_ratio, idx) in m.items():
        err = (got[k].double() - want[k]).abs()
        over = (err - (bnd[k][0] + bnd[k][1] - cd[k])).clamp_min(0)
        cshare = float(torch.where(over == 0, torch.zeros_like(over), over / cd[k].clamp_min(1e-300)).max())
        eq = f", equal {int((err == 0).sum())} of {err.numel()}" if grid else ""
        print(f"SPY_RATIO {label} {c.name} {k}: worst err/bound {ratio:.3f} at {idx}, accumulation share {acc_ratio:.3f}, coordinate share {cshare:.3f}{eq}")
    bad = {k: v for k, v in m.items() if not v[0] <= 1.0}
    assert not bad, (c.name, T.describe_failures_against(got, want, bnd))
    return m


def passes(c: Case, got):
    return all(v[0] <= 1.0 for v in measure(c, got).values())


def applicable(c: Case, mut):
    """Whether the mutation changes anything the operation of `c` computes AT ITS SHAPE (what is not observable where: MUTATION_NOTES)."""
    n, h, w = c.shape
    j = c.o("j", 0)
    cv, conv = c.hook in ("conv", "dgrad"), c.hook in CONV_HOOKS
    cin = {"conv": CI[j], "dgrad": CO[j], "wgrad": CI[j]}.get(c.hook, 0)
    if mut == "tap_mirrored":
        return conv and w >= 2
    if mut == "halo_cut_to_2":
        return cv and (h >= 4 or w >= 4)
    if mut == "drop_last_column":
        return c.hook == "wgrad"
    if mut == "eighth_tap_leaks":
        return cv and cin <= 16 and w >= 5
    if mut == "passes_swapped":
        return conv and cin == 64
    if mut == "pres_dropped":
        return c.hook == "conv" and bool(c.o("pres", 0))
    if mut == "relu_on_last_layer":
        return c.hook == "conv" and j == 4 and not c.o("act", 1)
    if mut == "mask_ge":
        return (c.hook == "dgrad" and bool(c.o("aux", 0))) or (c.hook == "dres" and bool(c.o("res", 1)))
    if mut == "accumulate_overwrites":
        return c.hook == "wgrad" and bool(c.o("accumulate", 0))
    up = c.hook in ("prepare", "prepare_bwd") and not c.o("level0", 0) and (c.hook == "prepare" or c.o("dprev", 1))
    if mut == "clip_mask_ignored":
        return c.hook == "prepare_bwd" and not c.o("level0", 0) and (h > 1 or w > 1)
    if mut == "flow_up_2x_missing":
        return up
    if mut == "align_corners_false":
        return up and (h > 2 or w > 2)
    if mut == "pair_swapped":
        return c.hook in ("prepare", "prepare_bwd") and not c.o("pair_mode", 1)
    if mut == "uv_scales_swapped":
        return c.hook in ("flow_out", "flow_out_bwd") and c.shape[1] * c.o("wu") != c.shape[2] * c.o("hu")
    raise KeyError(mut)


MUTATION_NOTES = {
    "tap_mirrored": "taps (3, 2) and (3, 4) are one pixel left and right of the centre: an image one pixel wide, (1,1,1), meets neither",
    "halo_cut_to_2": "the ring at distance 3 is met only by an image at least 4 pixels high or wide: not at (1,1,1), (1,2,2)",
    "eighth_tap_leaks": "the pixel at + 4 exists only in an image at least 5 pixels wide: not at (1,1,1), (1,2,2), (1,4,4); 16-channel inputs only",
    "align_corners_false": "from a 1 x 1 flow both conventions give the constant: not at level size (2,2)",
    "clip_mask_ignored": "none: a level > 0 is at least 2 x 2",
    "uv_scales_swapped": "the two factors are equal where h / hu = w / wu: the resizes from (1,1) and (32,64)",
}


# --------------------------------------------------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------------------------------------------------
def run_hip(c: Case, dev):
    """One hook call on the inputs of `c`; dict output name -> fp32 CPU tensor in reference()'s layout.  A HIP error ends the session."""
    return T.fault_guarded(c, _run_hip, dev)


def _pad_channels(t, cp):
    return t if t.shape[1] == cp else torch.cat([t, torch.zeros(t.shape[0], cp - t.shape[1], *t.shape[2:])], 1)


def _run_hip(c: Case, dev):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    inp = inputs_of(c)
    b, h, w = c.shape
    dt = VF.DT_BF16 if c.dtype == "bf16" else VF.DT_F32
    tdt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    st, nan = VF._stream(), float("nan")
    P = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    keep = []

    def held(t):
        keep.append(t)
        return t

    devf = lambda t: held(t.to(dev).contiguous())
    # a layer's padded channels hold zeros, as spynet_prepare and spynet_dres write them (their packed weights are zero as well)
    pm = lambda t, cp: held(T.pm_input(_pad_channels(t, cp), c.dtype, dev))
    planar_in = lambda t: held(T.Planar(t.shape[0], t.shape[1], t.shape[2], t.shape[3], t.shape[1] * t.shape[2] * t.shape[3], dev, nan, t))

    def planar_out(n_, c_, h_, w_, data=None):
        p = T.Planar(n_, c_, h_, w_, c_ * h_ * w_, dev, SENTINEL, data)
        if data is None:
            p.view.fill_(nan)                              # overwritten: whatever was there must not come through
        return held(p)

    if c.hook in CONV_HOOKS:
        j = c.o("j")
        wpack = held(torch.full((49 * 64 * 64,), 1.0, dtype=tdt, device=dev))
        if c.hook == "conv":
            x = pm(inp["x"], CIP[j])
            y = T.PmOutput(b, h, w, c.dtype, dev, c=CD[j]) if j < 4 else planar_out(b, 2, h, w)
            pres = planar_in(inp["pres"]) if c.o("pres", 0) else None
            rc = lib.vsr_debug_spy_conv(dt, j, P(x), P(devf(inp["w"])), P(devf(inp["bias"])), P(wpack), y.ptr() if j < 4 else P(y.view), c.o("act", 1),
                                        P(pres.view) if pres else None, b, h, w, st)
            assert rc == 0, (c.name, rc)
            T._sync()
            return dict(y=y.take())
        if c.hook == "dgrad":
            dy = pm(inp["dy"], DK[j])
            aux = pm(inp["aux"], CIP[j]) if c.o("aux", 0) else None
            dx = T.PmOutput(b, h, w, c.dtype, dev, c=CIP[j])
            rc = lib.vsr_debug_spy_dgrad(dt, j, P(dy), P(devf(inp["w"])), P(wpack), dx.ptr(), P(aux), b, h, w, st)
            assert rc == 0, (c.name, rc)
            T._sync()
            return dict(dx=dx.take()[:, :CI[j]])           # (layer 0: 8 real channels of the 16; spynet_prepare_bwd reads no other)
        x, dy = pm(inp["x"], CIP[j]), pm(inp["dy"], DK[j])
        acc = c.o("accumulate", 0)
        gw, gb = T.Guarded(CO[j] * CI[j] * 49, torch.float32, dev, SENTINEL), T.Guarded(CO[j], torch.float32, dev, SENTINEL)
        gw.body.copy_(inp["gw0"].flatten())
        gb.body.copy_(inp["gb0"])
        if not acc:
            gw.body.fill_(nan)
            if c.o("gb", True):
                gb.body.fill_(nan)
        slab = held(torch.empty(lib.vsr_conv3x3_c64_wgrad_slab_floats(), dtype=torch.float32, device=dev))
        rc = lib.vsr_debug_spy_wgrad(dt, j, P(x), P(dy), P(gw.body), P(gb.body) if c.o("gb", True) else None, acc, P(slab), b, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert gw.bands_untouched() and gb.bands_untouched(), "a weight gradient was written outside its tensor"
        out = dict(gw=gw.body.view(CO[j], CI[j], 7, 7).cpu().clone())
        if c.o("gb", True):
            out["gb"] = gb.body.cpu().clone()
        else:
            assert torch.equal(gb.body.cpu(), inp["gb0"]), "a bias gradient that was not asked for was written"
        return out
    if c.hook == "prepare":
        Pn, lv0 = b, c.o("level0", 0)
        fr = planar_in(inp["frames"])
        fp = None if lv0 else planar_in(inp["flow_prev"])
        fu, x16 = planar_out(Pn, 2, h, w), T.PmOutput(Pn, h, w, c.dtype, dev, c=16)
        rc = lib.vsr_debug_spy_prepare(dt, P(fr.view), P(fp.view) if fp else None, P(fu.view), x16.ptr(), c.o("n", 0), c.o("t", 0), Pn, c.o("pair_mode", 1),
                                       h, w, lv0, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(flow_up=fu.take(), x16=x16.take())
    if c.hook == "prepare_bwd":
        Pn, lv0 = b, c.o("level0", 0)
        fr, dx16 = planar_in(inp["frames"]), pm(inp["dx16"], 16)
        fu = None if lv0 else planar_in(inp["flow_up"])
        dl = None if lv0 else planar_in(inp["dflow_l"])
        dprev = None if lv0 else planar_out(Pn, 2, h // 2, w // 2, inp["dprev0"])
        dfr = planar_out(inp["frames"].shape[0], 3, h, w, inp["dframes0"]) if c.o("dframes", 1) else None
        rc = lib.vsr_debug_spy_prepare_bwd(dt, P(dx16), P(dl.view) if dl else None, P(fr.view), P(fu.view) if fu else None, P(dprev.view) if dprev else None,
                                           P(dfr.view) if dfr else None, c.o("n", 0), c.o("t", 0), Pn, c.o("pair_mode", 1), h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        out = {}
        if dfr:
            out["dframes"] = dfr.take()
        if dprev:
            out["dflow_prev"] = dprev.take()
        return out
    if c.hook == "dres":
        d = planar_in(inp["d"])
        res = planar_in(inp["res"]) if c.o("res", 1) else None
        y = T.PmOutput(b, h, w, c.dtype, dev, c=16)
        rc = lib.vsr_debug_spy_dres(dt, P(d.view), P(res.view) if res else None, y.ptr(), b, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(y=y.take())
    op = PLANAR_OPS.index(c.hook)
    hu, wu = c.o("hu", 0), c.o("wu", 0)
    mean = devf(inp["mean"]) if "mean" in inp else None
    std = devf(inp["std"]) if "std" in inp else None
    four = lambda t: t if t.dim() == 4 else t.unsqueeze(1)
    src = planar_in(four(inp["a" if c.hook == "add" else ("x" if "x" in inp else "d")]))
    src2 = planar_in(four(inp["b"])) if c.hook == "add" else None
    oshape = {"resize_norm": (b, 3, hu, wu), "resize_norm_bwd": (b, 3, h, w), "avgpool2": (b, 1, h // 2, w // 2), "avgpool2_bwd": (b, 1, h, w),
              "flow_out": (b, 2, h, w), "flow_out_bwd": (b, 2, hu, wu), "add": (b, 1, h, w)}[c.hook]
    out = planar_out(*oshape, data=four(inp["out0"]) if "out0" in inp else None)
    rc = lib.vsr_debug_spy_planar(op, P(src.view), P(src2.view) if src2 else None, P(out.view), P(mean), P(std), b, h, w, hu, wu, st)
    assert rc == 0, (c.name, rc)
    T._sync()
    y = out.take()
    return dict(y=y[:, 0] if c.hook in ("avgpool2", "avgpool2_bwd", "add") else y)


# --------------------------------------------------------------------------------------------------------------------
# the case lists of test_spynet_gpu.py (test_spynet_host.py dry-runs the criterion over them)
# --------------------------------------------------------------------------------------------------------------------
def conv_cases(shape, dtype, family="rand"):
    """Per layer the arms spynet_run runs: ReLU (j < 4); the last layer with and without ReLU, with and without pres."""
    k = lambda **o: case("conv", shape, dtype, family=family, **o)
    if shape == DEEP:
        return [k(j=j, act=1) for j in range(4)] + [k(j=4, act=1, pres=1)]
    return [k(j=j, act=1) for j in range(4)] + [k(j=4, act=1, pres=1), k(j=4, act=0, pres=1), k(j=4, act=1), k(j=4, act=0)]


def dgrad_cases(shape, dtype, family="rand"):
    k = lambda **o: case("dgrad", shape, dtype, family=family, **o)
    if shape == DEEP:
        return [k(j=j, aux=1) for j in range(1, 5)]
    return [k(j=0)] + [k(j=j, aux=1) for j in range(1, 5)] + [k(j=2), k(j=4)]


def wgrad_cases(shape, dtype, family="rand"):
    k = lambda **o: case("wgrad", shape, dtype, family=family, **o)
    if shape in (BIG, WG_MANY):
        return [k(j=j, accumulate=1) for j in range(5)]
    return [k(j=j, accumulate=1) for j in range(5)] + [k(j=0, accumulate=0), k(j=2, accumulate=0, gb=False), k(j=4, accumulate=1, gb=False)]


def conv_shapes(hook):
    return SMALL + [BIG] + ([WG_MANY] if hook == "wgrad" else [DEEP])


def families(shape, dtype):
    if shape in (DEEP, WG_MANY):
        return ("grid",)
    return ("rand", "grid")


def dtypes(shape):
    return ("bf16",) if shape == DEEP else ("bf16", "fp32")


def level_cases(size, dtype):
    """spynet_prepare, spynet_prepare_bwd in the engine's three forms, spynet_dres, add_f32, avgpool2 and its adjoint at one level size."""
    h, w = size
    lv0 = size in LEVEL0
    cs = []
    for pr in PAIRS:
        P = pr["P"] if pr["pair_mode"] else 2 * pr["n"] * (pr["t"] - 1)
        k = lambda hook, **o: case(hook, (P, h, w), dtype, **pr, **o)
        if lv0:
            cs += [k("prepare", level0=1), k("prepare_bwd", level0=1)]
        else:
            cs += [k("prepare"), k("prepare_bwd"), k("prepare_bwd", dframes=0)]
    P = 3
    cs += [case("dres", (P, h, w), dtype), case("dres", (P, h, w), dtype, res=0), case("add", (2 * P, h, w), dtype)]
    if not lv0:
        cs += [case("avgpool2", (6 * 3, h, w), dtype), case("avgpool2_bwd", (6 * 3, h, w), dtype)]
    return cs


def resize_cases(src, dst, dtype):
    (h, w), (hu, wu) = src, dst
    return [case(hk, (2, h, w), dtype, hu=hu, wu=wu) for hk in ("resize_norm", "resize_norm_bwd", "flow_out", "flow_out_bwd")]


ATOMIC = ("prepare_bwd", "flow_out_bwd", "resize_norm_bwd")      # held to the bound only: the order of their atomic adds is not fixed


def gpu_cases():
    cs = []
    for hook, make in (("conv", conv_cases), ("dgrad", dgrad_cases), ("wgrad", wgrad_cases)):
        for s in conv_shapes(hook):
            for dt in dtypes(s):
                for fam in families(s, dt):
                    cs += make(s, dt, fam)
    for dt in ("bf16", "fp32"):
        for size in LEVEL0 + LEVELS:
            cs += level_cases(size, dt)
        for src, dst in RESIZES:
            cs += resize_cases(src, dst, dt)
    return cs


def distinct(cases):
    seen, out = set(), []
    for c in cases:
        k = (_core(c), c.dtype)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out
