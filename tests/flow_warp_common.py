"""Shared by test_flow_warp_host.py and test_flow_warp_gpu.py: the flow warp of csrc/elementwise.hip (forward, the scatter and the gather
form of its adjoint, the flow gradient) restated in fp64, an elementwise error bound, and the driver of the ``vsr_debug_warp_*`` hooks
(csrc/warp_hooks.hip).  Case, Guarded, Planar, pm_input, PmOutput, measure_against / check_against and fault_guarded are
tests/hr_tail_common.py's, used as they are.

* ``reference(case)``: index arithmetic only, no ``grid_sample``.  The sample position is p = x + flow (0 where the extent is 1), clamped to
  the image in border mode; the taps are floor(p) and floor(p) + 1 with weights 1 - frac and frac, so a position on an integer has its
  second tap at weight 0 and ``d flow`` is the one-sided slope over the cell [floor(p), floor(p) + 1], which is what
  ``grid_sampler_2d_backward`` returns.  Border mode gates ``d flow`` by ATen's open interval 0 < p < dim - 1.  test_flow_warp_host.py
  pins all of it at 1e-10 to torch autograd.
* two families.  ``grid``: H - 1 and W - 1 powers of two, flows multiples of 1/4 in [-4.75, 4.75] (0, +-4.0 = the last near value and
  +-4.25 among them; two blocks of zero flow that touch all four edges), tensors from {-1, -1/2, 0, 1/2, 1}.  The fp32 round trip of
  ``warp_coord`` is then exact (asserted per case), every weight a multiple of 1/16, every term a multiple of 1/32: as long as
  32 A < 2^24 (asserted per case) an fp32 evaluation in any order and the 2^-44 fixed-point far sum are exact, so an fp32 output has to
  EQUAL the reference and a bf16 output its round-to-nearest-even.  ``rand``: values uniform(-1, 1), bf16-representable; flows
  multiples of 2^-10 such that both fractions of p lie in [1/16, 15/16] (asserted): no tap choice depends on rounding and no element
  is exempt.  Targets reach 6 px outside the image, a band of flows is far (|flow| > 4), and where the image is large enough a 5 x 5
  patch of sources aims into one cell and some more at one destination so that a destination has exactly GCAP hits and others more
  (asserted: otherwise the gather kernel's rescan arm is not covered).
* the bound, per element (rand family; the grid family's is 0):
      |err| <= u |r| (bf16 output)  +  2 K 2^-24 A  +  coordinate term  (+ 2^-45 per far hit: the fixed-point rounding)
  A: the same code on magnitudes.  K: forward 4 taps + 2 weight products; adjoint: the sources that hit the destination, + 1 for
  dtop / a, + 1 for the far share's conversion where a far source hits; ``d flow``: the channels (per channel one difference, two
  products, one sum and the accumulation: at most (C + 5) 2^-24 A, below 2 C 2^-24 A from C = 16 on).
  Coordinate term: ``warp_coord`` evaluates s = x + f, 2 s / d, - 1, + 1, * 0.5 (d - 1) with a rounding (relative 2^-24) after the sum,
  the quotient, the difference, the second sum and the last product (the factors 2 and 0.5 are exact).  In units of p these are
  |s|, |s|, |s| + d / 2, |s|, |s| times 2^-24: delta_p = 6 * 2^-24 * max(dim, |x + f|) covers their sum 5 |s| + d / 2 and the second-order
  remainder.  It multiplies the output's sensitivity to the position on magnitudes (the output is bilinear in (px, py) inside a cell,
  so sx dpx + sy dpy + sxy dpx dpy is the whole change).  delta_p is 0 where the position is exact: extent 1, a border-clamped
  position, the grid family.  No constant was tuned on a GPU.
* ``emulate(case, mut)``: the same code in fp32 on the fp32 restatement of ``warp_coord``, rounded to bf16 where the bf16 build stores;
  ``mut`` is one of MUTATIONS.
* ``run_hip(case, dev)``: one hook call.  Pixel-major inputs with NaN padding pixels in NaN-banded buffers, the flow in a NaN-filled
  planar buffer whose bits must not change, outputs between sentinel bands, ``dflow`` with sentinel gaps between its images, S all
  zero afterwards, the far counter between two sentinels."""
import functools

import torch

import hr_tail_common as T
from hr_tail_common import Case, EPS, SENTINEL, U, Guarded, Planar, PmOutput, bf16_round, draw, pm_input, sid  # noqa: F401
from trunk_common import draw_grid

GR, GCAP = 5, 8                  # csrc/elementwise.hip: the gather's search radius and the length of a destination's hit list
NEAR = float(GR - 1)             # |flow| <= 4 on both axes: near
FAR_BAD = 0x40000000
COORD_K = 6                      # delta_p = COORD_K 2^-24 max(dim, |x + f|), derived above
GRID_SHAPES = [(2, 9, 33), (1, 17, 65), (1, 5, 129)]
RAND_SHAPES = T.SHAPES + [(2, 1, 45), (1, 9, 1)]
OVER_CHUNKS = (2, 259, 261)      # x 8 chunks of 64 channels: more than grid_for's 4096 x 256 threads (forward, scatter)
OVER_PIXELS = (1, 1030, 1030)    # more than 4096 x 256 pixels (flow gradient, the far kernel); 4290 tiles for the gather
HOOKS = ("fwd", "scatter", "gather", "flowgrad")
# tap_test_inclusive   the in-image test lets index == extent through (it reads / adds to the last pixel of the row or column)
# weights_swapped      the weights of the two columns (and rows) change places
# halo_radius_4        the gather kernel built with GR = 4 (it scans +-4 and takes |flow| <= 3 for near) beside a far kernel that still
#                      leaves everything up to |flow| <= 4 to it: sources with 3 < |flow| <= 4 reach nobody
# hit_cap_truncates    a destination with more than GCAP hits keeps the first GCAP of the scan instead of rescanning
# far_share_dropped    S is not added
# far_threshold_open   |flow| == 4 counts as far (the values agree; the far counter does not)
# dtop_dropped         dtop / a is not added
# nstride_ignored      the flow of image n is read at n * 2HW whatever flow_nstride says
# border_gate_closed   border mode keeps d flow on the closed interval 0 <= p <= dim - 1
# dim1_uses_flow       at extent 1 the position is x + flow instead of 0
MUTATIONS = ("tap_test_inclusive", "weights_swapped", "halo_radius_4", "hit_cap_truncates", "far_share_dropped", "far_threshold_open",
             "dtop_dropped", "nstride_ignored", "border_gate_closed", "dim1_uses_flow")
F64, F32 = torch.float64, torch.float32


def case(hook, shape, dtype="bf16", **opts):
    return Case(hook, tuple(shape), dtype, tuple(sorted(opts.items())))


def zero_blocks(shape):
    """The two blocks of zero flow in the last image of a grid case, as (rows, columns): the top-left quadrant and a bottom-right block."""
    _, h, w = shape
    return (slice(0, (h + 1) // 2), slice(0, (w + 1) // 2)), (slice(h - (h // 4 + 1), h), slice(w - (w // 4 + 1), w))


def has_sink(shape):
    return shape[1] >= 9 and shape[2] >= 31


# --------------------------------------------------------------------------------------------------------------------
# geometry, in the dtype asked for
# --------------------------------------------------------------------------------------------------------------------
def positions(flow, h, w, dtype, mut=None):
    """(px, py) before the border clamp.  fp64: x + flow, 0 at extent 1.  fp32: ``warp_coord`` operation by operation."""
    f = flow.to(dtype)
    n = f.shape[0]
    xs = torch.arange(w, dtype=dtype).view(1, 1, w).expand(n, h, w)
    ys = torch.arange(h, dtype=dtype).view(1, h, 1).expand(n, h, w)
    out = []
    for base, fl, dim in ((xs, f[:, 0], w), (ys, f[:, 1], h)):
        if dim == 1 and mut == "dim1_uses_flow":
            p = base + fl
        elif dtype == F64:
            p = base + fl if dim > 1 else torch.zeros_like(fl)
        else:
            g = 2.0 * (base + fl) / float(max(dim - 1, 1)) - 1.0
            p = (g + 1.0) * 0.5 * float(dim - 1)
        out.append(p)
    return out


def delta_p(flow, h, w, border):
    """The bound on |warp_coord(x, f) - (x + f)| per pixel and axis (fp64); 0 where the position is exact."""
    out = []
    for p, dim in zip(positions(flow, h, w, F64), (w, h)):
        s = p if dim > 1 else torch.zeros_like(p)
        d = COORD_K * EPS * torch.maximum(s.abs(), torch.full_like(s, float(dim)))
        if dim == 1:
            d = torch.zeros_like(d)
        elif border:
            d = torch.where((p < 0) | (p > dim - 1), torch.zeros_like(d), d)
        out.append(d)
    return out


def sample(px, py, h, w, border, mut=None):
    """The four floor-based taps of every pixel: (flat index of the tap (clamped into the image), weight, in-image) and the weights."""
    if border:
        px, py = px.clamp(0, w - 1), py.clamp(0, h - 1)
    x0, y0 = px.floor(), py.floor()
    wx1, wy1 = px - x0, py - y0
    wx0, wy0 = 1 - wx1, 1 - wy1
    if mut == "weights_swapped":
        wx0, wx1, wy0, wy1 = wx1, wx0, wy1, wy0
    hi_x, hi_y = (w, h) if mut == "tap_test_inclusive" else (w - 1, h - 1)
    taps = []
    for t in range(4):
        xi, yi = x0 + (t & 1), y0 + (t >> 1)
        valid = (xi >= 0) & (xi <= hi_x) & (yi >= 0) & (yi <= hi_y)
        idx = torch.nan_to_num(yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()      # (a NaN position: NaN weights, any index)
        taps.append((idx, (wx1 if t & 1 else wx0) * (wy1 if t >> 1 else wy0), valid))
    return dict(taps=taps, wx=(wx0, wx1), wy=(wy0, wy1))


def _pix(v):
    """(N, H, W) -> (N, 1, HW): a per-pixel factor of an (N, C, HW) tensor."""
    return v.flatten(1)[:, None, :]


def _take(x, idx):
    """x (N, C, H, W) at the per-pixel flat indices idx (N, H, W): (N, C, HW)."""
    return x.flatten(2).gather(2, idx.flatten(1)[:, None, :].expand(-1, x.shape[1], -1))


def _fwd(x, s):
    out = None
    for idx, wgt, valid in s["taps"]:
        term = _take(x, idx) * _pix(wgt * valid)
        out = term if out is None else out + term
    return out.view_as(x)


def _adj(g, s, select=None, wgts=None):
    """sum over sources (of `select`) of weight x g[source] at each in-image tap; wgts: other per-tap weights (the sensitivities)."""
    n, c, h, w = g.shape
    out = torch.zeros(n, c, h * w, dtype=g.dtype)
    gf = g.flatten(2)
    for k, (idx, wgt, valid) in enumerate(s["taps"]):
        m = valid if select is None else valid & select
        out.scatter_add_(2, idx.flatten(1)[:, None, :].expand(-1, c, -1), gf * _pix((wgt if wgts is None else wgts[k]) * m))
    return out.view_as(g)


def _adj_capped(g, s, select):
    """_adj, but a destination keeps only its first GCAP hits in the kernel's scan order (sources row by row)."""
    n, c, h, w = g.shape
    hw = h * w
    out = torch.zeros(n, c, hw, dtype=g.dtype)
    for i in range(n):
        ok = torch.cat([(valid & select)[i].flatten() for _, _, valid in s["taps"]])
        dest = torch.cat([idx[i].flatten() for idx, _, _ in s["taps"]])[ok]
        wgt = torch.cat([wg[i].flatten() for _, wg, _ in s["taps"]])[ok]
        src = torch.arange(hw).repeat(4)[ok]
        order = torch.argsort(dest * hw + src)
        dest, src, wgt = dest[order], src[order], wgt[order]
        rank = torch.arange(len(dest)) - torch.searchsorted(dest, dest)
        keep = rank < GCAP
        out[i].index_add_(1, dest[keep], g[i].flatten(1)[:, src[keep]] * wgt[keep])
    return out.view_as(g)


def hits(s, select, shape):
    """(N, H, W): how many sources of `select` have an in-image tap on each destination (weight-0 taps count, as in the kernel)."""
    n, h, w = shape
    one = torch.ones(n, 1, h, w, dtype=F64)
    ones = [torch.ones(n, h, w, dtype=F64)] * 4
    return _adj(one, s, select, ones)[:, 0].round().long()


def is_far(flow, mut=None):
    ax, ay = flow[:, 0].abs(), flow[:, 1].abs()
    if mut == "far_threshold_open":
        return ~((ax < NEAR) & (ay < NEAR))
    return ~((ax <= NEAR) & (ay <= NEAR))


def _dflow(x, g, s, px, py, h, w, border, mut=None, mag=False):
    """(N, 2, H, W).  mag: the same sums on magnitudes (every difference a sum), ungated."""
    n = x.shape[0]
    v = [_take(x, idx) * _pix(valid) for idx, _, valid in s["taps"]]
    d = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    (wx0, wx1), (wy0, wy1) = s["wx"], s["wy"]
    gf = g.flatten(2)
    gx = (gf * (_pix(wy0) * d(v[1], v[0]) + _pix(wy1) * d(v[3], v[2]))).sum(1).view(n, h, w)
    gy = (gf * (_pix(wx0) * d(v[2], v[0]) + _pix(wx1) * d(v[3], v[1]))).sum(1).view(n, h, w)
    if not mag:
        gates = []
        for p, dim in ((px, w), (py, h)):
            gate = torch.full_like(p, dim > 1, dtype=torch.bool)
            if border:
                gate &= ((p >= 0) & (p <= dim - 1)) if mut == "border_gate_closed" else ((p > 0) & (p < dim - 1))
            gates.append(gate)
        gx, gy = torch.where(gates[0], gx, torch.zeros_like(gx)), torch.where(gates[1], gy, torch.zeros_like(gy))
    return torch.stack([gx, gy], 1)


def _misstrided(flow, nmul):
    """What a kernel that ignores flow_nstride reads: image n at n * 2HW of a NaN-filled buffer with the images nmul * 2HW apart."""
    n, _, h, w = flow.shape
    ns = nmul * 2 * h * w
    flat = torch.full(((n - 1) * ns + 2 * h * w,), float("nan"), dtype=flow.dtype)
    flat.as_strided((n, 2, h, w), (ns, h * w, w, 1)).copy_(flow)
    return flat.as_strided((n, 2, h, w), (2 * h * w, h * w, w, 1)).clone()


def _ops(c: Case, t, dtype, mut=None):
    """The operation of `c` on the tensors t (of `dtype`; the flow stays fp32) -> dict output name -> tensor (+ `_far`: the far counter)."""
    n, h, w = c.shape
    border = c.o("border", 0)
    flow = t["flow"]
    if mut == "nstride_ignored" and c.o("nmul", 1) > 1:
        flow = _misstrided(flow, c.o("nmul"))
    px, py = positions(flow, h, w, dtype, mut)
    s = sample(px, py, h, w, border, mut)
    top = t["top"] if (c.o("top", 0) and mut != "dtop_dropped") else None
    if c.hook == "fwd":
        return dict(out=_fwd(t["x"], s))
    if c.hook == "scatter":
        out = _adj(t["g"], s)
        return dict(out=out if top is None else top + out)
    if c.hook == "gather":
        far = is_far(flow, mut)
        near = ~is_far(flow) if mut != "halo_radius_4" else ((flow[:, 0].abs() <= NEAR - 1) & (flow[:, 1].abs() <= NEAR - 1))
        out = _adj_capped(t["g"], s, near) if mut == "hit_cap_truncates" else _adj(t["g"], s, near)
        if mut != "far_share_dropped":
            out = out + _adj(t["g"], s, far)
        return dict(out=out if top is None else out + top, _far=int(far.sum()))
    if c.hook == "flowgrad":
        return dict(dflow=_dflow(t["x"], t["g"], s, px, py, h, w, border, mut))
    raise KeyError(c.hook)


# --------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------
def _frac(gen, *shape):
    """Multiples of 2^-10 in [1/16, 15/16], fp64."""
    return 1 / 16 + torch.randint(0, 897, shape, generator=gen).double() / 1024


def near_hits(flow, h, w):
    px, py = positions(flow, h, w, F64)
    return hits(sample(px, py, h, w, 0), ~is_far(flow), (flow.shape[0], h, w))


def make_flow(shape, family, seed):
    """(N, 2, H, W) fp32."""
    n, h, w = shape
    gen = torch.Generator().manual_seed(int(seed))
    if family == "grid":
        f = torch.randint(-19, 20, (n, 2, h, w), generator=gen).double() / 4
        (ya, xa), (yb, xb) = zero_blocks(shape)             # zero flow in two blocks of the last image that touch all four edges
        f[-1, :, ya, xa] = 0
        f[-1, :, yb, xb] = 0
        special = [(4.0, 0.0), (-4.0, 0.0), (4.25, 0.0), (-4.25, 0.0), (0.0, 4.0), (0.0, -4.0), (0.0, 4.25), (0.0, -4.25), (4.0, 4.0), (-4.0, -4.25)]
        for i, (fx, fy) in enumerate(special):
            f[0, 0, h - 2, 1 + i], f[0, 1, h - 2, 1 + i] = fx, fy
        return f.float()
    ys = torch.arange(h).view(1, 1, h, 1).expand(n, 2, h, w)
    xs = torch.arange(w).view(1, 1, 1, w).expand(n, 2, h, w)
    di = torch.randint(-4, 4, (n, 2, h, w), generator=gen)                 # near: |flow| < 4
    dfar = torch.randint(-10, 10, (n, 2, h, w), generator=gen)             # the far band: rows 3, 10, .. and columns 6, 19, ..
    di = torch.where((ys % 7 == 3) | (xs % 13 == 6), dfar, di)
    f = di.double() + _frac(gen, n, 2, h, w)
    if h * w > 1:                                                          # 6 px outside the image at both ends of both axes
        f[:, :, 0, 0] = -6 + _frac(gen, n, 2)
        f[:, :, h - 1, w - 1] = 5 + _frac(gen, n, 2)
    if has_sink(shape):
        for y in range(2, 7):                                              # 25 sources into the cell (4..5, 12..13) of image 0
            for x in range(10, 15):
                f[0, 0, y, x], f[0, 1, y, x] = 12 - x + _frac(gen), 4 - y + _frac(gen)
        # ... and a destination (4, x) of image 0 with exactly GCAP hits: sources around it that miss it are aimed into the cell it opens
        for dx in range(22, w - 4):
            cnt = int(near_hits(f.float(), h, w)[0, 4, dx])
            if cnt > GCAP:
                continue
            px, py = positions(f.float(), h, w, F64)
            for y in range(2, 7):
                for x in range(dx - 2, dx + 3):
                    hit_now = 0 <= dx - int(px[0, y, x].floor()) <= 1 and 0 <= 4 - int(py[0, y, x].floor()) <= 1 and not bool(is_far(f.float())[0, y, x])
                    if cnt < GCAP and not hit_now:
                        f[0, 0, y, x], f[0, 1, y, x] = dx - x + _frac(gen), 4 - y + _frac(gen)
                        cnt += 1
            break
    return f.float()


@functools.lru_cache(maxsize=3)
def make_inputs(shape, C, family):
    """CPU fp32 tensors of one (shape, width, family): x the warped tensor, g the cotangent, top what the adjoint is added to, flow."""
    n, h, w = shape
    s = 11000 + 131 * h + 17 * w + n + 7 * C + (500 if family == "grid" else 0)
    d = draw_grid if family == "grid" else draw
    return dict(x=d(s, n, C, h, w), g=d(s + 1, n, C, h, w), top=d(s + 2, n, C, h, w), flow=make_flow(shape, family, s + 3))


def inputs_of(c: Case):
    return make_inputs(c.shape, c.o("C", 64), c.o("family", "rand"))


# --------------------------------------------------------------------------------------------------------------------
# reference and bound
# --------------------------------------------------------------------------------------------------------------------
def _core(c: Case):
    """The case without what changes only the operands' placement or the build."""
    return Case(c.hook, c.shape, "any", tuple((k, v) for k, v in c.opts if k != "nmul"))


@functools.lru_cache(maxsize=4)
def _values(c: Case):
    n, h, w = c.shape
    C, fam, border = c.o("C", 64), c.o("family", "rand"), c.o("border", 0)
    inp = inputs_of(c)
    t = {k: (v.double() if k != "flow" else v) for k, v in inp.items()}
    mag = {k: (v.abs() if k != "flow" else v) for k, v in t.items()}
    flow = inp["flow"]
    px, py = positions(flow, h, w, F64)
    s = sample(px, py, h, w, border)
    if fam == "grid":
        assert all(torch.equal(a.double(), b) for a, b in zip(positions(flow, h, w, F32), (px, py))), (c.name, "the fp32 round trip is not exact")
        dpx, dpy = torch.zeros_like(px), torch.zeros_like(py)
    else:
        for p, dim in ((px, w), (py, h)):
            fr = p - p.floor()
            assert dim == 1 or bool(((fr >= 1 / 16) & (fr <= 15 / 16)).all()), (c.name, "a fraction outside [1/16, 15/16]")
        dpx, dpy = delta_p(flow, h, w, border)
    r = {k: v for k, v in _ops(c, t, F64).items()}
    meta = {}
    if c.hook == "fwd":
        a = _fwd(mag["x"], s)
        K = torch.full_like(a, 6.0)
        v = [_take(mag["x"], idx) * _pix(valid) for idx, _, valid in s["taps"]]
        (wx0, wx1), (wy0, wy1) = s["wx"], s["wy"]
        sx = _pix(wy0) * (v[1] + v[0]) + _pix(wy1) * (v[3] + v[2])
        sy = _pix(wx0) * (v[2] + v[0]) + _pix(wx1) * (v[3] + v[1])
        coord = (_pix(dpx) * sx + _pix(dpy) * sy + _pix(dpx * dpy) * (v[0] + v[1] + v[2] + v[3])).view_as(a)
        out = dict(out=(r["out"], a, K, coord))
    elif c.hook in ("scatter", "gather"):
        a = _adj(mag["g"], s)
        far = is_far(flow) if c.hook == "gather" else torch.zeros_like(px, dtype=torch.bool)
        all_hits, far_hits = hits(s, None, c.shape), hits(s, far, c.shape)
        K = (all_hits + (far_hits > 0)).double()
        if c.o("top", 0):
            a, K = a + mag["top"], K + 1
        (wx0, wx1), (wy0, wy1) = s["wx"], s["wy"]
        sens = [dpx * (wy1 if k >> 1 else wy0) + dpy * (wx1 if k & 1 else wx0) + dpx * dpy for k in range(4)]
        coord = _adj(mag["g"], s, None, sens) + (far_hits.double() * 2.0 ** -45)[:, None]
        out = dict(out=(r["out"], a, K[:, None].expand_as(a), coord))
        if c.hook == "gather":
            meta["far"] = int(far.sum())
            nh = hits(s, ~far, c.shape)
            meta["max_hits"] = int(nh.max())
            if fam == "rand" and has_sink(c.shape):
                assert bool((nh == GCAP).any()) and bool((nh > GCAP).any()), (c.name, "the rescan arm and its threshold are not covered")
    elif c.hook == "flowgrad":
        a = _dflow(mag["x"], mag["g"], s, px, py, h, w, border, mag=True)
        v4 = sum(_take(mag["x"], idx) * _pix(valid) for idx, _, valid in s["taps"])
        sxy = (mag["g"].flatten(2) * v4).sum(1).view(n, h, w)
        coord = torch.stack([dpy * sxy, dpx * sxy], 1)      # d flow_x depends on py through the row weights, d flow_y on px
        gate = torch.stack(_gates(px, py, h, w, border), 1)      # a gated-off element is exactly 0 whatever the taps hold: bound 0
        a, coord = a * gate, coord * gate
        out = dict(dflow=(r["dflow"], a, torch.full_like(a, float(C)), coord))
    else:
        raise KeyError(c.hook)
    if fam == "grid":
        for k, (_, a, _, _) in out.items():
            assert float(a.max()) * 32 < 2.0 ** 24, (c.name, k, "the magnitudes do not keep fp32 exact")
    return out, meta


def _gates(px, py, h, w, border):
    gs = []
    for p, dim in ((px, w), (py, h)):
        gate = torch.full_like(p, float(dim > 1))
        if border:
            gate = gate * ((p > 0) & (p < dim - 1))
        gs.append(gate)
    return gs


def reference(c: Case):
    """(dict name -> (r, A, K, coordinate term), meta): fp64, computed once per operation, shape, width and family."""
    return _values(_core(c))


def bf16_outputs(c: Case):
    return ("out",) if c.dtype == "bf16" and c.hook != "flowgrad" else ()


def targets(c: Case):
    """(dict name -> what the output is compared with, dict name -> (accumulation term, the other terms))."""
    vals, _ = reference(c)
    grid = c.o("family", "rand") == "grid"
    r, b = {}, {}
    for k, (rv, a, K, coord) in vals.items():
        if grid:
            r[k] = bf16_round(rv.float()).double() if k in bf16_outputs(c) else rv
            b[k] = (torch.zeros_like(rv), torch.zeros_like(rv))
        else:
            r[k] = rv
            b[k] = (2 * K * EPS * a, coord + (U * rv.abs() if k in bf16_outputs(c) else 0))
    return r, b


def _tensors(got):
    return {k: v for k, v in got.items() if not k.startswith("_")}


def measure(c: Case, got):
    r, b = targets(c)
    return T.measure_against(c.name, _tensors(got), r, b)


def far_ok(c: Case, got):
    return c.hook != "gather" or got["_far"] == reference(c)[1]["far"]


def passes(c: Case, got):
    return far_ok(c, got) and all(v[0] <= 1.0 for v in measure(c, got).values())


def check(c: Case, got, label="hip"):
    """Every element inside its bound (grid family: equal), the far counter the reference's; prints and returns the worst ratios."""
    r, b = targets(c)
    m = T.check_against(c.name, _tensors(got), r, b, label, tag="FLOW_WARP_RATIO")
    assert far_ok(c, got), (c.name, "far counter", got["_far"], reference(c)[1]["far"])
    return m


def emulate(c: Case, mut=None):
    t = {k: v.float() for k, v in inputs_of(c).items()}
    out = _ops(c, t, F32, mut)
    return {k: (bf16_round(v) if k in bf16_outputs(c) else v) for k, v in out.items()}


def same_bits(a, b):
    return T.same_bits(_tensors(a), _tensors(b))


# --------------------------------------------------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------------------------------------------------
S_FILL = 0x5A5A5A5A5A5A5A5A
FAR_FILL = -77


def run_hip(c: Case, dev):
    """One hook call on the inputs of `c`; dict output name -> fp32 CPU tensor (+ `_far`).  A HIP error ends the session."""
    return T.fault_guarded(c, _run_hip, dev)


def _run_hip(c: Case, dev):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    inp = inputs_of(c)
    n, h, w = c.shape
    C, border = c.o("C", 64), c.o("border", 0)
    dt = VF.DT_BF16 if c.dtype == "bf16" else VF.DT_F32
    st, nan = VF._stream(), float("nan")
    ns = c.o("nmul", 1) * 2 * h * w
    flow = Planar(n, 2, h, w, ns, dev, nan, inp["flow"])
    flow_bits = flow.g.buf.view(torch.int32).clone()
    top = pm_input(inp["top"], c.dtype, dev) if c.o("top", 0) else None
    P = lambda t: None if t is None else t.data_ptr()

    def done(rc):
        assert rc == 0, (c.name, rc)
        T._sync()
        assert torch.equal(flow.g.buf.view(torch.int32), flow_bits), (c.name, "the flow buffer was written")

    if c.hook == "fwd":
        x, out = pm_input(inp["x"], c.dtype, dev), PmOutput(n, h, w, c.dtype, dev, c=C)
        done(lib.vsr_debug_warp_fwd(dt, C, P(x), P(flow.view), ns, out.ptr(), border, n, h, w, st))
        return dict(out=out.take())
    if c.hook == "scatter":
        g, out = pm_input(inp["g"], c.dtype, dev), PmOutput(n, h, w, c.dtype, dev, c=C)
        acc = Guarded(n * h * w * C, torch.float32, dev, SENTINEL)
        acc.body.zero_()
        done(lib.vsr_debug_warp_scatter(dt, C, P(g), P(flow.view), ns, P(acc.body), P(top), out.ptr(), border, n, h, w, st))
        assert acc.bands_untouched(), (c.name, "the scatter accumulator was written outside its tensor")
        return dict(out=out.take())
    if c.hook == "gather":
        g, out = pm_input(inp["g"], c.dtype, dev), PmOutput(n, h, w, c.dtype, dev, c=C)
        numel = n * h * w * C
        sbuf = torch.full((numel + 2 * T.GUARD,), S_FILL, dtype=torch.int64, device=dev)
        body = sbuf[T.GUARD:T.GUARD + numel]
        body.zero_()
        far = torch.tensor([FAR_FILL, 0, FAR_FILL], dtype=torch.int32, device=dev)
        done(lib.vsr_debug_warp_gather(dt, C, P(g), P(flow.view), ns, P(top), P(body), P(far[1:]), out.ptr(), n, h, w, st))
        assert not bool(body.any()), (c.name, "S is not all zero after the call")
        assert bool((sbuf[:T.GUARD] == S_FILL).all()) and bool((sbuf[T.GUARD + numel:] == S_FILL).all()), (c.name, "S was written outside its tensor")
        fc = far.cpu().tolist()
        assert fc[0] == FAR_FILL and fc[2] == FAR_FILL and not fc[1] & FAR_BAD, (c.name, "far counter", fc)
        return dict(out=out.take(), _far=fc[1])
    if c.hook == "flowgrad":
        x, g = pm_input(inp["x"], c.dtype, dev), pm_input(inp["g"], c.dtype, dev)
        dflow = Planar(n, 2, h, w, ns, dev, SENTINEL)
        done(lib.vsr_debug_warp_flowgrad(dt, C, P(x), P(g), P(flow.view), ns, P(dflow.view), border, n, h, w, st))
        return dict(dflow=dflow.take())
    raise KeyError(c.hook)


def run_add_cast(a, s, dtype, dev):
    """vsr_debug_warp_add_cast on a (N, C, H, W) or None and s (N, C, H, W) or None (handed over as plain [N][H][W][C] fp32)."""
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    n, C, h, w = (a if a is not None else s).shape
    c = case("add_cast", (n, h, w), dtype, C=C)

    def go(c, dev):
        a_pm = pm_input(a, dtype, dev) if a is not None else None
        sg = None
        if s is not None:
            sg = Guarded(s.numel(), torch.float32, dev, float("nan"))
            sg.body.copy_(s.permute(0, 2, 3, 1).contiguous().flatten().to(dev))
        out = PmOutput(n, h, w, dtype, dev, c=C)
        rc = lib.vsr_debug_warp_add_cast(VF.DT_BF16 if dtype == "bf16" else VF.DT_F32, C, None if a_pm is None else a_pm.data_ptr(),
                                         None if sg is None else sg.body.data_ptr(), out.ptr(), n, h, w, VF._stream())
        assert rc == 0, (c.name, rc)
        T._sync()
        return out.take()

    return T.fault_guarded(c, go, dev)


def run_converters(x, C, dtype, dev):
    """vsr_planar_to_pm of x (N, Cin, H, W) into C channels, then vsr_pm_to_planar of all C channels: (the C-channel image as
    from_pixel_major reads it, the planar round trip (N, C, H, W), whether every padding pixel still holds the sentinel)."""
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    n, cin, h, w = x.shape
    c = case("converters", (n, h, w), dtype, C=C, cin=cin)

    def go(c, dev):
        dt = VF.DT_BF16 if dtype == "bf16" else VF.DT_F32
        src = Planar(n, cin, h, w, cin * h * w, dev, float("nan"), x)
        pm = PmOutput(n, h, w, dtype, dev, c=C)
        assert lib.vsr_planar_to_pm(dt, src.view.data_ptr(), pm.ptr(), n, cin, h, w, C, VF._stream()) == 0, c.name
        back = Planar(n, C, h, w, C * h * w, dev, SENTINEL)
        assert lib.vsr_pm_to_planar(dt, pm.ptr(), back.view.data_ptr(), n, C, h, w, C, VF._stream()) == 0, c.name
        T._sync()
        v = pm.g.body.view(pm.shape)
        r = w % 32
        pad_ok = True if not r else bool((v[:, :, -1, :, r:, :].float() == SENTINEL).all())
        return pm.take(), back.take(), pad_ok

    return T.fault_guarded(c, go, dev)


# --------------------------------------------------------------------------------------------------------------------
# the cases of test_flow_warp_gpu.py (test_flow_warp_host.py dry-runs the criterion over them)
# --------------------------------------------------------------------------------------------------------------------
def hook_cases(hook, shape, C, family, dtype="bf16"):
    """Both padding modes, top given and NULL, flow_nstride 2HW and 3 x 2HW."""
    k = lambda **o: case(hook, shape, dtype, C=C, family=family, **o)
    if hook == "fwd":
        return [k(border=0, nmul=1), k(border=1, nmul=3), k(border=0, nmul=3)]
    if hook == "scatter":
        return [k(border=0, top=0, nmul=1), k(border=1, top=1, nmul=3), k(border=0, top=1, nmul=3)]
    if hook == "gather":
        return [k(top=0, nmul=1), k(top=1, nmul=3)]
    if hook == "flowgrad":
        return [k(border=0, nmul=3), k(border=1, nmul=1), k(border=1, nmul=3)]
    raise KeyError(hook)


# (shape, family, C): every shape at 64 channels; 16 and 32 at a ragged two-image shape of either family
PLACES = [(s, "rand", 64) for s in RAND_SHAPES] + [(s, "grid", 64) for s in GRID_SHAPES] + \
         [(s, f, C) for C in (16, 32) for s, f in (((2, 13, 37), "rand"), ((2, 9, 33), "grid"))]


def over_cap_cases():
    """One launch each, bf16: past grid_for's 4096 workgroups (and the far kernel's own 4096)."""
    return [case("fwd", OVER_CHUNKS, C=64, family="rand", border=0, nmul=1), case("scatter", OVER_CHUNKS, C=64, family="rand", border=0, top=1, nmul=1),
            case("gather", OVER_PIXELS, C=16, family="rand", top=1, nmul=1), case("flowgrad", OVER_PIXELS, C=16, family="rand", border=0, nmul=1)]


def gpu_cases():
    cs = []
    for shape, fam, C in PLACES:
        for hook in HOOKS:
            for dt in ("bf16", "fp32"):
                cs += hook_cases(hook, shape, C, fam, dt)
    return cs + over_cap_cases()


def distinct(cases):
    """One case per (operation, values, dtype), preferring the wider flow stride (the one a mutation can show at)."""
    seen = {}
    for c in cases:
        k = (_core(c), c.dtype)
        if k not in seen or c.o("nmul", 1) > seen[k].o("nmul", 1):
            seen[k] = c
    return list(seen.values())
