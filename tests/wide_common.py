"""Shared by test_wide_host.py and test_wide_gpu.py: the GAN side's launches (csrc/conv_wide.hip, the weight gradients of the wide layers,
perceptual_engine.hip's own kernels) restated in fp64, the elementwise bound of tests/hr_tail_common.py, and the driver of the
``vsr_debug_wide_*`` / ``vsr_debug_vgg_*`` hooks (csrc/wide_hooks.hip).

* ``reference(case)``: every operation from its definition in plain torch, float64 -- ``F.conv2d`` (padding 1; 4x4 stride 2),
  ``F.conv_transpose2d`` for the data gradients, autograd's weight gradient, ``F.interpolate(scale_factor=2, mode="bilinear",
  align_corners=False)`` and its autograd adjoint, ``F.max_pool2d(., 2, 2)`` and its autograd routing, ``sum |s - h|`` and ``sign``.  The
  epilogue of a wide conv, in the kernel's order: v = acc + bias -> activation -> y_act = v -> v += res -> v *= (aux > 0 ? 1 : slope), +0
  where the slope is 0 -> y.
* ``emulate(case, mut)``: the same operation ASSEMBLED the way the launches are described -- 64-channel slices, the parity-view sum of
  four 2x2-tap convolutions, the four output phases, separable (1/4, 3/4) upsampling with clamped borders, explicit first-argmax routing
  -- in fp32 with the slice order reversed, rounded where the build stores.  test_wide_host.py pins the assembly to the definitions at
  1e-10; ``mut`` names one of MUTATIONS, a deliberately wrong variant that ``check`` has to reject.
* ``check(case, got)``: every output element, with u = 2^-8:  bf16 output |err| <= u |r| + 2 K 2^-24 A,  fp32 output |err| <= 2 K 2^-24 A.
  K: the products summed into one element -- 9 cin, 4 cin for the stride-2 forms (each output meets 4 taps per channel in either
  direction), N H W for a weight gradient, 9 (18 with the skip) for up2, 16 for its adjoint, 2 for the pool's adjoint, 1 for the mask, 8
  for the fp32 part of a tap sum.  A: the sum of the absolute products from the same definition on the operands' magnitudes, plus |bias|,
  |res| and the pre-filled |gw| (each is one more term of the sum; K stays the product count).  An activation is 1-Lipschitz and a mask a
  factor <= 1: A is taken without the former and times the latter, so what a ReLU mask zeroes has bound 0.  Copies and selections (max
  pool, the tap's sign) have bound 0.  Grid family ({-1, -1/2, 0, 1/2, 1}): every partial sum is exact in fp32 in any order (A < 2^22 is
  asserted), so the bound is 0 against the reference rounded as the build stores, each fp32 step of the epilogue rounded in turn.
  Besides the bound: no element that a slope-0 mask zeroes may be -0.
* ``run_hip(case, dev)``: one hook call.  Every input is a blocked pixel-major tensor in a NaN-banded buffer with NaN padding pixels;
  every output sits between sentinel bands; the weight-gradient slab is filled with the sentinel."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import hr_tail_common as T
from hr_tail_common import Case, EPS, SENTINEL, U, bf16_round, draw, draw_aux, sid
from trunk_common import draw_grid

SLOPE = T.SLOPE2                    # LeakyReLU(0.2) as the kernels hold it (fp32)
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
# (N, H, W) of the conv domain; tiles are 8 rows x 32 pixels.  (1,2,5): the discriminator's coarsest level for a 16 x 40 frame
SHAPES = [(1, 1, 1), (1, 2, 5), (1, 8, 32), (2, 13, 37), (1, 3, 66), (1, 9, 31), (1, 17, 100)]
MANY = [((1, 40, 200), 3), ((3, 24, 70), 4)]         # (shape, max_wg): 35 tiles on 3 workgroups; 27 on 4, strides cross image boundaries
UNCAPPED = (3, 80, 352)             # 330 tiles on 256 workgroups
WG_MANY = (3, 72, 200)              # the weight gradient with several tiles per pixel part
UP2_SOURCES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 33), (13, 37), (17, 100)]
POOL_INPUTS = [(2, 2), (3, 5), (8, 64), (13, 37), (9, 31), (17, 100), (16, 66)]
MUTATIONS = ("views_swapped", "phases_swapped", "tap_mirrored", "drop_last_slice", "halves_swapped", "ksplit_half_dropped", "res_before_act",
             "y_act_after_res", "mask_before_res", "mask_ge", "masked_zero_negative", "drop_last_column", "halo_reads_beyond_w", "up2_no_clamp",
             "up2_adjoint_unfolded", "wgrad_view_wrong_ky", "wgrad_overwrites", "wgrad_empty_part_unwritten", "pool_last_max",
             "pool_mask_skipped_on_dropped_row", "tap_sign0_scale", "tap_padding_counted")


def case(hook, shape, dtype="bf16", **opts):
    return Case(hook, tuple(shape), dtype, tuple(sorted(opts.items())))


def pair_ksplit(npairs, tiles):
    """WideCtx::pair_ksplit (csrc/wide_recipes.h): pixel parts of a pair-batched weight-gradient launch."""
    k = max(((512 // npairs) + 7) & ~7, 8)
    return min(k, (tiles + 7) & ~7)


def tiles_of(shape):
    n, h, w = shape
    return n * ((h + 7) // 8) * ((w + 31) // 32)


# --------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------
def _specials(t):
    """+0, -0, +-2^-133 on channels 0..3 of the first and the last column."""
    special = torch.tensor([0.0, -0.0, T.SUBNORMAL, -T.SUBNORMAL])
    for col in (0, t.shape[-1] - 1):
        t[:, 0:4, :, col] = special.view(1, 4, 1)
    return t


def pool_input(seed, *shape):
    """{-1/2, 0, 1/2} with +-0 and +-2^-133 on the borders: the maximum of most 2 x 2 windows is tied."""
    return _specials(torch.sign(draw_grid(seed, *shape)) * 0.5)


def _in_shape(c: Case):
    """(x channels, x height, x width, y channels, y height, y width) of a conv case."""
    n, h, w = c.shape
    mode, cout, cin = c.o("mode", 0), c.o("cout"), c.o("cin")
    xs = 2 if mode == 1 else 1
    ys = 2 if mode == 3 else 1
    return (cout if mode >= 2 else cin), h * xs, w * xs, (cin if mode >= 2 else cout), h * ys, w * ys


@functools.lru_cache(maxsize=3)
def make_inputs(hook, shape, key):
    n, h, w = shape
    o = dict(key)
    fam = o.get("family", "rand")
    d = draw_grid if fam == "grid" else draw
    s = 9000 + 131 * h + 17 * w + n
    if hook == "conv":
        c0 = Case(hook, shape, "any", key)
        xC, hx, wx, yC, hy, wy = _in_shape(c0)
        ks = 4 if o.get("mode", 0) in (1, 3) else 3
        wt = d(s + 1, o["cout"], o["cin"], ks, ks)
        bias = d(s + 2, yC) if fam == "grid" else torch.randn(yC, generator=torch.Generator().manual_seed(s + 2))
        return dict(x=d(s, n, xC, hx, wx), w=wt, bias=bias, res=d(s + 3, n, yC, hy, wy), aux=draw_aux(s + 4, n, hy, wy, yC))
    if hook == "wgrad":
        st = 2 if o["views"] == 4 else 1
        ks = 4 if o["views"] == 4 else 3
        return dict(x=d(s + 10, n, o["xC"], h * st, w * st), dy=d(s + 11, n, o["dyC"], h, w), gw0=d(s + 12, o["dyC"], o["xC"], ks, ks))
    C = o.get("C", 64)
    if hook == "up2_fwd":
        return dict(a=d(s + 20, n, C, h, w), b=d(s + 21, n, C, h, w))
    if hook == "up2_bwd":
        return dict(dout=d(s + 30, n, C, 2 * h, 2 * w), m=draw_aux(s + 31, n, h, w, C))
    if hook == "mask":
        return dict(g=d(s + 40, n, C, h, w), m=draw_aux(s + 41, n, h, w, C))
    if hook == "pool_fwd":
        return dict(a=pool_input(s + 50, n, C, h, w))
    if hook == "pool_bwd":
        return dict(a=pool_input(s + 50, n, C, h, w), g=d(s + 51, n, C, h, w), dp=d(s + 52, n, C, h // 2, w // 2))
    if hook == "tap":
        sr, hr = d(s + 60, n, C, h, w), d(s + 61, n, C, h, w)
        same = torch.rand(n, C, h, w, generator=torch.Generator().manual_seed(s + 62)) < 0.25      # a fixed share with s == h exactly
        hr = torch.where(same, sr, hr)
        hr[:, 0, :, 0] = sr[:, 0, :, 0]
        return dict(s=sr, h=hr)
    raise KeyError(hook)


_PLACEMENT = ("max_wg",)


def _key(c: Case):
    return tuple((k, v) for k, v in c.opts if k not in _PLACEMENT)


def inputs_of(c: Case):
    keep = {"conv": ("mode", "cout", "cin", "family"), "wgrad": ("views", "xC", "dyC", "family")}.get(c.hook, ("C", "family"))
    return make_inputs(c.hook, c.shape, tuple((k, v) for k, v in c.opts if k in keep))


# --------------------------------------------------------------------------------------------------------------------
# the definitions (reference) and the assembled forms (emulation, mutations)
# --------------------------------------------------------------------------------------------------------------------
def conv_def(x, w, mode):
    """The reference's definition of the four modes."""
    if mode == 0:
        return F.conv2d(x, w, padding=1)
    if mode == 1:
        return F.conv2d(x, w, stride=2, padding=1)
    if mode == 2:
        return F.conv_transpose2d(x, w, padding=1)
    return F.conv_transpose2d(x, w, stride=2, padding=1)


def _c3(x, w3, mut=None):
    """3x3 'same' convolution."""
    if mut == "halo_reads_beyond_w":                       # the column right of the image is the NaN padding, not zero
        xp = F.pad(x, (1, 1, 1, 1))
        xp[:, :, 1:-1, -1] = float("nan")
        return F.conv2d(xp, w3)
    return F.conv2d(x, w3, padding=1)


def _s2_fwd(parity, d):
    """(view parity, offset d in {-1, 0, 1}) -> the 4x4 tap index, or -1: out(y) = sum_k W[k] in(2 y + k - 1)."""
    k = 2 * d + parity + 1                                 # view_p(y + d) = in(2 y + 2 d + p)
    return k if 0 <= k <= 3 else -1


def _s2_bwd(phase, d):
    """(output phase, offset d) -> tap: dX(2 q + p) = sum_k W[k] dY(q + d), 2 (q + d) + k - 1 = 2 q + p."""
    k = phase + 1 - 2 * d
    return k if 0 <= k <= 3 else -1


def conv_views(x, w, mode, mut=None, rev=False):
    """The four modes assembled from 64-channel slices of 3x3-tap convolutions: mode 1 as the sum over the four parity views of its input
    (view_p(y, x) = in(2 y + p_y, 2 x + p_x)), mode 3 as four output phases."""
    dgrad = mode >= 2
    if mut == "tap_mirrored" and mode in (1, 3):           # ky <-> 3 - ky
        w = w.flip(2)
    xC = x.shape[1]
    starts = list(range(0, xC, 64))
    if rev:
        starts = starts[::-1]
    out = None
    for s0 in starts:
        keep = 32 if mut == "ksplit_half_dropped" else 64
        xs = x[:, s0:s0 + keep]
        ws = w[s0:s0 + keep] if dgrad else w[:, s0:s0 + keep]
        if mode == 0:
            part = _c3(xs, ws, mut)
        elif mode == 2:
            part = _c3(xs, ws.transpose(0, 1).flip(2, 3), mut)
        elif mode == 1:
            part = None
            for v in range(4):
                py, px = v >> 1, v & 1
                src = {1: 2, 2: 1}.get(v, v) if mut == "views_swapped" else v
                xv = xs[:, :, (src >> 1)::2, (src & 1)::2]
                w3 = ws.new_zeros(ws.shape[0], ws.shape[1], 3, 3)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ky, kx = _s2_fwd(py, dy), _s2_fwd(px, dx)
                        if ky >= 0 and kx >= 0:
                            w3[:, :, dy + 1, dx + 1] = ws[:, :, ky, kx]
                p = _c3(xv, w3, mut)
                part = p if part is None else part + p
        else:
            n, _, h, wd = xs.shape
            part = xs.new_zeros(n, ws.shape[1], 2 * h, 2 * wd)
            for ph in range(4):
                py, px = ph >> 1, ph & 1
                w3 = ws.new_zeros(ws.shape[1], ws.shape[0], 3, 3)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ky, kx = _s2_bwd(py, dy), _s2_bwd(px, dx)
                        if ky >= 0 and kx >= 0:
                            w3[:, :, dy + 1, dx + 1] = ws[:, :, ky, kx].transpose(0, 1)
                dst = {1: 2, 2: 1}.get(ph, ph) if mut == "phases_swapped" else ph
                part[:, :, (dst >> 1)::2, (dst & 1)::2] = _c3(xs, w3, mut)
        if mut == "drop_last_slice" and s0 == xC - 64:
            part = part * 0
        out = part if out is None else out + part
    if mut == "halves_swapped":                            # the two 64-row halves of every 128-row block
        n, yC, hh, ww = out.shape
        out = out.view(n, yC // 128, 2, 64, hh, ww).flip(2).reshape(n, yC, hh, ww)
    return out


def mask_apply(v, aux, slope, mut=None):
    """v * (aux > 0 ? 1 : slope); what slope 0 zeroes is +0."""
    pos = (aux >= 0) if mut == "mask_ge" else (aux > 0)
    if slope == 0:
        zero = torch.zeros_like(v)
        if mut == "masked_zero_negative":                  # the product 0 * v: -0 for a negative v
            zero = torch.where(v < 0, torch.full_like(v, -0.0), zero)
        return torch.where(pos, v, zero)
    return torch.where(pos, v, v * slope)


def _activate(v, act, slope):
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    return v


def epilogue(c: Case, acc, t, mut=None, step=lambda v: v):
    """The wide kernels' epilogue in their order; step: applied after every fp32 operation (the grid family rounds each to fp32)."""
    act, slope = c.o("act", ACT_NONE), c.o("slope", SLOPE)
    v = acc
    if c.o("bias", 0):
        v = step(v + t["bias"].view(1, -1, 1, 1))
    res = t["res"] if c.o("res", 0) else None
    aux = t["aux"] if c.o("aux", 0) else None
    if mut == "res_before_act" and res is not None:
        v = step(v + res)
    v = step(_activate(v, act, slope))
    out = {}
    if c.o("y_act", 0) and mut != "y_act_after_res":
        out["y_act"] = v
    if mut == "mask_before_res" and aux is not None and res is not None:
        v = step(step(mask_apply(v, aux, slope)) + res)
    else:
        if res is not None and mut != "res_before_act":
            v = step(v + res)
        if c.o("y_act", 0) and mut == "y_act_after_res":
            out["y_act"] = v
        if aux is not None:
            v = step(mask_apply(v, aux, slope, mut))
    out["y"] = v
    if mut == "drop_last_column":
        out = {k: torch.cat([x[..., :-1], x[..., -1:] * 0], -1) for k, x in out.items()}
    return out


def wgrad_def(x, dy, views):
    """Autograd's weight gradient of conv2d (3x3 padding 1, or 4x4 stride 2), summed over the frames."""
    ks = 4 if views == 4 else 3
    w = torch.zeros(dy.shape[1], x.shape[1], ks, ks, dtype=x.dtype, requires_grad=True)
    y = F.conv2d(x, w, stride=2 if views == 4 else 1, padding=1)
    (g,) = torch.autograd.grad(y, w, dy)
    return g


def wgrad_views(x, dy, views, mut=None, rev=False):
    """The weight gradient assembled per (view, cout block, cin slice): a 3x3 correlation of the (view of the) input with dy, the taps a
    view owns scattered into the 4x4 gradient."""
    def corr(xv, d):                                       # gw[co][ci][ty][tx] = sum_p d[co][p] xv[ci][p + (ty - 1, tx - 1)]
        if rev:
            xv, d = xv.flip(0), d.flip(0)
        return F.conv2d(F.pad(xv, (1, 1, 1, 1)).transpose(0, 1), d.transpose(0, 1)).transpose(0, 1)
    if mut == "drop_last_column":
        dy = torch.cat([dy[..., :-1], dy[..., -1:] * 0], -1)
    if views == 1:
        return corr(x, dy)
    gw = x.new_zeros(dy.shape[1], x.shape[1], 4, 4)
    for v in range(4):
        py, px = v >> 1, v & 1
        g3 = corr(x[:, :, py::2, px::2], dy)
        for d_y in (-1, 0, 1):
            for d_x in (-1, 0, 1):
                ky, kx = _s2_fwd(py, d_y), _s2_fwd(px, d_x)
                if ky >= 0 and kx >= 0:
                    if mut == "wgrad_view_wrong_ky":        # the view's two rows of taps change places
                        ky = {1: 3, 3: 1, 0: 2, 2: 0}[ky]
                    gw[:, :, ky, kx] = g3[:, :, d_y + 1, d_x + 1]
    return gw


def up2_def(v):
    return F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)


def up2_adjoint_def(d):
    n, c, h2, w2 = d.shape
    x = torch.zeros(n, c, h2 // 2, w2 // 2, dtype=d.dtype, requires_grad=True)
    (g,) = torch.autograd.grad(up2_def(x), x, d)
    return g


def _axis_up(v, dim, mut):
    n = v.shape[dim]
    idx = torch.arange(n)
    vp, vn = v.index_select(dim, (idx - 1).clamp(min=0)), v.index_select(dim, (idx + 1).clamp(max=n - 1))
    if mut == "up2_no_clamp":                              # the neighbour beyond the border is zero, not the border pixel
        shape = [1] * v.dim()
        shape[dim] = n
        vp = vp * (idx > 0).to(v.dtype).view(shape)
        vn = vn * (idx < n - 1).to(v.dtype).view(shape)
    even, odd = 0.25 * vp + 0.75 * v, 0.75 * v + 0.25 * vn
    return torch.stack([even, odd], dim + 1).flatten(dim, dim + 1)


def up2_sep(v, mut=None):
    """x2 bilinear, align_corners=False, as two separable (1/4, 3/4) passes with clamped neighbours."""
    return _axis_up(_axis_up(v, 3, mut), 2, mut)


def _axis_up_t(d, dim, mut):
    n = d.shape[dim] // 2
    idx = torch.arange(n)
    de, do = d.index_select(dim, 2 * idx), d.index_select(dim, 2 * idx + 1)
    shape = [1] * d.dim()
    shape[dim] = n
    first, last = (idx == 0).to(d.dtype).view(shape), (idx == n - 1).to(d.dtype).view(shape)
    out = 0.75 * de + 0.75 * do + 0.25 * do.index_select(dim, (idx - 1).clamp(min=0)) * (1 - first) + 0.25 * de.index_select(dim, (idx + 1).clamp(max=n - 1)) * (1 - last)
    if mut != "up2_adjoint_unfolded":                      # the output that clamped its missing neighbour onto this pixel carries that weight too
        out = out + 0.25 * de * first + 0.25 * do * last
    return out


def up2_sep_adjoint(d, mut=None):
    return _axis_up_t(_axis_up_t(d, 2, mut), 3, mut)


def pool_route_def(a, dp):
    """route(dp): autograd through F.max_pool2d(a, 2, 2)."""
    a = a.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.max_pool2d(a, 2, 2), a, dp)
    return g


def pool_route_first(a, dp, mut=None):
    """route(dp) with the argmax spelled out: the first maximum of the window in row-major order."""
    n, c, h, w = a.shape
    ho, wo = h // 2, w // 2
    win = torch.stack([a[:, :, q >> 1:2 * ho:2, (q & 1):2 * wo:2] for q in range(4)], -1)
    arg = 3 - win.flip(-1).argmax(-1) if mut == "pool_last_max" else win.argmax(-1)
    out = torch.zeros_like(a)
    for q in range(4):
        out[:, :, q >> 1:2 * ho:2, (q & 1):2 * wo:2] = torch.where(arg == q, dp, torch.zeros_like(dp))
    return out


def _ops(c: Case, t, mut=None, rev=False, assembled=False, step=lambda v: v):
    """The operation of `c` on the tensors t.  assembled: from the launch-shaped pieces (emulation) instead of the definitions."""
    n, h, w = c.shape
    if c.hook == "conv":
        mode = c.o("mode", 0)
        acc = conv_views(t["x"], t["w"], mode, mut, rev) if assembled else conv_def(t["x"], t["w"], mode)
        return epilogue(c, step(acc), t, mut, step)
    if c.hook == "wgrad":
        g = wgrad_views(t["x"], t["dy"], c.o("views"), mut, rev) if assembled else wgrad_def(t["x"], t["dy"], c.o("views"))
        if mut == "wgrad_empty_part_unwritten" and c.dtype == "bf16":
            npairs = (c.o("xC") // 64) * (c.o("dyC") // 64) * c.o("views")
            g = g + SENTINEL * max(pair_ksplit(npairs, tiles_of(c.shape)) - tiles_of(c.shape), 0)
        return dict(gw=step(g) if mut == "wgrad_overwrites" else step(t["gw0"] + step(g)))
    slope = c.o("slope", SLOPE)
    if c.hook == "up2_fwd":
        v = step(t["a"] + t["b"]) if c.o("b", 0) else t["a"]
        return dict(out=up2_sep(v, mut) if assembled else up2_def(v))
    if c.hook == "up2_bwd":
        din = up2_sep_adjoint(t["dout"], mut) if assembled else up2_adjoint_def(t["dout"])
        out = dict(dmask=step(mask_apply(din, t["m"], slope, mut)))
        if c.o("din", 1):
            out["din"] = din
        return out
    if c.hook == "mask":
        return dict(out=step(mask_apply(t["g"], t["m"], slope, mut)))
    if c.hook == "pool_fwd":
        return dict(out=F.max_pool2d(t["a"], 2, 2))
    if c.hook == "pool_bwd":
        route = pool_route_first(t["a"], t["dp"], mut) if assembled else pool_route_def(t["a"], t["dp"])
        pos = t["a"] > 0
        if mut == "pool_mask_skipped_on_dropped_row":
            pos = pos.clone()
            pos[:, :, 2 * (h // 2):, :] = True
            pos[:, :, :, 2 * (w // 2):] = True
        return dict(g=torch.where(pos, step(t["g"] + route), torch.zeros_like(route)))
    if c.hook == "tap":
        d = t["s"] - t["h"]
        sums = d.abs().sum(dim=(1, 2, 3), dtype=torch.float64)
        if mut == "tap_padding_counted":                   # a padding pixel holds NaN
            sums = sums + float("nan")
        out = dict(sums=sums)
        if c.o("grad", 1):
            sg = torch.sign(d)
            if mut == "tap_sign0_scale":
                sg = torch.where(d == 0, torch.ones_like(sg), sg)
            out["g"] = c.o("scale", 0.5) * sg
        return out
    raise KeyError(c.hook)


def applicable(c: Case, mut):
    """Whether the mutation changes anything the operation of `c` computes (at its shape)."""
    n, h, w = c.shape
    hk = c.hook
    mode = c.o("mode", 0)
    yC = (c.o("cin") if mode >= 2 else c.o("cout")) if hk == "conv" else 0
    if mut == "views_swapped":
        return hk == "conv" and mode == 1
    if mut == "phases_swapped":
        return hk == "conv" and mode == 3
    if mut == "tap_mirrored":
        return hk == "conv" and mode in (1, 3)
    if mut == "drop_last_slice":
        return hk == "conv"
    if mut == "halves_swapped":
        return hk == "conv" and yC % 128 == 0
    if mut == "ksplit_half_dropped":
        return hk == "conv" and (yC // 64) % 2 == 1
    if mut == "res_before_act":
        return hk == "conv" and bool(c.o("res", 0)) and c.o("act", 0) != ACT_NONE
    if mut == "y_act_after_res":
        return hk == "conv" and bool(c.o("res", 0)) and bool(c.o("y_act", 0))
    if mut == "mask_before_res":
        return hk == "conv" and bool(c.o("res", 0)) and bool(c.o("aux", 0))
    masked = (hk == "conv" and bool(c.o("aux", 0))) or hk in ("up2_bwd", "mask")
    if mut == "mask_ge":
        return masked
    if mut == "masked_zero_negative":
        return masked and c.o("slope", SLOPE) == 0
    if mut == "drop_last_column":
        return hk in ("conv", "wgrad")
    if mut == "halo_reads_beyond_w":
        return hk == "conv"
    if mut == "up2_no_clamp":
        return hk == "up2_fwd"
    if mut == "up2_adjoint_unfolded":
        return hk == "up2_bwd"
    if mut == "wgrad_view_wrong_ky":
        return hk == "wgrad" and c.o("views") == 4
    if mut == "wgrad_overwrites":
        return hk == "wgrad"
    if mut == "wgrad_empty_part_unwritten":
        if hk != "wgrad" or c.dtype != "bf16":
            return False
        npairs = (c.o("xC") // 64) * (c.o("dyC") // 64) * c.o("views")
        return pair_ksplit(npairs, tiles_of(c.shape)) > tiles_of(c.shape)
    if mut == "pool_last_max":
        return hk == "pool_bwd"
    if mut == "pool_mask_skipped_on_dropped_row":
        return hk == "pool_bwd" and (h % 2 == 1 or w % 2 == 1)
    if mut == "tap_sign0_scale":
        return hk == "tap" and bool(c.o("grad", 1))
    if mut == "tap_padding_counted":
        return hk == "tap" and w % 32 != 0
    raise KeyError(mut)


# --------------------------------------------------------------------------------------------------------------------
# the bound
# --------------------------------------------------------------------------------------------------------------------
def terms(c: Case):
    n, h, w = c.shape
    if c.hook == "conv":
        mode = c.o("mode", 0)
        k = (4 if mode in (1, 3) else 9) * (c.o("cout") if mode >= 2 else c.o("cin"))
        return dict(y=k, y_act=k)
    return {"wgrad": dict(gw=n * h * w), "up2_fwd": dict(out=18 if c.o("b", 0) else 9), "up2_bwd": dict(din=16, dmask=16), "mask": dict(out=1),
            "pool_fwd": dict(out=0), "pool_bwd": dict(g=2), "tap": dict(sums=8, g=0)}[c.hook]


def bf16_outputs(c: Case):
    if c.dtype != "bf16":
        return ()
    return {"conv": ("y", "y_act"), "up2_fwd": ("out",), "up2_bwd": ("din", "dmask"), "mask": ("out",), "pool_fwd": ("out",), "pool_bwd": ("g",),
            "tap": ("g",)}.get(c.hook, ())


def _core(c: Case):
    return Case(c.hook, c.shape, "any", _key(c))


def _linear(c: Case):
    o = dict(c.opts)
    if c.hook == "conv":
        o["act"] = ACT_NONE
    return Case(c.hook, c.shape, c.dtype, tuple(sorted(o.items())))


def _values_of(c: Case, inp):
    grid = c.o("family", "rand") == "grid"
    step = (lambda v: v.float().double()) if grid else (lambda v: v)
    r = _ops(c, inp, step=step)
    mag = {k: v.abs() for k, v in inp.items()}
    for k in ("aux", "m", "a"):
        if k in inp and c.hook not in ("up2_fwd",):
            mag[k] = inp[k]                                # mask and argmax sources keep their sign
    if c.hook == "tap":
        a = dict(sums=(inp["s"] - inp["h"]).abs().sum(dim=(1, 2, 3)), g=torch.zeros_like(inp["s"]))
    elif c.hook == "pool_fwd":
        a = dict(out=torch.zeros_like(r["out"]))
    else:
        a = _ops(_linear(c), mag)
    if grid:
        for k, v in a.items():
            assert float(v.max()) < 2.0 ** 22, (c.name, k, float(v.max()))      # multiples of 1/4 below 2^22: exact in fp32 in any order
    return r, a


@functools.lru_cache(maxsize=4)
def _values(c: Case):
    return _values_of(c, {k: v.double() for k, v in inputs_of(c).items()})


def reference(c: Case, given=None):
    """(r, A) per output name, fp64.  given: tensors that replace drawn inputs (what an engine stored): not cached."""
    if given:
        return _values_of(_core(c), {k: v.double() for k, v in given.items()})
    return _values(_core(c))


def bounds(c: Case, given=None):
    r, a = reference(c, given)
    grid = c.o("family", "rand") == "grid"
    out = {}
    for k in r:
        acc = torch.zeros_like(a[k]) if grid else 2 * terms(c)[k] * EPS * a[k]
        rnd = U * r[k].abs() if (k in bf16_outputs(c) and not grid and terms(c)[k] > 0) else torch.zeros_like(acc)
        out[k] = (acc, rnd)
    return out


def expected(c: Case, given=None):
    """The fp64 values; grid family: rounded as the build stores them (then the bound is 0)."""
    r, _ = reference(c, given)
    if c.o("family", "rand") == "grid":
        return {k: (bf16_round(v.float()).double() if k in bf16_outputs(c) else (v if k == "sums" else v.float().double())) for k, v in r.items()}
    return r


def emulate(c: Case, mut=None, given=None):
    inp = {k: v.float() for k, v in (given or inputs_of(c)).items()}
    out = _ops(c, inp, mut=mut, rev=True, assembled=True)
    return {k: (bf16_round(v) if k in bf16_outputs(c) else v) for k, v in out.items()}


def zeroed_by_mask(c: Case, given=None):
    """Per output, the elements a slope-0 mask zeroes (None: the case has none)."""
    t = given or inputs_of(c)
    if c.o("slope", SLOPE) != 0:
        return {}
    if c.hook == "conv" and c.o("aux", 0):
        return dict(y=~(t["aux"] > 0))
    if c.hook == "up2_bwd":
        return dict(dmask=~(t["m"] > 0))
    if c.hook == "mask":
        return dict(out=~(t["m"] > 0))
    return {}


def negative_zeros(c: Case, got, given=None):
    """How many elements that a slope-0 mask zeroes came back as -0: the project's rule is +0."""
    return sum(int((torch.signbit(got[k]) & (got[k] == 0) & z).sum()) for k, z in zeroed_by_mask(c, given).items())


def measure(c: Case, got, given=None):
    return T.measure_against(c.name, got, expected(c, given), bounds(c, given))


def check(c: Case, got, label="hip", given=None):
    """Every element of every output inside its bound (grid family: equal), nothing a ReLU mask zeroes -0; prints the worst ratios."""
    m = T.check_against(c.name, got, expected(c, given), bounds(c, given), label, tag="WIDE_RATIO")
    nz = negative_zeros(c, got, given)
    assert nz == 0, (c.name, f"{nz} masked elements are -0")
    return m


def passes(c: Case, got, given=None):
    return all(v[0] <= 1.0 for v in measure(c, got, given).values()) and negative_zeros(c, got, given) == 0


# --------------------------------------------------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------------------------------------------------
def to_pm(t, tdt):
    """(N, C, H, W) -> blocked pixel-major (N, H, ceil(W/32), C/8, 32, 8), padding pixels NaN: index arithmetic only, every bit kept."""
    n, c, h, w = t.shape
    ws = (w + 31) // 32
    buf = torch.full((n, c, h, ws * 32), float("nan"), dtype=torch.float32)
    buf[..., :w] = t
    return buf.view(n, c // 8, 8, h, ws, 32).permute(0, 3, 4, 1, 5, 2).contiguous().to(tdt)


def from_pm(v, w):
    n, h, ws, c8, _, _ = v.shape
    return v.float().permute(0, 3, 5, 1, 2, 4).reshape(n, c8 * 8, h, ws * 32)[..., :w].contiguous()


class PmIn:
    """An input (or an in-place operand) in a NaN-banded buffer."""

    def __init__(self, t, dtype, dev):
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        pm = to_pm(t, tdt)
        self.g = T.Guarded(pm.numel(), tdt, dev, float("nan"))
        self.v = self.g.body.view(pm.shape)
        self.v.copy_(pm.to(dev))
        self.w = t.shape[-1]

    def ptr(self):
        return self.g.body.data_ptr()

    def take(self):
        assert self.g.bands_untouched(), "an in-place operand was written outside its buffer"
        return from_pm(self.v.cpu(), self.w)


class PmOut:
    def __init__(self, n, c, h, w, dtype, dev):
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.shape, self.w = (n, h, (w + 31) // 32, c // 8, 32, 8), w
        self.g = T.Guarded(int(np.prod(self.shape)), tdt, dev, SENTINEL)

    def ptr(self):
        return self.g.body.data_ptr()

    def take(self):
        assert self.g.bands_untouched(), "a pixel-major output was written outside its buffer"
        return from_pm(self.g.body.view(self.shape).cpu(), self.w)


def run_hip(c: Case, dev, given=None):
    """One hook call; dict output name -> fp32 CPU tensor.  A HIP error anywhere in it ends the session."""
    return T.fault_guarded(c, _run_hip, dev, given)


def wpack_elems(dtype, cout, cin, mode):
    """Elements of the weight image (vsr_wide2_pack_elems for bf16, vsr_wide_pack_elems for fp32; the hook refuses a smaller scratch)."""
    s2 = mode in (1, 3)
    if dtype != "bf16":
        return (4 if s2 else 1) * (cout // 64) * (cin // 64) * 9 * 4096
    nsl, rows = (cin if mode < 2 else cout) // 64, (cout if mode < 2 else cin)
    ks = rows % 128 != 0
    steps = ((4 if s2 else 9) + 1) // 2 if ks else (4 if s2 else 9)
    return (rows // (64 if ks else 128)) * (4 if mode == 3 else 1) * nsl * (4 if mode == 1 else 1) * steps * 8192


def grid_of(lib, ncob, out_step, shape, max_wg, num_cus=0):
    """(workgroups per column, columns, tiles) of the conv_wide2 launch (vsr_debug_wide_grid)."""
    import ctypes
    out = (ctypes.c_int * 3)()
    rc = lib.vsr_debug_wide_grid(ncob, out_step, shape[0], shape[1], shape[2], max_wg, num_cus, out)
    assert rc == 0, rc
    return tuple(out)


def _run_hip(c: Case, dev, given):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    inp = given or inputs_of(c)
    n, h, w = c.shape
    dt = VF.DT_BF16 if c.dtype == "bf16" else VF.DT_F32
    tdt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    st = VF._stream()
    P = lambda t: None if t is None else (t.ptr() if hasattr(t, "ptr") else t.data_ptr())
    slope = c.o("slope", SLOPE)
    if c.hook == "conv":
        xC, hx, wx, yC, hy, wy = _in_shape(c)
        cout, cin = c.o("cout"), c.o("cin")
        x = PmIn(inp["x"], c.dtype, dev)
        wt = inp["w"].to(dev).contiguous()
        bias = inp["bias"].to(dev).contiguous() if c.o("bias", 0) else None
        res = PmIn(inp["res"], c.dtype, dev) if c.o("res", 0) else None
        aux = PmIn(inp["aux"], c.dtype, dev) if c.o("aux", 0) else None
        y = PmOut(n, yC, hy, wy, c.dtype, dev)
        ya = PmOut(n, yC, hy, wy, c.dtype, dev) if c.o("y_act", 0) else None
        ne = wpack_elems(c.dtype, cout, cin, c.o("mode", 0))
        wp = T.Guarded(ne, tdt, dev, float("nan"))
        rc = lib.vsr_debug_wide_conv(dt, c.o("mode", 0), cout, cin, P(x), P(wt), P(bias), wp.body.data_ptr(), ne, P(y), c.o("act", ACT_NONE), slope,
                                     P(ya), P(res), P(aux), c.o("max_wg", 0), n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert wp.bands_untouched(), "the weight image was written outside its buffer"
        out = dict(y=y.take())
        if ya:
            out["y_act"] = ya.take()
        return out
    if c.hook == "wgrad":
        x, dy = PmIn(inp["x"], c.dtype, dev), PmIn(inp["dy"], c.dtype, dev)
        gw0 = inp["gw0"]
        gw = T.Guarded(gw0.numel(), torch.float32, dev, SENTINEL)
        gw.body.copy_(gw0.flatten().to(dev))
        nf = 2 * lib.vsr_conv3x3_c64_wgrad_slab_floats()
        slab = T.Guarded(nf, torch.float32, dev, SENTINEL)
        rc = lib.vsr_debug_wide_wgrad(dt, c.o("views"), c.o("xC"), c.o("dyC"), P(x), P(dy), gw.body.data_ptr(), slab.body.data_ptr(), nf, n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert gw.bands_untouched() and slab.bands_untouched(), "a weight gradient or its slabs were written outside their buffers"
        return dict(gw=gw.body.view(gw0.shape).cpu().clone())
    C = c.o("C", 64)
    if c.hook == "up2_fwd":
        a = PmIn(inp["a"], c.dtype, dev)
        b = PmIn(inp["b"], c.dtype, dev) if c.o("b", 0) else None
        out = PmOut(n, C, 2 * h, 2 * w, c.dtype, dev)
        rc = lib.vsr_debug_wide_up2_fwd(dt, P(a), P(b), P(out), n, h, w, C, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(out=out.take())
    if c.hook == "up2_bwd":
        dout, m = PmIn(inp["dout"], c.dtype, dev), PmIn(inp["m"], c.dtype, dev)
        din = PmOut(n, C, h, w, c.dtype, dev) if c.o("din", 1) else None
        dmask = PmOut(n, C, h, w, c.dtype, dev)
        rc = lib.vsr_debug_wide_up2_bwd(dt, P(dout), P(din), P(dmask), P(m), slope, n, h, w, C, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        out = dict(dmask=dmask.take())
        if din:
            out["din"] = din.take()
        return out
    if c.hook == "mask":
        g, m = PmIn(inp["g"], c.dtype, dev), PmIn(inp["m"], c.dtype, dev)
        out = PmOut(n, C, h, w, c.dtype, dev)
        rc = lib.vsr_debug_wide_mask(dt, P(g), P(m), P(out), slope, g.v.numel(), st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(out=out.take())
    if c.hook == "pool_fwd":
        a = PmIn(inp["a"], c.dtype, dev)
        out = PmOut(n, C, h // 2, w // 2, c.dtype, dev)
        rc = lib.vsr_debug_vgg_pool(dt, 0, P(a), None, P(out), n, h, w, C, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(out=out.take())
    if c.hook == "pool_bwd":
        a, g, dp = PmIn(inp["a"], c.dtype, dev), PmIn(inp["g"], c.dtype, dev), PmIn(inp["dp"], c.dtype, dev)
        rc = lib.vsr_debug_vgg_pool(dt, 1, P(a), P(dp), P(g), n, h, w, C, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(g=g.take())
    if c.hook == "tap":
        s, hh = PmIn(inp["s"], c.dtype, dev), PmIn(inp["h"], c.dtype, dev)
        partial = T.Guarded(2 * n * 512, torch.float32, dev, SENTINEL)      # doubles, in fp32 buffers: the bands are compared as 32-bit words
        sums = T.Guarded(2 * n * 5, torch.float32, dev, SENTINEL)
        grad = c.o("grad", 1)
        rc = lib.vsr_debug_vgg_tap(dt, P(s), P(hh), grad, c.o("scale", 0.5), partial.body.data_ptr(), sums.body.data_ptr(), n, h, w, C, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert partial.bands_untouched() and sums.bands_untouched(), "the tap sums were written outside their buffers"
        sm = sums.body.view(torch.float64).view(n, 5).cpu()
        assert bool((sm[:, 1:] == 0).all()), "the other taps' sums of a one-tap call are zero"
        out = dict(sums=sm[:, 0].clone())
        got_h = hh.take()
        if grad:
            out["g"] = got_h
        else:
            assert torch.equal(got_h, inp["h"].float()), "the tap without a gradient wrote over h"
        return out
    raise KeyError(c.hook)


def same_bits(a, b):
    """Bit for bit, key by key (fp32 tensors and the fp64 tap sums)."""
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k].contiguous().flatten().view(torch.uint8), b[k].contiguous().flatten().view(torch.uint8))
               for k in a)


# --------------------------------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------------------------------
def _cv(shape, dtype, family, mode, cin, cout, **o):
    return case("conv", shape, dtype, mode=mode, cin=cin, cout=cout, family=family, **o)


def conv_geometries():
    """(id, options) of every wide-conv geometry the two engines launch; cin -> cout of the LAUNCH is (x channels -> y channels)."""
    g = []
    for ci, co in ((512, 256), (256, 128)):
        g.append((f"m0_leaky_{ci}_{co}", dict(mode=0, cin=ci, cout=co, act=ACT_LEAKY)))
    g.append(("m0_leaky_128_64_yact_res", dict(mode=0, cin=128, cout=64, act=ACT_LEAKY, y_act=1, res=1)))
    for ci, co in ((64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)):
        g.append((f"m0_relu_{ci}_{co}", dict(mode=0, cin=ci, cout=co, act=ACT_RELU, bias=1, slope=0.0)))
    g.append(("m0_bias_512_512", dict(mode=0, cin=512, cout=512, act=ACT_NONE, bias=1, slope=0.0)))
    for ci, co in ((64, 128), (128, 256), (256, 512)):
        g.append((f"m1_leaky_{ci}_{co}", dict(mode=1, cin=ci, cout=co, act=ACT_LEAKY)))
    # data gradients: the launch reads `cout` channels and writes `cin`; the table's a -> b is launch input -> launch output
    for a, b in ((64, 128), (128, 256), (256, 512)):
        g.append((f"m2_plain_{a}_{b}", dict(mode=2, cout=a, cin=b)))
    for a, b in ((128, 64), (128, 128), (256, 128), (256, 256), (512, 256), (512, 512)):
        g.append((f"m2_relumask_{a}_{b}", dict(mode=2, cout=a, cin=b, aux=1, slope=0.0)))
    for a, b in ((512, 256), (256, 128), (128, 64)):
        g.append((f"m3_res_mask_{a}_{b}", dict(mode=3, cout=a, cin=b, res=1, aux=1)))
    return g


MANY_GEOMETRIES = [("m0_64_128", dict(mode=0, cin=64, cout=128, act=ACT_LEAKY)), ("m0_128_128", dict(mode=0, cin=128, cout=128, act=ACT_RELU, bias=1, slope=0.0)),
                   ("m0_128_64_ks", dict(mode=0, cin=128, cout=64, act=ACT_LEAKY, y_act=1, res=1)), ("m1_64_128", dict(mode=1, cin=64, cout=128, act=ACT_LEAKY)),
                   ("m3_128_64_ks", dict(mode=3, cout=128, cin=64, res=1, aux=1))]
WGRAD_GEOMETRIES = [(1, 128, 64), (1, 256, 128), (1, 512, 256), (4, 64, 128), (4, 128, 256), (4, 256, 512)]      # (views, xC, dyC)


def launch_ncob(c: Case):
    """64-channel output blocks and out_step of a conv case's launch."""
    mode = c.o("mode", 0)
    return (c.o("cin") if mode >= 2 else c.o("cout")) // 64, 2 if mode == 3 else 1


def small_cases():
    """One small case per form: what test_wide_host.py dry-runs the criterion and the mutations over."""
    cs = []
    for shape in [(1, 1, 1), (1, 2, 5), (2, 5, 7)]:
        for fam in ("rand", "grid"):
            for dt in ("bf16", "fp32"):
                cs += [_cv(shape, dt, fam, 0, 128, 64, act=ACT_LEAKY, y_act=1, res=1), _cv(shape, dt, fam, 0, 64, 128, act=ACT_RELU, bias=1, slope=0.0),
                       _cv(shape, dt, fam, 1, 64, 128, act=ACT_LEAKY), _cv(shape, dt, fam, 2, 128, 128, aux=1, slope=0.0),
                       _cv(shape, dt, fam, 3, 64, 128, res=1, aux=1),
                       case("wgrad", shape, dt, views=1, xC=128, dyC=64, family=fam), case("wgrad", shape, dt, views=4, xC=64, dyC=128, family=fam),
                       case("up2_fwd", shape, dt, C=16, b=1, family=fam), case("up2_fwd", shape, dt, C=16, b=0, family=fam),
                       case("up2_bwd", shape, dt, C=16, din=1, family=fam), case("up2_bwd", shape, dt, C=16, din=0, slope=0.0, family=fam),
                       case("mask", shape, dt, C=16, family=fam), case("mask", shape, dt, C=16, slope=0.0, family=fam),
                       case("tap", shape, dt, C=16, grad=1, family=fam)]
        for dt in ("bf16", "fp32"):
            hw = (shape[0], shape[1] + 2, shape[2] + 2)
            cs += [case("pool_fwd", hw, dt, C=16, family="grid"), case("pool_bwd", hw, dt, C=16, family="grid")]
    return cs
