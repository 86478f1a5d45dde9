"""Shared by test_hr_tail_host.py and test_hr_tail_gpu.py: the reconstruction tail (the pixel-shuffle layers, conv_last.2 with the
bilinear skip, the planar stems, and their backward) restated in fp64, an elementwise error bound, and the driver of the
``vsr_debug_tail_*`` hooks (csrc/hr_tail_hooks.hip).

* ``reference(case, inp)``: every operation from ``F.conv2d``, ``F.pixel_shuffle`` and ``F.interpolate(mode="bilinear",
  align_corners=False)``; the data and weight gradients are restated as convolutions too (test_hr_tail_host.py pins them at 1e-10 to
  torch autograd on the oracle's ``pixel_shuffle_pack`` / ``conv_last``).  Each output comes with ``A``, the sum of the absolute
  products of its ``K`` terms, from the same code on the operands' magnitudes.  The activation-gradient mask is taken from a GIVEN
  ``aux``: gradient x (aux > 0 ? 1 : slope), torch's LeakyReLU convention.  The phase-plane layout of ``ConvArgs::unshuffle`` is index
  arithmetic: pixel (y, x) lives in plane 2 (y & 1) + (x & 1) at (y >> 1, x >> 1).
* ``emulate(case, inp, mut)``: the same operation in fp32 with another summation order (the reduction axis reversed), rounded to
  bf16 where the bf16 build stores; ``mut`` names one of MUTATIONS, a deliberately wrong variant that the bound has to reject.
* ``check(case, got, ref)``: for every output element, with u = 2^-8,
      bf16 output   |err| <= u |r| + 2 K 2^-24 A          fp32 output   |err| <= 2 K 2^-24 A
  (2: the MFMA's internal summation order is not specified).  The four-launch bf16 pixel-shuffle data gradient rounds three partial
  sums to bf16: + u (|s1| + |s1+s2| + |s1+s2+s3|) from the reference's own partial sums.  The bilinear skip: + 16 2^-24 sum |w_i tap_i|
  and nothing else (it is not part of A; bias and planar residual are, as two of the K terms).
  No element is exempt.  Returns the worst err / bound and the worst share of the accumulation term alone.
* ``run_hip(case, inp, dev)``: one hook call.  Pixel-major operands come from ``to_pixel_major``; the padding pixels (index >= W of a
  row's last 32-pixel segment) of every INPUT are overwritten with NaN; planar inputs sit in NaN-filled buffers (the gaps between
  images included); every output sits between sentinel bands that must come back untouched, planar outputs with sentinel gaps
  between their images.  Output padding pixels are not asserted on.

Operands that a kernel rounds to bf16 (activations, weights, cotangents -- the fp32 dSR too: last2_dgrad and last2_wgrad feed it to the
MFMA as bf16) are drawn bf16-representable, so operand rounding is the identity in both builds.  ``aux`` carries exact +0.0, -0.0 and
the smallest bf16 subnormal of either sign."""
import functools
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -8
EPS = 2.0 ** -24
GUARD = 4096                    # elements on each side of every buffer: a multiple of 4, so 16-byte alignment is kept
SENTINEL = -7.25                # finite, exact in bf16
SLOPE = float(np.float32(0.1))  # the path's LeakyReLU slope as the kernels hold it
SLOPE2 = float(np.float32(0.2)) # another slope (the discriminator's): the hooks' slope argument is what the kernels use
SUBNORMAL = 2.0 ** -133         # the smallest bf16 subnormal

# (N, H, W); tiles are 8 rows x 32 pixels.  (3, 80, 352): 330 tiles, more than one per persistent workgroup
SHAPES = [(1, 1, 1), (1, 8, 32), (2, 13, 37), (1, 3, 66), (1, 9, 31), (1, 17, 100), (3, 80, 352)]
BIG_DGRAD = (4, 168, 790)       # 2100 tiles against last2_dgrad's 2048-workgroup cap
SKIP_SHAPES = [(1, 8, 32), (2, 12, 36), (3, 80, 352)]      # both sizes divide by 4; (2, 12, 36): LR width 9, odd
MUTATIONS = ("drop_last_column", "halo_reads_beyond_w", "tap_mirrored", "phases_swapped", "mask_ge")


def ragged(shape):
    return shape[1] % 8 != 0 or shape[2] % 32 != 0


def sid(shape):
    return "x".join(str(s) for s in shape)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def draw(seed, *shape):
    """uniform(-1, 1), bf16-representable, fp32."""
    g = torch.Generator().manual_seed(int(seed))
    return bf16_round(torch.rand(*shape, generator=g) * 2 - 1)


def draw_aux(seed, n, h, w, c=64):
    """An activation (N, c, H, W): bf16-representable values of both signs with +0.0, -0.0 and +-2^-133 at every pixel's channels
    0..3 of the first and the last column and sprinkled over ~3 % of the rest."""
    a = draw(seed, n, c, h, w)
    g = torch.Generator().manual_seed(int(seed) + 1)
    pick = torch.rand(n, c, h, w, generator=g)
    special = torch.tensor([0.0, -0.0, SUBNORMAL, -SUBNORMAL])
    kind = torch.randint(0, 4, (n, c, h, w), generator=g)
    a = torch.where(pick < 0.03, special[kind], a)
    for col in (0, w - 1):
        a[:, 0:4, :, col] = special.view(1, 4, 1)
    return a


@dataclass(frozen=True)
class Case:
    """hook: last2_fwd | last2_dgrad | planar_c64 | last2_wgrad | unshuffle | ps_dgrad | ps_wgrads.  shape: the layer's input size
    (unshuffle: its output is 2H x 2W).  opts: see make_inputs / run_hip."""
    hook: str
    shape: tuple
    dtype: str = "bf16"
    opts: tuple = ()

    def o(self, key, default=None):
        return dict(self.opts).get(key, default)

    @property
    def name(self):
        return f"{self.hook}[{sid(self.shape)},{self.dtype}" + "".join(f",{k}={v}" for k, v in self.opts) + "]"


def case(hook, shape, dtype="bf16", **opts):
    return Case(hook, tuple(shape), dtype, tuple(sorted(opts.items())))


# --------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def make_inputs(hook, shape, opts=()):
    """CPU fp32 tensors of one (hook, shape); the options that change the operands' shapes are part of the key."""
    n, h, w = shape
    o = dict(opts)
    s = 7000 + 131 * h + 17 * w + n
    if hook == "last2_fwd":
        co = o.get("co", 3)
        d = dict(x=draw(s, n, 64, h, w), w=draw(s + 1, co, 64, 3, 3), bias=torch.randn(co, generator=torch.Generator().manual_seed(s + 2)),
                 pres=torch.randn(n, co, h, w, generator=torch.Generator().manual_seed(s + 3)))
        sc = o.get("scale", 0)
        if sc:
            d["base"] = torch.rand(n, co, h // sc, w // sc, generator=torch.Generator().manual_seed(s + 4))
        return d
    if hook == "last2_dgrad":
        return dict(dsr=draw(s + 10, n, 3, h, w), w=draw(s + 11, 3, 64, 3, 3), aux=draw_aux(s + 12, n, h, w))
    if hook == "planar_c64":
        pc = o.get("pc", 3)
        return dict(src=draw(s + 20, n, pc, h, w), w=draw(s + 21, 64, pc, 3, 3), bias=torch.randn(64, generator=torch.Generator().manual_seed(s + 22)),
                    aux=draw_aux(s + 23, n, h, w))
    if hook == "last2_wgrad":
        return dict(x=draw(s + 30, n, 64, h, w), dy=draw(s + 31, n, 3, h, w))
    if hook == "unshuffle":
        return dict(x=draw(s + 40, n, 64, 2 * h, 2 * w), w=draw(s + 41, 64, 64, 3, 3), bias=torch.randn(64, generator=torch.Generator().manual_seed(s + 42)))
    if hook == "ps_dgrad":
        return dict(dy=draw(s + 50, n, 64, 2 * h, 2 * w), w=draw(s + 51, 256, 64, 3, 3), aux=draw_aux(s + 52, n, h, w))
    if hook == "ps_wgrads":
        return dict(x=draw(s + 60, n, 64, h, w), dy=draw(s + 61, n, 64, 2 * h, 2 * w))
    raise KeyError(hook)


def inputs_of(c: Case):
    key = tuple((k, v) for k, v in c.opts if k in ("co", "scale", "pc"))
    return make_inputs(c.hook, c.shape, key)


# --------------------------------------------------------------------------------------------------------------------
# the operations.  Everything below runs in the dtype of its operands; `rev` reverses the reduction axis (another summation order);
# `mut` is one of MUTATIONS
# --------------------------------------------------------------------------------------------------------------------
def _conv(x, w, mut=None, rev=False):
    """3x3 'same' convolution of x (N, Ci, H, W) with w (Co, Ci, 3, 3)."""
    if mut == "tap_mirrored":                              # taps (1, 0) and (1, 2) change places
        w = w.clone()
        w[:, :, 1, 0], w[:, :, 1, 2] = w[:, :, 1, 2].clone(), w[:, :, 1, 0].clone()
    if rev:
        x, w = x.flip(1), w.flip(1)
    if mut == "halo_reads_beyond_w":                       # the column right of the image holds something, not zero
        xp = F.pad(x, (1, 1, 1, 1))
        xp[:, :, 1:-1, -1] = 0.5
        return F.conv2d(xp, w)
    return F.conv2d(x, w, padding=1)


def _dgrad_w(w):
    """The weights of the data gradient as a forward convolution: roles swapped, taps flipped."""
    return w.transpose(0, 1).flip(2, 3)


def mask_factor(aux, slope, mut=None):
    pos = (aux >= 0) if mut == "mask_ge" else (aux > 0)
    return torch.where(pos, torch.ones_like(aux), torch.full_like(aux, slope))


def unshuffle_planes(y, mut=None):
    """(N, C, H, W), H and W even -> (4, N, C, H/2, W/2): plane z = 2 (y & 1) + (x & 1) holds pixel (y >> 1, x >> 1)."""
    order = (0, 2, 1, 3) if mut == "phases_swapped" else (0, 1, 2, 3)
    return torch.stack([y[:, :, (z >> 1)::2, (z & 1)::2] for z in order])


def shuffle_planes(p):
    """The inverse of unshuffle_planes."""
    _, n, c, h, w = p.shape
    y = p.new_zeros(n, c, 2 * h, 2 * w)
    for z in range(4):
        y[:, :, (z >> 1)::2, (z & 1)::2] = p[z]
    return y


def _wgrad(x, dy, mut=None, rev=False):
    """gw[co][ci][ky][kx] = sum_p dy[co][p] x[ci][p + (ky - 1, kx - 1)], gb[co] = sum_p dy[co][p]: a convolution of x^T with dy^T."""
    if mut == "drop_last_column":
        dy = dy.clone()
        dy[..., -1] = 0
    dy0 = dy
    if rev:
        x, dy = x.flip(0, 3), dy.flip(0, 3)
    gw = F.conv2d(F.pad(x, (1, 1, 1, 1)).transpose(0, 1), dy.transpose(0, 1)).transpose(0, 1)      # (Co, Ci, 3, 3)
    if rev:
        gw = gw.flip(3)
    if mut == "halo_reads_beyond_w":
        gw = gw.clone()
        gw[:, :, :, 2] += 0.5 * dy0[..., -1].sum(dim=(0, 2)).view(-1, 1, 1)
    if mut == "tap_mirrored":
        gw = gw.clone()
        gw[:, :, 1, 0], gw[:, :, 1, 2] = gw[:, :, 1, 2].clone(), gw[:, :, 1, 0].clone()
    return gw, dy.sum(dim=(0, 2, 3))


def applicable(c, mut):
    """Whether the mutation changes anything the operation of `c` computes."""
    if mut == "drop_last_column":
        return c.hook in ("last2_wgrad", "ps_wgrads")
    if mut == "phases_swapped":
        return c.hook in ("unshuffle", "ps_dgrad", "ps_wgrads")
    if mut == "mask_ge":
        return c.hook in ("last2_dgrad", "planar_c64", "ps_dgrad") and c.o("mask", "aux" if c.hook == "last2_dgrad" else "none") != "none"
    if mut == "tap_mirrored":                              # a 1-pixel-wide image meets the centre column of the taps only
        return c.shape[2] * (2 if c.hook == "unshuffle" else 1) >= 2
    return True


def _ops(c: Case, t, mut=None, rev=False, partials=None):
    """The operation of `c` on the tensors t (any dtype).  dict: output name -> tensor.  partials (ps_dgrad): a function applied to each
    running phase sum (the bf16 build stores them), and the running sums are returned as `_s1.._s3`."""
    n, h, w = c.shape
    slope = c.o("slope", SLOPE)
    if c.hook == "last2_fwd":
        y = _conv(t["x"], t["w"], mut, rev)
        if c.o("bias", True):
            y = y + t["bias"].view(1, -1, 1, 1)
        if c.o("pres", False):
            y = y + t["pres"]
        if c.o("scale", 0):
            y = y + F.interpolate(t["base"], scale_factor=c.o("scale"), mode="bilinear", align_corners=False)
        return dict(y=y)
    if c.hook == "last2_dgrad":
        dx = _conv(t["dsr"], _dgrad_w(t["w"]), mut, rev)
        if c.o("mask", "aux") != "none":
            dx = dx * mask_factor(t["aux"], 0.0 if c.o("mode", 2) == 1 else slope, mut)
        return dict(dx=dx)
    if c.hook == "planar_c64":
        y = _conv(t["src"], t["w"], mut, rev)
        if c.o("bias", True):
            y = y + t["bias"].view(1, -1, 1, 1)
        if c.o("act", 2) == 2:
            y = torch.where(y > 0, y, y * slope)
        if c.o("mask", "none") != "none":
            y = y * mask_factor(t["aux"], slope, mut)
        return dict(y=y)
    if c.hook == "last2_wgrad":
        pc = c.o("pc", 3)
        gw, gb = _wgrad(t["x"], t["dy"][:, :pc], mut, rev)
        return dict(gw=gw, gb=gb)
    if c.hook == "unshuffle":
        wt = _dgrad_w(t["w"]) if c.o("mode", 0) == 1 else t["w"]
        y = _conv(t["x"], wt, mut, rev)
        if c.o("bias", True):
            y = y + t["bias"].view(1, -1, 1, 1)
        return dict(planes=unshuffle_planes(y, mut))
    if c.hook == "ps_dgrad":
        # PixelShuffle(2): out[c, 2y+i, 2x+j] = conv[4c + 2i + j, y, x]: phase z = 2i + j uses the conv's rows 4c + z
        order = (0, 2, 1, 3) if mut == "phases_swapped" else (0, 1, 2, 3)
        out, s = {}, None
        for k, z in enumerate(order):
            part = _conv(t["dy"][:, :, (k >> 1)::2, (k & 1)::2], _dgrad_w(t["w"][z::4]), mut, rev)
            s = part if s is None else s + part
            if k < 3:
                if partials is not None:
                    s = partials(s)
                out[f"_s{k + 1}"] = s
        if c.o("mask", "none") != "none":
            s = s * mask_factor(t["aux"], slope, mut)
        out["dx"] = s
        return out
    if c.hook == "ps_wgrads":
        gw = t["x"].new_zeros(256, 64, 3, 3)
        gb = t["x"].new_zeros(256)
        order = (0, 2, 1, 3) if mut == "phases_swapped" else (0, 1, 2, 3)
        for k, z in enumerate(order):
            gw[z::4], gb[z::4] = _wgrad(t["x"], t["dy"][:, :, (k >> 1)::2, (k & 1)::2], mut, rev)
        return dict(gw=gw, gb=gb)
    raise KeyError(c.hook)


def terms(c: Case):
    """K per output: the products (and bias / residual / activation / mask steps) summed into one element."""
    n, h, w = c.shape
    return {"last2_fwd": dict(y=576 + 2), "last2_dgrad": dict(dx=27 + 1), "planar_c64": dict(y=9 * c.o("pc", 3) + 3),
            "last2_wgrad": dict(gw=n * h * w, gb=n * h * w), "unshuffle": dict(planes=576 + 1), "ps_dgrad": dict(dx=4 * 576 + 1),
            "ps_wgrads": dict(gw=n * h * w, gb=n * h * w)}[c.hook]


def bf16_outputs(c: Case):
    """The outputs the build of `c` stores as bf16."""
    if c.dtype != "bf16":
        return ()
    return {"last2_dgrad": ("dx",), "planar_c64": ("y",), "unshuffle": ("planes",), "ps_dgrad": ("dx",)}.get(c.hook, ())


_LAYOUT_OPTS = ("dy_planes", "dx_planes", "nstride_mul", "gap", "misalign")


def _core(c: Case):
    """The case without what changes only the operands' placement (and the two mask sources, which carry the same mask)."""
    o = {k: ("aux" if k == "mask" and v == "bits" else v) for k, v in c.opts if k not in _LAYOUT_OPTS}
    return Case(c.hook, c.shape, "any", tuple(sorted(o.items())))


@functools.lru_cache(maxsize=6)
def _values(c: Case):
    inp = {k: v.double() for k, v in inputs_of(c).items()}
    r = _ops(c, inp)
    mag = {k: v.abs() for k, v in inp.items()}
    if "aux" in inp:
        mag["aux"] = inp["aux"]                            # the mask is a factor, not a term: it keeps its sign test
    ca = c
    if c.hook == "planar_c64" and c.o("act", 2) == 2:
        # LeakyReLU is 1-Lipschitz: the error of its argument passes at most unchanged, whichever side of zero either evaluation is on
        lin = dict(c.opts)
        lin["act"] = 0
        ca = Case(c.hook, c.shape, c.dtype, tuple(sorted(lin.items())))
    if c.hook == "last2_fwd" and c.o("scale", 0):
        # the skip is not one of the K accumulated terms: it has its own term (16 2^-24 sum |w_i tap_i|) and stays out of A
        ns = dict(c.opts)
        ns["scale"] = 0
        ca = Case(c.hook, c.shape, c.dtype, tuple(sorted(ns.items())))
    a = _ops(ca, mag)
    bil = None
    if c.hook == "last2_fwd" and c.o("scale", 0):
        bil = F.interpolate(mag["base"], scale_factor=c.o("scale"), mode="bilinear", align_corners=False)
    return r, a, bil


def reference(c: Case):
    """(r, A, extra): fp64 values, absolute-product sums and the additional terms of the bound, per output name.  Computed once per
    operation and shape: the dtype and the operands' placement change the bound or nothing."""
    r, a, bil = _values(_core(c))
    extra = {}
    if bil is not None:
        extra["y"] = 16 * EPS * bil
    if c.hook == "ps_dgrad" and c.dtype == "bf16":
        e = U * (r["_s1"].abs() + r["_s2"].abs() + r["_s3"].abs())
        if c.o("mask", "none") != "none":
            e = e * mask_factor(inputs_of(c)["aux"].double(), c.o("slope", SLOPE))
        extra["dx"] = e
    keys = [k for k in r if not k.startswith("_")]
    return {k: r[k] for k in keys}, {k: a[k] for k in keys}, extra


def emulate(c: Case, mut=None):
    """fp32 arithmetic on the same operands in another summation order; rounded to bf16 where the build of `c` stores."""
    inp = {k: v.float() for k, v in inputs_of(c).items()}
    store = bf16_round if c.dtype == "bf16" else (lambda v: v)
    out = _ops(c, inp, mut=mut, rev=True, partials=store if c.hook == "ps_dgrad" else None)
    return {k: (bf16_round(v) if k in bf16_outputs(c) else v) for k, v in out.items() if not k.startswith("_")}


def bounds(c: Case):
    r, a, extra = reference(c)
    out = {}
    for k, kk in terms(c).items():
        acc = 2 * kk * EPS * a[k]
        rnd = (U * r[k].abs() if k in bf16_outputs(c) else torch.zeros_like(acc)) + extra.get(k, 0)
        out[k] = (acc, rnd)
    return out


def measure(c: Case, got):
    """dict name -> (worst err / bound, worst (err - rounding terms) / accumulation term, index of the worst element).  An element whose
    bound is 0 has to be exact (ratio 0 or inf).  NaN anywhere in `got` gives inf."""
    return measure_against(c.name, got, reference(c)[0], bounds(c))


def measure_against(name, got, r, bnds):
    """measure() on explicit references: r[k] the fp64 values, bnds[k] = (accumulation term, rounding terms) (tests/trunk_common.py too)."""
    res = {}
    for k, (acc, rnd) in bnds.items():
        g = got[k].double()
        assert g.shape == r[k].shape, (name, k, tuple(g.shape), tuple(r[k].shape))
        err = (g - r[k]).abs()
        err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
        b = acc + rnd
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b)      # (a zero bound: exact or inf)
        over = (err - rnd).clamp_min(0)
        acc_ratio = torch.where(over == 0, torch.zeros_like(over), over / acc.clamp_min(1e-300))
        i = int(ratio.argmax())
        res[k] = (float(ratio.flatten()[i]), float(acc_ratio.max()), tuple(int(v) for v in np.unravel_index(i, ratio.shape)))
    return res


def describe_failures(c: Case, got, limit=6):
    """Which elements are outside their bound: per output the count and the first few (index, got, reference, bound)."""
    return describe_failures_against(got, reference(c)[0], bounds(c), limit)


def describe_failures_against(got, r, bnds, limit=6):
    lines = []
    for k, (acc, rnd) in bnds.items():
        g = got[k].double()
        bad = ~((g - r[k]).abs() <= acc + rnd)
        idx = bad.nonzero()
        if len(idx):
            lines.append(f"{k}: {len(idx)} of {bad.numel()} elements outside the bound; first: " + "; ".join(
                f"{tuple(int(v) for v in i)} got {float(g[tuple(i)]):.6g} ref {float(r[k][tuple(i)]):.6g} bound {float((acc + rnd)[tuple(i)]):.3g}" for i in idx[:limit]))
    return lines


def check(c: Case, got, label="hip"):
    """Every element of every output inside its bound; prints the worst ratios; returns measure()'s dict."""
    return check_against(c.name, got, reference(c)[0], bounds(c), label)


def check_against(name, got, r, bnds, label="hip", tag="HR_TAIL_RATIO"):
    m = measure_against(name, got, r, bnds)
    for k, (ratio, acc_ratio, idx) in m.items():
        print(f"{tag} {label} {name} {k}: worst err/bound {ratio:.3f} at {idx}, accumulation share {acc_ratio:.3f}")
    bad = {k: v for k, v in m.items() if not v[0] <= 1.0}
    assert not bad, (name, describe_failures_against(got, r, bnds))
    return m


def passes(c: Case, got):
    return all(v[0] <= 1.0 for v in measure(c, got).values())


# --------------------------------------------------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _sync():
    """A HIP error here is a GPU fault: nothing more is started on the card in this session."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit(f"GPU fault in a reconstruction-tail hook: {e}", returncode=3)


class Guarded:
    """A flat buffer of `numel` elements between two GUARD bands, all `fill`.  untouched(): the bands still hold `fill` bit for bit."""

    def __init__(self, numel, dtype, dev, fill, offset=0):
        self.buf = torch.full((numel + 2 * GUARD + offset,), fill, dtype=dtype, device=dev)
        self.fill, self.numel, self.lo = fill, numel, GUARD + offset
        self.body = self.buf[self.lo:self.lo + numel]

    def bands_untouched(self):
        want = torch.full_like(self.buf, self.fill)
        return (torch.equal(_bits(self.buf[:self.lo]), _bits(want[:self.lo])) and
                torch.equal(_bits(self.buf[self.lo + self.numel:]), _bits(want[self.lo + self.numel:])))

    def all_fill(self):
        return torch.equal(_bits(self.buf), _bits(torch.full_like(self.buf, self.fill)))


class Planar:
    """(N, C, H, W) fp32 with `nstride` floats between images, inside a Guarded buffer: the gaps between images hold `fill` too.
    offset: floats by which the tensor starts off its 16-byte alignment."""

    def __init__(self, n, c, h, w, nstride, dev, fill, data=None, offset=0):
        assert nstride >= c * h * w
        self.g = Guarded((n - 1) * nstride + c * h * w, torch.float32, dev, fill, offset)
        self.view = self.g.body.as_strided((n, c, h, w), (nstride, h * w, w, 1))
        self.nstride = nstride
        if data is not None:
            self.view.copy_(data.to(dev))

    def take(self):
        """The tensor's values (CPU); afterwards the whole buffer must hold the fill again."""
        out = self.view.cpu().clone()
        self.view.fill_(self.g.fill)
        assert self.g.all_fill(), "a planar output was written outside its images"
        return out


def pm_input(t, dtype, dev):
    """(N, C, H, W) CPU fp32, C = 16, 32 or 64 -> the blocked pixel-major tensor in a NaN-banded buffer, padding pixels NaN."""
    from vsrlab_amd import functional as VF
    pm = VF.to_pixel_major(t.to(dev), VF.DT_BF16 if dtype == "bf16" else VF.DT_F32, t.shape[1])
    g = Guarded(pm.numel(), pm.dtype, dev, float("nan"))
    v = g.body.view(pm.shape)
    v.copy_(pm)
    r = t.shape[-1] % 32
    if r:
        v[:, :, -1, :, r:, :] = float("nan")
    v.pm_w = t.shape[-1]
    return v


def pm_planes_input(t, dtype, dev):
    """(N, 64, 2H, 2W) -> its four phase planes, each a whole pixel-major tensor, back to back."""
    planes = unshuffle_planes(t)
    pms = [pm_input(planes[z], dtype, dev) for z in range(4)]
    out = torch.stack(pms).contiguous()
    return out


class PmOutput:
    def __init__(self, n, h, w, dtype, dev, planes=1, c=64):
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        shape = (n, h, (w + 31) // 32, c // 8, 32, 8)
        numel = planes * int(np.prod(shape))
        self.g = Guarded(numel, tdt, dev, SENTINEL)
        self.shape, self.planes, self.w, self.c = shape, planes, w, c

    def ptr(self):
        return self.g.body.data_ptr()

    def take(self):
        from vsrlab_amd import functional as VF
        assert self.g.bands_untouched(), "a pixel-major output was written outside its buffer"
        outs = []
        for v in self.g.body.view(self.planes, *self.shape):
            v.pm_w = self.w
            outs.append(VF.from_pixel_major(v, self.c).cpu())
        return outs[0] if self.planes == 1 else torch.stack(outs)


def fault_guarded(c: Case, driver, *args):
    """driver(c, *args), the one fault guard of the five per-launch drivers (this file's, trunk_common's, spynet_common's,
    wide_common's and flow_warp_common's): a HIP error anywhere in it ends the session, so nothing more is started on a card that has faulted."""
    try:
        return driver(c, *args)
    except RuntimeError as e:
        if "HIP" in str(e) or "hip" in str(e):
            import pytest
            pytest.exit(f"GPU fault in {c.name}: {e}", returncode=3)
        raise


def run_hip(c: Case, dev):
    """One hook call on the inputs of `c`; dict output name -> fp32 CPU tensor (the layout of reference()).  A HIP error ends the
    session (fault_guarded)."""
    return fault_guarded(c, _run_hip, dev)


def _run_hip(c: Case, dev):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    inp = inputs_of(c)
    n, h, w = c.shape
    dt = VF.DT_BF16 if c.dtype == "bf16" else VF.DT_F32
    tdt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    st, nan = VF._stream(), float("nan")
    P = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    slope = c.o("slope", SLOPE)
    mask_src = {"none": 0, "aux": 1, "bits": 2}[c.o("mask", "aux" if c.hook == "last2_dgrad" else "none")]
    dev_w = inp["w"].to(dev).contiguous() if "w" in inp else None
    keep = []                                              # scratch tensors live until the call has been synchronised

    def held(t):
        keep.append(t)
        return t

    scratch = lambda numel, dtype=tdt: held(torch.full((numel,), 1.0, dtype=dtype, device=dev))
    slab = lambda: held(torch.empty(lib.vsr_conv3x3_c64_wgrad_slab_floats(), dtype=torch.float32, device=dev))
    sign = lambda: held(torch.full((n * ((h + 7) // 8) * ((w + 31) // 32) * 512,), -1, dtype=torch.int32, device=dev))

    if c.hook == "last2_fwd":
        co, sc = c.o("co", 3), c.o("scale", 0)
        x = pm_input(inp["x"], c.dtype, dev)
        ns = co * h * w + c.o("gap", 8)
        y = Planar(n, co, h, w, ns, dev, SENTINEL)
        pres = Planar(n, co, h, w, ns, dev, nan, inp["pres"]) if c.o("pres", False) else None
        base = Planar(n, co, h // sc, w // sc, co * (h // sc) * (w // sc) + 4, dev, nan, inp["base"]) if sc else None
        bias = inp["bias"].to(dev) if c.o("bias", True) else None
        rc = lib.vsr_debug_tail_last2_fwd(dt, P(x), P(dev_w), P(bias), P(scratch(9 * 32 * 64)), P(scratch(64, torch.float32)), P(y.view), ns,
                                          P(pres.view) if pres else None, P(base.view) if base else None, base.nstride if base else 0,
                                          h // sc if sc else 0, w // sc if sc else 0, sc, co, n, h, w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        return dict(y=y.take())
    if c.hook == "last2_dgrad":
        ns = c.o("nstride_mul", 1) * 3 * h * w
        dsr = Planar(n, 3, h, w, ns, dev, nan, inp["dsr"])
        aux = pm_input(inp["aux"], "bf16", dev) if mask_src else None
        dx = PmOutput(n, h, w, "bf16", dev)
        rc = lib.vsr_debug_tail_last2_dgrad(P(dsr.view), ns, P(dev_w), P(aux), mask_src, P(sign()) if mask_src == 2 else None, c.o("mode", 2),
                                            slope, dx.ptr(), n, h, w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        return dict(dx=dx.take())
    if c.hook == "planar_c64":
        pc = c.o("pc", 3)
        ns = pc * h * w + c.o("gap", 0)
        src = Planar(n, pc, h, w, ns, dev, nan, inp["src"])
        aux = pm_input(inp["aux"], c.dtype, dev) if mask_src else None
        bias = inp["bias"].to(dev) if c.o("bias", True) else None
        y = PmOutput(n, h, w, c.dtype, dev)
        rc = lib.vsr_debug_tail_planar_c64(dt, P(src.view), ns, pc, P(dev_w), P(bias), P(scratch(9 * 64 * 16)), y.ptr(), c.o("act", 2), slope,
                                           P(aux), 2 if mask_src else 0, n, h, w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        return dict(y=y.take())
    if c.hook == "last2_wgrad":
        pc = c.o("pc", 3)
        ns = c.o("nstride_mul", 1) * 3 * h * w
        # pc planes of the cotangent exist; what lies behind them (the rest of the image stride, the band) is NaN
        dy = Planar(n, pc, h, w, ns, dev, nan, inp["dy"][:, :pc], offset=c.o("misalign", 0))
        x = pm_input(inp["x"], c.dtype, dev)
        gw, gb = Guarded(pc * 576, torch.float32, dev, SENTINEL), Guarded(pc, torch.float32, dev, SENTINEL)
        rc = lib.vsr_debug_tail_last2_wgrad(dt, P(x), P(dy.view), ns, pc, P(gw.body), P(gb.body), P(slab()), n, h, w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        assert gw.bands_untouched() and gb.bands_untouched(), "a weight gradient was written outside its tensor"
        return dict(gw=gw.body.view(pc, 64, 3, 3).cpu().clone(), gb=gb.body.cpu().clone())
    if c.hook == "unshuffle":
        x = pm_input(inp["x"], c.dtype, dev)
        bias = inp["bias"].to(dev) if c.o("bias", True) else None
        y = PmOutput(n, h, w, c.dtype, dev, planes=4)
        rc = lib.vsr_debug_tail_conv_unshuffle(dt, P(x), P(dev_w), P(bias), c.o("mode", 0), P(scratch(9 * 64 * 64)), y.ptr(), n, 2 * h, 2 * w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        return dict(planes=y.take())
    if c.hook == "ps_dgrad":
        dyp, dxp = c.o("dy_planes", 0), c.o("dx_planes", 0)
        dy = pm_planes_input(inp["dy"], c.dtype, dev) if dyp else pm_input(inp["dy"], c.dtype, dev)
        aux = pm_input(inp["aux"], c.dtype, dev) if mask_src else None
        dx = PmOutput(n, h // 2, w // 2, c.dtype, dev, planes=4) if dxp else PmOutput(n, h, w, c.dtype, dev)
        rc = lib.vsr_debug_tail_ps_dgrad(dt, P(dy), P(dev_w), P(scratch(4 * 9 * 64 * 64)), dx.ptr(), P(aux), 2 if mask_src else 0, mask_src,
                                         P(sign()) if mask_src == 2 else None, dyp, dxp, n, h, w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        out = dx.take()
        return dict(dx=shuffle_planes(out) if dxp else out)
    if c.hook == "ps_wgrads":
        dyp = c.o("dy_planes", 0)
        x = pm_input(inp["x"], c.dtype, dev)
        dy = pm_planes_input(inp["dy"], c.dtype, dev) if dyp else pm_input(inp["dy"], c.dtype, dev)
        gw, gb = Guarded(256 * 576, torch.float32, dev, SENTINEL), Guarded(256, torch.float32, dev, SENTINEL)
        rc = lib.vsr_debug_tail_ps_wgrads(dt, P(x), P(dy), dyp, P(gw.body), P(gb.body), P(slab()), n, h, w, st)
        assert rc == 0, (c.name, rc)
        _sync()
        assert gw.bands_untouched() and gb.bands_untouched(), "a weight gradient was written outside its tensor"
        return dict(gw=gw.body.view(256, 64, 3, 3).cpu().clone(), gb=gb.body.cpu().clone())
    raise KeyError(c.hook)


def same_bits(a, b):
    return all(torch.equal(_bits(a[k].contiguous()), _bits(b[k].contiguous())) for k in a)


# --------------------------------------------------------------------------------------------------------------------
# the cases of test_hr_tail_gpu.py that are compared with the reference (test_hr_tail_host.py dry-runs the criterion over them)
# --------------------------------------------------------------------------------------------------------------------
def fwd_cases(shape, dtype):
    """conv_last.2 forward: cout_real 1..4, with / without bias and planar residual, a destination image stride with and without a gap."""
    return [case("last2_fwd", shape, dtype, co=3), case("last2_fwd", shape, dtype, co=1, bias=False, pres=True, gap=0),
            case("last2_fwd", shape, dtype, co=4, pres=True), case("last2_fwd", shape, dtype, co=2, gap=4 * shape[1] * shape[2])]


def skip_cases(shape, dtype):
    """... with the bilinear skip: x4 on the 3-channel fast path and on the general path (a residual as well), x2."""
    return [case("last2_fwd", shape, dtype, co=3, scale=4), case("last2_fwd", shape, dtype, co=3, scale=4, pres=True),
            case("last2_fwd", shape, dtype, co=3, scale=2), case("last2_fwd", shape, dtype, co=1, scale=2, bias=False)]


def dgrad_cases(shape):
    """conv_last.2's data gradient (bf16 only): no mask, LeakyReLU mask from aux and from its sign bits (slope 0.1 and 0.2), ReLU mask;
    dsr_nstride 3HW and 6HW."""
    return [case("last2_dgrad", shape, mask="none"), case("last2_dgrad", shape, mask="aux"), case("last2_dgrad", shape, mask="bits"),
            case("last2_dgrad", shape, mask="aux", nstride_mul=2), case("last2_dgrad", shape, mask="bits", mode=1),
            case("last2_dgrad", shape, mask="bits", slope=SLOPE2)]


def planar_cases(shape, dtype):
    """planar -> 64: the stem / conv_0 (3 planes, bias, LeakyReLU), conv_9's data gradient (1 plane, mask), and everything at once with
    slope 0.1 and 0.2 (activation and mask)."""
    return [case("planar_c64", shape, dtype, pc=3), case("planar_c64", shape, dtype, pc=1, act=0, bias=False, mask="aux"),
            case("planar_c64", shape, dtype, pc=3, mask="aux", gap=12), case("planar_c64", shape, dtype, pc=3, mask="aux", slope=SLOPE2)]


def wgrad_cases(shape, dtype):
    return [case("last2_wgrad", shape, dtype, pc=pc, nstride_mul=m) for pc in (1, 2, 3) for m in (1, 2)]


def unshuffle_cases(shape):
    return [case("unshuffle", shape, mode=0), case("unshuffle", shape, mode=1, bias=False)]


def ps_dgrad_cases(shape, dtype):
    cs = [case("ps_dgrad", shape, dtype), case("ps_dgrad", shape, dtype, mask="aux")]
    if dtype == "bf16":
        cs += [case("ps_dgrad", shape, dtype, mask="bits"), case("ps_dgrad", shape, dtype, dy_planes=1),
               case("ps_dgrad", shape, dtype, mask="bits", dy_planes=1)]
    return cs


def ps_wgrads_cases(shape, dtype):
    return [case("ps_wgrads", shape, dtype), case("ps_wgrads", shape, dtype, dy_planes=1)]


def gpu_cases():
    cs = []
    for s in SHAPES:
        for dt in ("bf16", "fp32"):
            cs += fwd_cases(s, dt) + planar_cases(s, dt) + wgrad_cases(s, dt) + ps_dgrad_cases(s, dt) + ps_wgrads_cases(s, dt)
        cs += dgrad_cases(s) + unshuffle_cases(s)
    for s in SKIP_SHAPES:
        for dt in ("bf16", "fp32"):
            cs += skip_cases(s, dt)
    cs += [case("last2_dgrad", BIG_DGRAD, mask="aux"), case("last2_dgrad", BIG_DGRAD, mask="bits")]
    return cs


def distinct(cases):
    """One case per (operation, values, dtype): placement options repeat the same numbers."""
    seen, out = set(), []
    for c in cases:
        k = (_core(c), c.dtype)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out
