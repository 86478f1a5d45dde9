"""Shared by test_trunk_host.py and test_trunk_gpu.py: the propagation trunk's launches (the C -> C convolutions of the residual
blocks and their masked data gradients, the stem on cat([lr, feat]), the 1x1 fusion conv, their weight gradients, the chain launch)
restated in fp64, the elementwise bound of tests/hr_tail_common.py, and the driver of the ``vsr_debug_trunk_*`` hooks
(csrc/trunk_hooks.hip).  The pieces of hr_tail_common are used as they are: Case, Guarded, Planar, PmOutput, pm_input, draw, draw_aux,
mask_factor, _conv, _wgrad, measure_against / check_against.

* ``reference(case)``: every operation from ``F.conv2d`` and index arithmetic (test_trunk_host.py pins them at 1e-10 to torch autograd on
  the oracle's ``residual_conv``, the stem on ``cat([lr, feat])`` and the 1x1 fusion on ``cat([a, b])``).  Each output comes with
  ``A = sum |a_k b_k|`` from the same code on the operands' magnitudes and its term count K.
* the bound is the tail's: a bf16 output |err| <= u |r| + 2 K 2^-24 A, an fp32 output |err| <= 2 K 2^-24 A, no element exempt.  ReLU and
  LeakyReLU are 1-Lipschitz, so the bound of the activation's argument holds behind it; a bias, a residual, a planar `pres` and the
  pre-filled gradient of an accumulating weight gradient are each one of the K terms.  What a launch must leave alone (the other
  input-channel half of a weight gradient written at ``i_off``) has A = 0, hence the bound 0: bit-exact.
* masks come from a GIVEN activation ``aux`` (``draw_aux``: +-0 and +-2^-133 on the first and the last column), gradient x (aux > 0 ? 1 :
  slope).  Where a forward launch has written sign bits, the GPU tests hand the launch's own stored output in as ``aux``
  (``given=``) and compare the three mask sources bit for bit; the word layout is never restated here.
* two input families.  ``rand``: uniform(-1, 1), bf16-representable.  ``grid``: every operand (bias, residual, pre-filled gradient
  too) from {-1, -1/2, 0, 1/2, 1}, ReLU or no activation, ReLU masks only.  Then every product and every partial sum is a multiple of
  1/4, and fp32 holds multiples of 1/4 exactly below 2^22: as long as A < 2^22 (asserted per case by ``reference``) an fp32
  evaluation in ANY order is exact, so an fp32 output has to equal the fp64 reference and a bf16 output its round-to-nearest-even,
  bit for bit.  At (3, 80, 352) with three segments K is 2.5e5 and 2 K 2^-24 A exceeds the gradient itself: the grid family is what
  sees a missing column, segment or accumulate there.
* a chain is checked layer by layer against fp64 applied to the image the GPU stored for that layer's input, with the mask from the
  stored activation: the per-element bound then holds at every depth and nothing compounds (``chain_layers`` / ``check_chain``).
* ``emulate(case, mut)``: fp32, reduction axes reversed, rounded to bf16 where the bf16 build stores; ``mut`` is one of MUTATIONS.
* ``run_hip(case, dev)``: one hook call; inputs with NaN padding pixels in NaN-banded buffers, outputs between sentinel bands, the
  status checked before anything reads an output."""
import ctypes
import functools

import torch
import torch.nn.functional as F

import hr_tail_common as T
from hr_tail_common import Case, EPS, SENTINEL, SLOPE, U, bf16_round, draw, draw_aux, mask_factor, ragged, same_bits, sid  # noqa: F401

SMALL = T.SHAPES[:-1]                # (1,1,1) (1,8,32) (2,13,37) (1,3,66) (1,9,31) (1,17,100)
BIG = T.SHAPES[-1]                   # (3,80,352): 330 tiles on 256 persistent workgroups; a TileIter crosses an image boundary
WIDE = (1, 40, 1000)                 # 5 x 32 tiles: a workgroup's stride wraps tile rows; second tile buffer and the weight-gradient rings re-used
SHAPES = T.SHAPES + [WIDE]
MUTATIONS = ("drop_last_segment", "drop_last_column", "accumulate_overwrites", "i_off_ignored", "stem_sets_swapped", "res_from_layer_input",
             "tap_mirrored", "halo_reads_beyond_w", "mask_ge")
NONE = 0xffffffff
CHAIN_RELU, CHAIN_SKIP, CHAIN_MASK = 0, 1, 2


def case(hook, shape, dtype="bf16", **opts):
    return Case(hook, tuple(shape), dtype, tuple(sorted(opts.items())))


def draw_grid(seed, *shape):
    """{-1, -1/2, 0, 1/2, 1}, fp32."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(0, 5, shape, generator=g).float() / 2 - 1


# --------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def make_inputs(hook, shape, key):
    """CPU fp32 tensors of one (hook, shape); key: the options that change the operands."""
    n, h, w = shape
    o = dict(key)
    C, fam = o.get("C", 64), o.get("family", "rand")
    s = 9000 + 131 * h + 17 * w + n + 7 * C + {"conv": 0, "stem": 100, "stem_dgrad": 200, "point": 300, "wgrad_cc": 400, "stem_wgrads": 500, "chain": 600}[hook]
    d = draw_grid if fam == "grid" else draw
    fl = d if fam == "grid" else (lambda sd, *sh: torch.randn(*sh, generator=torch.Generator().manual_seed(sd)))      # fp32 operands: bias, pres, pre-filled gradients
    if hook == "conv":
        ks = o.get("ks", 3)
        return dict(x=d(s, n, C, h, w), w=d(s + 1, C, C, ks, ks), bias=fl(s + 2, C), res=d(s + 3, n, C, h, w), aux=draw_aux(s + 4, n, h, w, C))
    if hook == "stem":
        return dict(lr=d(s, n, 3, h, w), feat=d(s + 1, n, C, h, w), w=d(s + 2, C, C + 3, 3, 3), bias=fl(s + 3, C))
    if hook == "stem_dgrad":
        return dict(g0=d(s, n, C, h, w), w=d(s + 1, C, C + 3, 3, 3), pres=fl(s + 2, n, 3, h, w))
    if hook == "point":
        return dict(a=d(s, n, C, h, w), b=d(s + 1, n, C, h, w), w=d(s + 2, C, 2 * C, 1, 1), bias=fl(s + 3, C))
    if hook == "wgrad_cc":
        ns, ks = o.get("nseg", 1), o.get("ks", 3)
        return dict(x=d(s, ns, n, C, h, w), dy=d(s + 1, ns, n, C, h, w), gw0=fl(s + 2, C, 2 * C, ks, ks), gb0=fl(s + 3, C))
    if hook == "stem_wgrads":
        ns = o.get("nseg", 1)
        return dict(lr=d(s, ns, n, 3, h, w), feat=d(s + 1, ns, n, C, h, w), g0=d(s + 2, ns, n, C, h, w), gw0=fl(s + 3, C, C + 3, 3, 3), gb0=fl(s + 4, C))
    if hook == "chain":
        nb = o.get("blocks", 2)
        # (small weights in the rand family keep the images O(1) through the blocks; the grid family's are what they are)
        sc = 1.0 if fam == "grid" else 0.125
        return dict(x0=d(s, n, 64, h, w), dx=d(s + 1, n, 64, h, w), w=bf16_round(d(s + 2, 2 * nb, 64, 64, 3, 3) * sc), bias=fl(s + 3, 2 * nb, 64) * sc)
    raise KeyError(hook)


_OPERAND_OPTS = ("C", "family", "ks", "nseg", "blocks")


def inputs_of(c: Case):
    return make_inputs(c.hook, c.shape, tuple((k, v) for k, v in c.opts if k in _OPERAND_OPTS))


# --------------------------------------------------------------------------------------------------------------------
# the operations, in the dtype of their operands.  rev: the reduction axes reversed; mut: one of MUTATIONS
# --------------------------------------------------------------------------------------------------------------------
def _convk(x, w, mut=None, rev=False):
    """'same' convolution, 3x3 or 1x1."""
    if w.shape[-1] == 3:
        return T._conv(x, w, mut, rev)
    return F.conv2d(x.flip(1), w.flip(1)) if rev else F.conv2d(x, w)


def _dgrad_w(w):
    return w.transpose(0, 1).flip(2, 3)


def _wgradk(x, dy, ks, mut=None, rev=False):
    """(gw (Co, Ci, ks, ks), gb (Co)) of one segment."""
    if ks == 3:
        return T._wgrad(x, dy, mut if mut in ("drop_last_column", "halo_reads_beyond_w", "tap_mirrored") else None, rev)
    if mut == "drop_last_column":
        dy = dy.clone()
        dy[..., -1] = 0
    if rev:
        x, dy = x.flip(0, 3), dy.flip(0, 3)
    return F.conv2d(x.transpose(0, 1), dy.transpose(0, 1)).transpose(0, 1), dy.sum(dim=(0, 2, 3))


def _act(y, act, slope):
    return torch.relu(y) if act == 1 else (torch.where(y > 0, y, y * slope) if act == 2 else y)


def conv_layer(x, w, bias=None, res=None, aux=None, act=0, mask_mode=0, slope=SLOPE, mode=0, mut=None, rev=False):
    """Ctx::conv: act(conv(x) + bias) (+ res) (* mask(aux)); mode 1: the data-gradient weights of w.  (A residual comes with no
    activation in every recipe of the engines: that is the order stated, and the only one used.)"""
    y = _convk(x, _dgrad_w(w) if mode else w, mut, rev)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    y = _act(y, act, slope)
    if res is not None:
        y = y + (x if mut == "res_from_layer_input" else res)
    if mask_mode:
        y = y * mask_factor(aux, 0.0 if mask_mode == 1 else slope, mut)
    return y


def _segsum(parts, mut):
    parts = list(parts)
    if mut == "drop_last_segment" and len(parts) > 1:
        parts = parts[:-1]
    return functools.reduce(lambda a, b: a + b, parts)


def _ops(c: Case, t, mut=None, rev=False):
    n, h, w = c.shape
    C, slope = c.o("C", 64), c.o("slope", SLOPE)
    if c.hook == "conv":
        mask_mode = 0 if c.o("mask", "none") == "none" else c.o("mask_mode", 1)
        return dict(y=conv_layer(t["x"], t["w"], t["bias"] if c.o("bias", True) else None, t["res"] if c.o("res", 0) else None, t["aux"], c.o("act", 0),
                                 mask_mode, slope, c.o("mode", 0), mut, rev))
    if c.hook == "stem":
        wl, wf = t["w"][:, :3], t["w"][:, 3:]
        if c.o("cat", 1) and mut == "stem_sets_swapped":   # as if the input were cat([feat, lr])
            wl, wf = t["w"][:, C:], t["w"][:, :C]
        y = _convk(t["lr"], wl, mut, rev)
        if c.o("cat", 1) and c.o("feat", 1):
            y = y + _convk(t["feat"], wf, mut, rev)
        y = y + t["bias"].view(1, -1, 1, 1)
        return dict(y=_act(y, c.o("act", 2), slope))
    if c.hook == "stem_dgrad":
        cat = c.o("cat", 1)
        wl, wf = t["w"][:, :3], t["w"][:, 3:]
        if cat and mut == "stem_sets_swapped":
            wl, wf = t["w"][:, C:], t["w"][:, :C]
        out = dict(dlr=_convk(t["g0"], _dgrad_w(wl), mut, rev))
        if c.o("accumulate", 0) and mut != "accumulate_overwrites":
            out["dlr"] = out["dlr"] + t["pres"]
        if cat:
            out["dfeat"] = _convk(t["g0"], _dgrad_w(wf), mut, rev)
        return out
    if c.hook == "point":
        if c.o("backward", 0):
            wa, wb = t["w"][:, :C], t["w"][:, C:]
            if mut == "i_off_ignored":
                wb = wa
            return dict(d0=_convk(t["a"], _dgrad_w(wa), mut, rev), d1=_convk(t["a"], _dgrad_w(wb), mut, rev))
        y = _convk(torch.cat([t["a"], t["b"]], 1), t["w"], mut, rev) + t["bias"].view(1, -1, 1, 1)
        return dict(y=_act(y, 2, slope))
    if c.hook == "wgrad_cc":
        ks, ns, acc = c.o("ks", 3), c.o("nseg", 1), c.o("accumulate", 0)
        it, io = c.o("I_total", C), c.o("i_off", 0)
        parts = [_wgradk(t["x"][s], t["dy"][s], ks, mut if (s == 0 or mut != "drop_last_column") else None, rev) for s in range(ns)]
        gw, gb = _segsum([p[0] for p in parts], mut), _segsum([p[1] for p in parts], mut)
        out_w = t["gw0"][:, :it].clone()
        at = 0 if mut == "i_off_ignored" else io
        keep = acc and mut != "accumulate_overwrites"
        out_w[:, at:at + C] = (out_w[:, at:at + C] + gw) if keep else gw
        out = dict(gw=out_w)
        if c.o("gb", True):
            out["gb"] = (t["gb0"] + gb) if keep else gb
        return out
    if c.hook == "stem_wgrads":
        cat, ns, acc = c.o("cat", 1), c.o("nseg", 1), c.o("accumulate", 0)
        nf = ns - 1 if cat else 0                          # the first frame of a direction has no state
        pl = [_wgradk(t["lr"][s], t["g0"][s], 3, mut if (s == 0 or mut != "drop_last_column") else None, rev) for s in range(ns)]
        pf = [_wgradk(t["feat"][s], t["g0"][s + 1], 3, mut if mut != "drop_last_column" else None, rev)[0] for s in range(nf)]
        keep = acc and mut != "accumulate_overwrites"
        out_w = t["gw0"][:, :(C + 3 if cat else 3)].clone()
        sl_l, sl_f = (slice(C, C + 3), slice(0, C)) if (cat and mut == "stem_sets_swapped") else (slice(0, 3), slice(3, C + 3))
        gl = _segsum([p[0] for p in pl], mut)
        out_w[:, sl_l] = (out_w[:, sl_l] + gl) if keep else gl
        if nf:
            gf = _segsum(pf, mut)
            out_w[:, sl_f] = (out_w[:, sl_f] + gf) if keep else gf
        gb = _segsum([p[1] for p in pl], mut)
        return dict(gw=out_w, gb=(t["gb0"] + gb) if keep else gb)
    raise KeyError(c.hook)


def terms(c: Case):
    n, h, w = c.shape
    C = c.o("C", 64)
    if c.hook == "conv":
        return dict(y=c.o("ks", 3) ** 2 * C + 3)
    if c.hook == "stem":
        return dict(y=9 * (C + 3) + 1)
    if c.hook == "stem_dgrad":
        return dict(dlr=9 * C + 1, dfeat=9 * C)
    if c.hook == "point":
        return dict(d0=C, d1=C) if c.o("backward", 0) else dict(y=2 * C + 1)
    k = c.o("nseg", 1) * n * h * w + 1
    return dict(gw=k, gb=k)


def bf16_outputs(c: Case):
    if c.dtype != "bf16":
        return ()
    return {"conv": ("y",), "stem": ("y",), "stem_dgrad": ("dfeat",), "point": ("y", "d0", "d1")}.get(c.hook, ())


def applicable(c: Case, mut):
    """Whether the mutation changes anything the operation of `c` computes."""
    ks3 = c.o("ks", 3) == 3 and c.hook != "point"
    wg = c.hook in ("wgrad_cc", "stem_wgrads")
    if mut == "drop_last_segment":
        return wg and c.o("nseg", 1) > 1
    if mut == "drop_last_column":
        return wg
    if mut == "accumulate_overwrites":
        return (wg or c.hook == "stem_dgrad") and c.o("accumulate", 0) == 1
    if mut == "i_off_ignored":
        return (c.hook == "wgrad_cc" and c.o("i_off", 0) > 0) or (c.hook == "point" and c.o("backward", 0) == 1)
    if mut == "stem_sets_swapped":
        return c.hook in ("stem", "stem_dgrad", "stem_wgrads") and c.o("cat", 1) == 1
    if mut == "res_from_layer_input":
        return c.hook == "conv" and bool(c.o("res", 0))
    if mut == "tap_mirrored":
        return ks3 and c.shape[2] >= 2
    if mut == "halo_reads_beyond_w":
        return ks3
    if mut == "mask_ge":
        return c.hook == "conv" and c.o("mask", "none") != "none"
    raise KeyError(mut)


_LAYOUT_OPTS = ("gap", "inplace", "sign_out")


def _core(c: Case):
    o = {k: ("aux" if k == "mask" and v != "none" else v) for k, v in c.opts if k not in _LAYOUT_OPTS}
    return Case(c.hook, c.shape, "any", tuple(sorted(o.items())))


def _linear(c: Case):
    """The case without its activation: ReLU and LeakyReLU are 1-Lipschitz, the bound of the argument passes."""
    o = dict(c.opts)
    if c.hook in ("conv", "stem"):
        o["act"] = 0
    return Case(c.hook, c.shape, c.dtype, tuple(sorted(o.items())))


def _values_of(c: Case, inp):
    r = _ops(c, inp)
    mag = {k: v.abs() for k, v in inp.items()}
    if "aux" in inp:
        mag["aux"] = inp["aux"]                            # the mask is a factor, not a term: it keeps its sign test
    if c.hook == "point" and not c.o("backward", 0):
        y = F.conv2d(torch.cat([mag["a"], mag["b"]], 1), mag["w"]) + mag["bias"].view(1, -1, 1, 1)
        a = dict(y=y)
    else:
        a = _ops(_linear(c), mag)
    if c.hook == "wgrad_cc":                               # what the launch leaves alone: A = 0, bit-exact
        C, it, io = c.o("C", 64), c.o("I_total", c.o("C", 64)), c.o("i_off", 0)
        keep = torch.zeros(it, dtype=torch.bool)
        keep[io:io + C] = True
        a["gw"] = a["gw"] * keep.view(1, -1, 1, 1)
    if c.hook == "stem_wgrads" and c.o("cat", 1) and c.o("nseg", 1) == 1:
        a["gw"][:, 3:] = 0
    if c.o("family", "rand") == "grid":
        for k, v in a.items():
            assert float(v.max()) < 2.0 ** 22, (c.name, k, float(v.max()))      # multiples of 1/4 below 2^22: exact in fp32 in any order
    return r, a


@functools.lru_cache(maxsize=6)
def _values(c: Case):
    return _values_of(c, {k: v.double() for k, v in inputs_of(c).items()})


def _with(c: Case, given):
    inp = dict(inputs_of(c))
    inp.update(given or {})
    return inp


def reference(c: Case, given=None):
    """(r, A) per output name, fp64.  given: tensors that replace drawn inputs (a stored activation as `aux`): not cached."""
    if given:
        return _values_of(_core(c), {k: v.double() for k, v in _with(c, given).items()})
    return _values(_core(c))


def bounds(c: Case, given=None):
    r, a = reference(c, given)
    out = {}
    grid = c.o("family", "rand") == "grid"
    for k in r:
        acc = torch.zeros_like(a[k]) if grid else 2 * terms(c)[k] * EPS * a[k]
        rnd = U * r[k].abs() if (k in bf16_outputs(c) and not grid) else torch.zeros_like(acc)
        out[k] = (acc, rnd)
    return out


def expected(c: Case, given=None):
    """What the outputs are held to: the fp64 values; grid family, bf16 output: their round-to-nearest-even (then the bound is 0)."""
    r, _ = reference(c, given)
    if c.o("family", "rand") == "grid":
        return {k: (bf16_round(v.float()).double() if k in bf16_outputs(c) else v) for k, v in r.items()}
    return r


def emulate(c: Case, mut=None, given=None):
    inp = {k: v.float() for k, v in _with(c, given).items()}
    out = _ops(c, inp, mut=mut, rev=True)
    return {k: (bf16_round(v) if k in bf16_outputs(c) else v) for k, v in out.items()}


def measure(c: Case, got, given=None):
    return T.measure_against(c.name, got, expected(c, given), bounds(c, given))


def check(c: Case, got, label="hip", given=None):
    """Every element of every output inside its bound (grid family: equal); prints the worst ratios."""
    return T.check_against(c.name, got, expected(c, given), bounds(c, given), label, tag="TRUNK_RATIO")


def passes(c: Case, got, given=None):
    return all(v[0] <= 1.0 for v in measure(c, got, given).values())


# --------------------------------------------------------------------------------------------------------------------
# chains: layer lists, the layer-by-layer check
# --------------------------------------------------------------------------------------------------------------------
def chain_layers(nb):
    """(forward, backward): per layer (variant, src, dst, res, mask source, weight index, has bias) by image NAME, as
    trunk_chain_forward / trunk_chain_backward of engine.hip build them."""
    fwd, bwd = [], []
    for b in range(nb):
        fwd.append((CHAIN_RELU, f"x{b}", f"a{b}", None, None, 2 * b, True))
        fwd.append((CHAIN_SKIP, f"a{b}", f"x{b + 1}", f"x{b}", None, 2 * b + 1, True))
    for b in range(nb - 1, -1, -1):
        bwd.append((CHAIN_MASK, f"dx{b + 1}", f"da{b}", None, f"a{b}", 2 * b + 1, False))
        if b > 0:
            bwd.append((CHAIN_SKIP, f"da{b}", f"dx{b}", f"dx{b + 1}", None, 2 * b, False))
    return fwd, bwd


def chain_layer_eval(c: Case, layer, img, backward, dtype=torch.float64, mut=None, rev=False):
    """One layer of the chain on the images `img` (name -> (N, 64, H, W)), in `dtype`."""
    variant, src, dst, res, msk, wi, has_bias = layer
    t = inputs_of(c)
    cv = lambda v: v.to(dtype)
    return conv_layer(cv(img[src]), cv(t["w"][wi]), cv(t["bias"][wi]) if has_bias else None, cv(img[res]) if res else None,
                      cv(img[msk]) if msk else None, act=1 if variant == CHAIN_RELU else 0, mask_mode=1 if msk else 0, mode=1 if backward else 0,
                      mut=mut, rev=rev)


def emulate_chain(c: Case, mut=None):
    """The stored images of the forward and the backward chain: fp32, reversed order, every image rounded to bf16."""
    t = inputs_of(c)
    nb = c.o("blocks", 2)
    img = dict(x0=t["x0"], **{f"dx{nb}": t["dx"]})
    fwd, bwd = chain_layers(nb)
    for L in fwd:
        img[L[2]] = bf16_round(chain_layer_eval(c, L, img, False, torch.float32, mut, True))
    for L in bwd:
        img[L[2]] = bf16_round(chain_layer_eval(c, L, img, True, torch.float32, mut, True))
    return img


def measure_chain(c: Case, img):
    """Every layer's stored output against fp64 applied to the layer's STORED inputs.  dict image name -> measure()'s triple."""
    nb = c.o("blocks", 2)
    grid = c.o("family", "rand") == "grid"
    fwd, bwd = chain_layers(nb)
    res = {}
    for layers, backward in ((fwd, False), (bwd, True)):
        for L in layers:
            r = chain_layer_eval(c, L, img, backward)
            mag = {k: v.abs() for k, v in img.items()}
            if L[4]:
                mag[L[4]] = img[L[4]]
            tm = inputs_of(c)
            a = conv_layer(mag[L[1]].double(), tm["w"][L[5]].abs().double().transpose(0, 1).flip(2, 3) if backward else tm["w"][L[5]].abs().double(),
                           tm["bias"][L[5]].abs().double() if L[6] else None, mag[L[3]].double() if L[3] else None,
                           mag[L[4]].double() if L[4] else None, act=0, mask_mode=1 if L[4] else 0)
            if grid:
                # stored images are multiples of 1/4 (the bf16 rounding of a multiple of 1/4 is one), weights and biases of 1/2:
                # every product and partial sum is a multiple of 1/8, which fp32 holds exactly below 2^21
                assert float(a.max()) < 2.0 ** 21, (c.name, L[2], float(a.max()))
                want, bnd = bf16_round(r.float()).double(), (torch.zeros_like(a), torch.zeros_like(a))
            else:
                want, bnd = r, (2 * (576 + 3) * EPS * a, U * r.abs())
            res.update(T.measure_against(c.name, {L[2]: img[L[2]]}, {L[2]: want}, {L[2]: bnd}))
    return res


def check_chain(c: Case, img, label="hip"):
    m = measure_chain(c, img)
    for k, (ratio, acc_ratio, idx) in m.items():
        print(f"TRUNK_RATIO {label} {c.name} {k}: worst err/bound {ratio:.3f} at {idx}, accumulation share {acc_ratio:.3f}")
    bad = {k: v for k, v in m.items() if not v[0] <= 1.0}
    assert not bad, (c.name, bad)
    return m


# --------------------------------------------------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------------------------------------------------
def _ptrs(ts):
    arr = (ctypes.c_void_p * max(len(ts), 1))()
    for i, t in enumerate(ts):
        arr[i] = t if isinstance(t, int) else t.data_ptr()
    return arr


def sign_words(n, h, w):
    return n * ((h + 7) // 8) * ((w + 31) // 32) * 512      # int32 words: 2048 bytes per tile


def run_hip(c: Case, dev, given=None, bits=None):
    """One hook call on the inputs of `c` (`given` replaces some); dict output name -> fp32 CPU tensor in reference()'s layout.  conv cases
    with sign_out also return `_bits` (the device tensor of sign words, to be handed back in as `bits=`).  A HIP error ends the session."""
    return T.fault_guarded(c, _run_hip, dev, given, bits)


def _run_hip(c: Case, dev, given, bits):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    inp = _with(c, given)
    n, h, w = c.shape
    C = c.o("C", 64)
    CO = max(C, 32)
    dt = VF.DT_BF16 if c.dtype == "bf16" else VF.DT_F32
    tdt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    st, nan = VF._stream(), float("nan")
    P = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    keep = []

    def held(t):
        keep.append(t)
        return t

    scratch = lambda numel, dtype=tdt: held(torch.full((numel,), 1.0, dtype=dtype, device=dev))
    slab = lambda: held(torch.empty(lib.vsr_conv3x3_c64_wgrad_slab_floats(), dtype=torch.float32, device=dev))
    pm = lambda t: held(T.pm_input(t, c.dtype, dev))
    out_pm = lambda: T.PmOutput(n, h, w, c.dtype, dev, c=C)
    devf = lambda t: held(t.to(dev).contiguous())
    slope = c.o("slope", SLOPE)

    if c.hook == "conv":
        ks, mask = c.o("ks", 3), c.o("mask", "none")
        x = pm(inp["x"])
        y = out_pm()
        res = None
        if c.o("res", 0):
            if c.o("inplace", 0):                          # res aliases y: the residual is read from the destination
                y.g.body.view(y.shape).copy_(T.pm_input(inp["res"], c.dtype, dev))
                res = y.ptr()
            else:
                res = P(pm(inp["res"]))
        aux = pm(inp["aux"]) if mask != "none" else None
        sout = T.Guarded(sign_words(n, h, w), torch.int32, dev, -1) if c.o("sign_out", 0) else None
        made = T.Guarded(sign_words(n, h, w), torch.int32, dev, -1) if mask == "made" else None
        sbits = bits if mask == "bits" else (made.body if made else None)
        rc = lib.vsr_debug_trunk_conv(dt, C, ks, c.o("mode", 0), P(x), P(devf(inp["w"])), P(devf(inp["bias"])) if c.o("bias", True) else None,
                                      P(scratch(ks * ks * CO * C)), y.ptr(), c.o("act", 0), slope, res, P(aux), c.o("mask_mode", 1) if aux is not None else 0,
                                      P(sout.body) if sout else None, P(sbits), int(mask == "made"), 0, n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert all(g.bands_untouched() for g in (sout, made) if g), "sign words were written outside their buffer"
        out = dict(y=y.take())
        if sout is not None:
            out["_bits"] = sout.body
        return out
    if c.hook == "stem":
        cat = c.o("cat", 1)
        ns = 3 * h * w + c.o("gap", 0)
        lr = T.Planar(n, 3, h, w, ns, dev, nan, inp["lr"])
        feat = pm(inp["feat"]) if (cat and c.o("feat", 1)) else None
        y = out_pm()
        wt = inp["w"] if cat else inp["w"][:, :3]
        rc = lib.vsr_debug_trunk_stem(dt, C, cat, P(feat), P(lr.view), ns, P(devf(wt)), P(devf(inp["bias"])), P(scratch(9 * CO * (C + 16))), y.ptr(),
                                      c.o("act", 2), slope, n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(y=y.take())
    if c.hook == "stem_dgrad":
        cat, acc = c.o("cat", 1), c.o("accumulate", 0)
        ns = 3 * h * w + c.o("gap", 0)
        g0 = pm(inp["g0"])
        dlr = T.Planar(n, 3, h, w, ns, dev, SENTINEL, inp["pres"] if acc else None)
        if not acc:
            dlr.view.fill_(nan)                            # overwritten: whatever was there must not come through
        dfeat = out_pm() if cat else None
        wt = inp["w"] if cat else inp["w"][:, :3]
        rc = lib.vsr_debug_trunk_stem_dgrad(dt, C, cat, P(g0), P(devf(wt)), P(scratch(9 * CO * C + 9 * 32 * C)), dfeat.ptr() if cat else None, P(dlr.view), ns, acc,
                                            n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        out = dict(dlr=dlr.take())
        if cat:
            out["dfeat"] = dfeat.take()
        return out
    if c.hook == "point":
        a = pm(inp["a"])
        wp = scratch(2 * CO * C)
        if c.o("backward", 0):
            d0, d1 = out_pm(), out_pm()
            rc = lib.vsr_debug_trunk_point(dt, C, 1, P(a), None, P(devf(inp["w"])), None, P(wp), d0.ptr(), d1.ptr(), n, h, w, st)
            assert rc == 0, (c.name, rc)
            T._sync()
            return dict(d0=d0.take(), d1=d1.take())
        y = out_pm()
        rc = lib.vsr_debug_trunk_point(dt, C, 0, P(a), P(pm(inp["b"])), P(devf(inp["w"])), P(devf(inp["bias"])), P(wp), y.ptr(), None, n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        return dict(y=y.take())
    if c.hook == "wgrad_cc":
        ks, ns, acc = c.o("ks", 3), c.o("nseg", 1), c.o("accumulate", 0)
        it, io = c.o("I_total", C), c.o("i_off", 0)
        xs, dys = [pm(inp["x"][s]) for s in range(ns)], [pm(inp["dy"][s]) for s in range(ns)]
        gw, gb = T.Guarded(C * it * ks * ks, torch.float32, dev, SENTINEL), T.Guarded(C, torch.float32, dev, SENTINEL)
        gw.body.copy_(inp["gw0"][:, :it].contiguous().flatten())      # pre-filled: accumulated into, or -- outside [i_off, i_off + C) -- left alone
        gb.body.copy_(inp["gb0"])
        if not acc:
            gw.body.view(C, it, ks, ks)[:, io:io + C] = nan            # overwritten
            gb.body.fill_(nan)
        rc = lib.vsr_debug_trunk_wgrad_cc(dt, C, ks, _ptrs(xs), _ptrs(dys), ns, P(gw.body), it, io, P(gb.body) if c.o("gb", True) else None, acc, P(slab()),
                                          n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert gw.bands_untouched() and gb.bands_untouched(), "a weight gradient was written outside its tensor"
        out = dict(gw=gw.body.view(C, it, ks, ks).cpu().clone())
        if c.o("gb", True):
            out["gb"] = gb.body.cpu().clone()
        return out
    if c.hook == "stem_wgrads":
        cat, ns, acc = c.o("cat", 1), c.o("nseg", 1), c.o("accumulate", 0)
        nf = ns - 1 if cat else 0
        xns = 3 * h * w + c.o("gap", 0)
        lrs = [held(T.Planar(n, 3, h, w, xns, dev, nan, inp["lr"][s])) for s in range(ns)]
        g0 = [pm(inp["g0"][s]) for s in range(ns)]
        feat = [pm(inp["feat"][s]) for s in range(nf)]
        it = C + 3 if cat else 3
        gw, gb = T.Guarded(C * it * 9, torch.float32, dev, SENTINEL), T.Guarded(C, torch.float32, dev, SENTINEL)
        gw.body.copy_(inp["gw0"][:, :it].contiguous().flatten())
        gb.body.copy_(inp["gb0"])
        if not acc:
            gw.body.view(C, it, 3, 3)[:, :(it if nf else 3)] = nan
            gb.body.fill_(nan)
        rc = lib.vsr_debug_trunk_stem_wgrads(dt, C, cat, _ptrs([p.view for p in lrs]), xns, _ptrs(g0), ns, _ptrs(feat) if nf else None,
                                             _ptrs(g0[1:]) if nf else None, nf, P(gw.body), P(gb.body), acc, P(slab()), n, h, w, st)
        assert rc == 0, (c.name, rc)
        T._sync()
        assert gw.bands_untouched() and gb.bands_untouched(), "a weight gradient was written outside its tensor"
        return dict(gw=gw.body.view(C, it, 3, 3).cpu().clone(), gb=gb.body.cpu().clone())
    raise KeyError(c.hook)


GAP = 4096                            # sentinel bytes between the slots of a chain's allocation (a multiple of 256)
FILL = 0xA5


def run_chain(c: Case, dev):
    """The forward chain of `blocks` residual blocks, then the matching backward chain reading the sign words the forward one wrote:
    images, packed weights, biases, sign words and the sync block are slots of ONE allocation with sentinel gaps, addressed as
    256-byte offsets from its base.  dict image name -> (N, 64, H, W) fp32 CPU: what each layer stored (and the two given images).
    A HIP error ends the session."""
    return T.fault_guarded(c, _run_chain, dev)


def _run_chain(c: Case, dev):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    inp = inputs_of(c)
    n, h, w = c.shape
    nb = c.o("blocks", 2)
    fwd, bwd = chain_layers(nb)
    names = ["x0"] + [L[2] for L in fwd] + [f"dx{nb}"] + [L[2] for L in bwd]
    img_bytes = n * h * ((w + 31) // 32) * 32 * 64 * 2
    sync_bytes = int(lib.vsr_conv3x3_c64_chain_sync_bytes(2 * nb, n, h, w))
    slots, off = {}, GAP

    def take(name, nbytes):
        nonlocal off
        slots[name] = (off, nbytes)
        off += (nbytes + 255) // 256 * 256 + GAP

    for k in names:
        take(k, img_bytes)
    for l in range(2 * nb):
        take(f"wf{l}", 9 * 64 * 64 * 2)
        take(f"wb{l}", 9 * 64 * 64 * 2)
        take(f"b{l}", 256)
    for b in range(nb):
        take(f"s{b}", sign_words(n, h, w) * 4)
    take("sync", sync_bytes)
    buf = torch.full((off,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    region = lambda k: buf[slots[k][0]:slots[k][0] + slots[k][1]]
    shape = (n, h, (w + 31) // 32, 8, 32, 8)
    for k in names:
        region(k).view(torch.bfloat16).fill_(SENTINEL)
    for k in ("x0", f"dx{nb}"):                            # the given images, padding pixels NaN
        region(k).view(torch.bfloat16).view(shape).copy_(T.pm_input(inp["x0" if k == "x0" else "dx"], "bf16", dev))
    for l in range(2 * nb):
        region(f"b{l}").view(torch.float32).copy_(inp["bias"][l].to(dev))
    wdev = [inp["w"][l].to(dev).contiguous() for l in range(2 * nb)]
    o256 = lambda k: NONE if k is None else slots[k][0] // 256

    def launch(layers, backward):
        words = []
        for (variant, src, dst, res, msk, wi, has_bias) in layers:
            b = wi // 2
            words += [o256(src), o256(dst), o256(res), o256(f"s{b}") if variant == CHAIN_MASK else NONE, o256(f"s{b}") if variant == CHAIN_RELU else NONE,
                      o256(("wb" if backward else "wf") + str(wi)), o256(f"b{wi}") if has_bias else NONE, variant]
        arr = (ctypes.c_uint * len(words))(*words)
        rc = lib.vsr_debug_trunk_chain(VF.DT_BF16, 64, buf.data_ptr(), buf.data_ptr() + slots["sync"][0], arr, len(layers), _ptrs([wdev[L[5]] for L in layers]),
                                       int(backward), n, h, w, VF._stream())
        assert rc == 0, (c.name, "backward" if backward else "forward", rc)
        T._sync()
        err = int(region("sync").view(torch.int32)[1])
        assert err == 0, (c.name, "the chain's error word is set", err)

    launch(fwd, False)
    launch(bwd, True)
    # every gap still holds the sentinel byte
    mask = torch.ones(off, dtype=torch.bool, device=dev)
    for o, nbytes in slots.values():
        mask[o:o + (nbytes + 255) // 256 * 256] = False
    assert bool((buf[mask] == FILL).all()), (c.name, "a chain launch wrote between its buffers")
    out = {}
    for k in names:
        v = region(k).view(torch.bfloat16).view(shape)
        v.pm_w = w
        out[k] = VF.from_pixel_major(v, 64).cpu()
    return out


# --------------------------------------------------------------------------------------------------------------------
# the case lists of test_trunk_gpu.py (test_trunk_host.py dry-runs the criterion over them)
# --------------------------------------------------------------------------------------------------------------------
def conv_cases(shape, dtype, C=64, family="rand"):
    """The arms the engines run: conv1 of a block (bias + ReLU), conv2 + skip (in place as well), the plain data gradient, the ReLU-masked
    one, (data gradient + dX) x LeakyReLU' of the stem, the 1x1."""
    k = lambda **o: case("conv", shape, dtype, C=C, family=family, **o)
    if shape in (BIG, WIDE):      # (their fp64 references take the CPU a second each: the arms whose tile walk differs, one family each)
        return [k(act=1), k(mode=1, bias=False, res=1, mask="aux", mask_mode=2)] if family == "rand" else \
               [k(res=1, inplace=1), k(mode=1, bias=False, mask="aux", mask_mode=1)]
    cs = [k(act=1), k(res=1), k(res=1, inplace=1), k(mode=1, bias=False), k(mode=1, bias=False, mask="aux", mask_mode=1), k(ks=1, act=1), k(ks=1, mode=1, bias=False)]
    if family == "rand":
        cs += [k(act=2), k(mode=1, bias=False, res=1, mask="aux", mask_mode=2), k(mode=1, bias=False, mask="aux", mask_mode=2)]
    return cs


def stem_cases(shape, dtype, C=64, family="rand"):
    k = lambda **o: case("stem", shape, dtype, C=C, family=family, act=0 if family == "grid" else 2, **o)
    if shape == BIG:
        return [k()]
    return [k(), k(feat=0), k(cat=0, gap=8)]


def stem_dgrad_cases(shape, dtype, C=64, family="rand"):
    k = lambda **o: case("stem_dgrad", shape, dtype, C=C, family=family, **o)
    if shape == BIG:
        return [k(accumulate=1, gap=3 * shape[1] * shape[2])]
    return [k(accumulate=1, gap=3 * shape[1] * shape[2]), k(accumulate=0), k(cat=0, accumulate=1)]


def point_cases(shape, dtype, C=64, family="rand"):
    return [case("point", shape, dtype, C=C, family=family, backward=1)] + ([case("point", shape, dtype, C=C, family=family)] if family == "rand" else [])


def wgrad_cc_cases(shape, dtype, C=64, family="rand"):
    k = lambda **o: case("wgrad_cc", shape, dtype, C=C, family=family, **o)
    if shape in (BIG, WIDE):
        return [k(nseg=3, accumulate=1), k(ks=1, nseg=8, accumulate=1, i_off=C, I_total=2 * C, gb=False)] if family == "grid" else [k(nseg=3, accumulate=1)]
    return [k(nseg=1, accumulate=0), k(nseg=3, accumulate=1), k(nseg=8, accumulate=0, gb=False), k(ks=1, nseg=3, accumulate=0, i_off=0, I_total=2 * C),
            k(ks=1, nseg=8, accumulate=1, i_off=C, I_total=2 * C, gb=False)]


def stem_wgrads_cases(shape, dtype, C=64, family="rand"):
    k = lambda **o: case("stem_wgrads", shape, dtype, C=C, family=family, **o)
    if shape == BIG:
        return [k(nseg=3, accumulate=1, gap=3 * shape[1] * shape[2])]
    return [k(nseg=3, accumulate=1, gap=3 * shape[1] * shape[2]), k(nseg=1, accumulate=0), k(cat=0, nseg=2, accumulate=1), k(nseg=8, accumulate=0)]


def chain_cases(shape):
    cs = [case("chain", shape, blocks=2), case("chain", shape, blocks=2, family="grid")]
    if shape not in (BIG, WIDE):
        cs.append(case("chain", shape, blocks=3))
    return cs


def hook_cases(shape, dtype, C=64):
    """Every non-chain case of one (shape, dtype, width).  WIDE: conv and wgrad_cc only; C < 64: the small shapes only."""
    cs = []
    for fam in ("rand", "grid"):
        cs += conv_cases(shape, dtype, C, fam) + wgrad_cc_cases(shape, dtype, C, fam)
        if shape != WIDE:
            cs += stem_cases(shape, dtype, C, fam) + stem_dgrad_cases(shape, dtype, C, fam) + point_cases(shape, dtype, C, fam) + stem_wgrads_cases(shape, dtype, C, fam)
    return cs


def gpu_cases():
    cs = []
    for s in SHAPES:
        for dt in ("bf16", "fp32"):
            cs += hook_cases(s, dt, 64)
    for s in SMALL:
        for C in (16, 32):
            for dt in ("bf16", "fp32"):
                cs += hook_cases(s, dt, C)
    return cs


def distinct(cases):
    seen, out = set(), []
    for c in cases:
        k = (_core(c), c.dtype)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out
