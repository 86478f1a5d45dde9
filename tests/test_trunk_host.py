"""CPU side of the propagation-trunk harness (tests/trunk_common.py, csrc/trunk_hooks.hip):

* the fp64 restatements that test_trunk_gpu.py measures the kernels against are pinned at 1e-10 to torch autograd on the oracle's
  ``residual_conv``, on the stem as ``residual_block`` writes it on ``cat([lr, feat])`` and on the 1x1 fusion conv on ``cat([a, b])``,
  weight gradients summed over frames included;
* the criterion is dry-run: over every GPU case an fp32 evaluation in the reversed summation order (rounded to bf16 where the bf16
  build stores) is inside the bound -- in the grid family: EQUAL to the fp64 reference / its bf16 rounding, at every shape used --
  and nine deliberately wrong evaluations are rejected at every ragged small shape, in both families;
* the hooks refuse what no kernel supports, with the library's status codes, before any launch (the pointers are fake and never
  dereferenced); tools/trunk_hooks_hostcheck.hip (run by test_hr_tail_host.py's `make hooks_hostcheck`) records what the accepted
  calls hand to the launchers."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import hr_tail_common as T
import trunk_common as R
from oracle import basicvsr_oracle as O

BADARG, UNSUPPORTED = -1, -2
F32, BF16 = 0, 1
A = [0x10000000 + 0x1000000 * i for i in range(12)]        # 256-byte aligned, never dereferenced


def _close(a, b, tol=1e-10):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _randn(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


# --------------------------------------------------------------------------------------------------------------------
# the references
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 4, 34)], ids=T.sid)
def test_residual_blocks_and_their_gradients_are_pinned_to_autograd_on_the_oracle(shape):
    """Two frames through the same two residual blocks behind a LeakyReLU stem output: the chain's layer list, layer by layer, the masked
    data gradients (ReLU mask from A_b, LeakyReLU mask from the stem's output with the residual inside) and the two-segment weight
    gradients, against autograd on ``residual_conv``."""
    n, h, w = shape
    nb, C = 2, 64
    c = R.case("chain", shape, blocks=nb)
    t = {k: v.double() for k, v in R.inputs_of(c).items()}
    sd = {}
    for b in range(nb):
        for j in (1, 2):
            sd[f"res_block.{b}.conv{j}.weight"] = t["w"][2 * b + j - 1].clone().requires_grad_(True)
            sd[f"res_block.{b}.conv{j}.bias"] = t["bias"][2 * b + j - 1].clone().requires_grad_(True)
    fwd, bwd = R.chain_layers(nb)
    assert [L[0] for L in fwd] == [0, 1, 0, 1] and [L[0] for L in bwd] == [2, 1, 2] and [L[2] for L in bwd] == ["da1", "dx1", "da0"]
    frames = []
    for s in range(2):
        p = T.draw_aux(70 + s, n, h, w).double().requires_grad_(True)      # the stem's pre-activation
        cot = T.draw(80 + s, n, C, h, w).double()
        xs = [F.leaky_relu(p, T.SLOPE)]
        pre = []
        for b in range(nb):
            xs[-1].retain_grad()
            q = F.conv2d(xs[-1], sd[f"res_block.{b}.conv1.weight"], sd[f"res_block.{b}.conv1.bias"], padding=1)
            q.retain_grad()
            pre.append(q)
            # the block written out, so that conv1's pre-activation is a node of the graph; its value is the oracle's
            nxt = xs[-1] + F.conv2d(F.relu(q), sd[f"res_block.{b}.conv2.weight"], sd[f"res_block.{b}.conv2.bias"], padding=1)
            assert _close(nxt.detach(), O.residual_conv(sd, f"res_block.{b}.", xs[-1]).detach())
            xs.append(nxt)
        (xs[-1] * cot).sum().backward()
        img = {"x0": xs[0].detach(), f"dx{nb}": cot}
        for L in fwd:
            img[L[2]] = R.chain_layer_eval(c, L, img, False)
        for L in bwd:
            img[L[2]] = R.chain_layer_eval(c, L, img, True)
        for b in range(nb):
            assert _close(img[f"x{b + 1}"], xs[b + 1].detach()) and _close(img[f"a{b}"], F.relu(pre[b].detach()))
            assert _close(img[f"da{b}"], pre[b].grad)
        assert _close(img["dx1"], xs[1].grad)
        # (dgrad(conv1 of block 0)(dA_0) + dX_1) x LeakyReLU'(stem output): the gradient of the stem's pre-activation
        g0 = R.conv_layer(img["da0"], t["w"][0], None, img["dx1"], img["x0"], act=0, mask_mode=2, mode=1)
        assert _close(g0, p.grad)
        frames.append(img)
    for b in range(nb):
        for j, (xk, dk) in ((1, (f"x{b}", f"da{b}")), (2, (f"a{b}", f"dx{b + 1}"))):
            g = R._ops(R.case("wgrad_cc", shape, nseg=2), dict(x=torch.stack([f[xk] for f in frames]), dy=torch.stack([f[dk] for f in frames]),
                                                               gw0=torch.zeros(C, 2 * C, 3, 3, dtype=torch.float64), gb0=torch.zeros(C, dtype=torch.float64)))
            assert _close(g["gw"], sd[f"res_block.{b}.conv{j}.weight"].grad) and _close(g["gb"], sd[f"res_block.{b}.conv{j}.bias"].grad)


@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 4, 34)], ids=T.sid)
def test_stem_and_fusion_conv_are_pinned_to_autograd(shape, C):
    n, h, w = shape
    wt, b = T.draw(1, C, C + 3, 3, 3).double().requires_grad_(True), _randn(2, C).requires_grad_(True)
    lr = [T.draw(3 + s, n, 3, h, w).double().requires_grad_(True) for s in range(2)]
    feat = [None, T.draw(6, n, C, h, w).double().requires_grad_(True)]      # the first frame of a direction has the zero state
    cot = [T.draw(8 + s, n, C, h, w).double() for s in range(2)]
    pres = _randn(10, n, 3, h, w)
    sd = {"conv.0.weight": wt, "conv.0.bias": b}
    loss, ys, pre = 0, [], []
    for s in range(2):
        x = torch.cat([lr[s], feat[s] if feat[s] is not None else torch.zeros(n, C, h, w, dtype=torch.float64)], 1)
        ys.append(O.residual_block(sd, "", x, 0))
        q = F.conv2d(x, wt, b, padding=1)
        q.retain_grad()
        pre.append(q)
        loss = loss + (F.leaky_relu(q, T.SLOPE) * cot[s]).sum()
    loss.backward()
    k = lambda hook, **o: R.case(hook, shape, C=C, **o)
    tw = dict(w=wt.detach(), bias=b.detach())
    # (slope: the oracle's double 0.1; the kernels hold float(0.1), which the cases use by default)
    assert _close(R._ops(k("stem", feat=0, slope=0.1), dict(lr=lr[0].detach(), feat=None, **tw))["y"], ys[0].detach())
    assert _close(R._ops(k("stem", slope=0.1), dict(lr=lr[1].detach(), feat=feat[1].detach(), **tw))["y"], ys[1].detach())
    assert _close(R._ops(k("stem"), dict(lr=lr[1].detach(), feat=feat[1].detach(), **tw))["y"], F.leaky_relu(pre[1].detach(), T.SLOPE))
    g0 = [q.grad for q in pre]
    d = R._ops(k("stem_dgrad", accumulate=1), dict(g0=g0[1], w=wt.detach(), pres=pres))
    assert _close(d["dfeat"], feat[1].grad) and _close(d["dlr"], lr[1].grad + pres)
    assert _close(R._ops(k("stem_dgrad", accumulate=0), dict(g0=g0[0], w=wt.detach(), pres=pres))["dlr"], lr[0].grad)
    zero = dict(gw0=torch.zeros(C, C + 3, 3, 3, dtype=torch.float64), gb0=torch.zeros(C, dtype=torch.float64))
    g = R._ops(k("stem_wgrads", nseg=2), dict(lr=torch.stack([v.detach() for v in lr]), feat=feat[1].detach()[None], g0=torch.stack(g0), **zero))
    assert _close(g["gw"], wt.grad) and _close(g["gb"], b.grad)
    # the stem on the planar frames alone (the pre-clean stack): the first three input channels
    w3 = wt.detach()[:, :3].clone().requires_grad_(True)
    (F.conv2d(lr[0].detach(), w3, padding=1) * cot[0]).sum().backward()
    g = R._ops(k("stem_wgrads", cat=0, nseg=1), dict(lr=lr[0].detach()[None], g0=cot[0][None], gw0=zero["gw0"], gb0=zero["gb0"]))
    assert _close(g["gw"], w3.grad)
    # the 1x1 fusion conv on cat([a, b]), two frames
    pw, pb = T.draw(20, C, 2 * C, 1, 1).double().requires_grad_(True), _randn(21, C).requires_grad_(True)
    fa = [T.draw(22 + s, n, C, h, w).double().requires_grad_(True) for s in range(2)]
    fb = [T.draw(24 + s, n, C, h, w).double().requires_grad_(True) for s in range(2)]
    loss, pre = 0, []
    for s in range(2):
        q = F.conv2d(torch.cat([fa[s], fb[s]], 1), pw, pb)
        q.retain_grad()
        pre.append(q)
        y = F.leaky_relu(q, T.SLOPE)
        assert _close(R._ops(k("point"), dict(a=fa[s].detach(), b=fb[s].detach(), w=pw.detach(), bias=pb.detach()))["y"], y.detach())
        loss = loss + (y * cot[s]).sum()
    loss.backward()
    for s in range(2):
        d = R._ops(k("point", backward=1), dict(a=pre[s].grad, w=pw.detach()))
        assert _close(d["d0"], fa[s].grad) and _close(d["d1"], fb[s].grad)
    gw = torch.zeros(C, 2 * C, 1, 1, dtype=torch.float64)
    for half, xs in ((0, fa), (1, fb)):                    # recon_point_wgrads: one launch per half, both accumulating into the same tensor
        out = R._ops(k("wgrad_cc", ks=1, nseg=2, accumulate=1, i_off=half * C, I_total=2 * C, gb=half == 0),
                     dict(x=torch.stack([v.detach() for v in xs]), dy=torch.stack([q.grad for q in pre]), gw0=gw, gb0=torch.zeros(C, dtype=torch.float64)))
        gw = out["gw"]
        if half == 0:
            assert _close(out["gb"], pb.grad)
    assert _close(gw, pw.grad)


# --------------------------------------------------------------------------------------------------------------------
# the criterion
# --------------------------------------------------------------------------------------------------------------------
DISTINCT = R.distinct(R.gpu_cases())


def test_the_case_list_covers_every_hook_shape_width_and_dtype():
    hooks = {"conv", "stem", "stem_dgrad", "point", "wgrad_cc", "stem_wgrads"}
    cs = R.gpu_cases()
    for s in R.SHAPES:
        for hk in hooks:
            dts = {(c.dtype, c.o("family")) for c in cs if c.hook == hk and c.shape == s and c.o("C") == 64}
            want = {(d, f) for d in ("bf16", "fp32") for f in ("rand", "grid")}
            assert dts == (want if (s != R.WIDE or hk in ("conv", "wgrad_cc")) else set()), (hk, s, dts)
    for C in (16, 32):
        assert {c.shape for c in cs if c.o("C") == C} == set(R.SMALL) and {c.hook for c in cs if c.o("C") == C} == hooks
    wg = [c for c in cs if c.hook == "wgrad_cc"]
    assert {c.o("nseg") for c in wg} == {1, 3, 8} and {c.o("accumulate") for c in wg} == {0, 1} and {c.o("i_off", 0) for c in wg if c.o("C") == 64} == {0, 64}
    tiles = lambda s: s[0] * ((s[1] + 7) // 8) * ((s[2] + 31) // 32)
    assert {tiles(c.shape) & 1 for c in wg} == {0, 1}                                              # an odd and an even tile count
    assert any(c.shape == R.BIG and c.o("nseg") == 3 and c.o("family") == "grid" for c in wg)
    assert all(c.o("act", 0) != 2 and c.o("mask_mode", 1) != 2 for c in cs if c.o("family") == "grid")      # ReLU or nothing, ReLU masks only
    assert not any(c.hook == "point" and c.o("family") == "grid" and not c.o("backward", 0) for c in cs)      # LeakyReLU's 0.1 is not exact
    assert {c.o("blocks") for s in R.SHAPES for c in R.chain_cases(s)} == {2, 3}


@pytest.mark.parametrize("shape", R.SHAPES, ids=T.sid)
def test_same_precision_emulation_is_inside_the_bound_and_mutations_are_outside(shape):
    """Per shape: every distinct GPU case's emulation (fp32, reversed summation order) passes check() -- in the grid family that is
    bit-equality with the fp64 reference or its bf16 rounding.  At a ragged small shape every applicable mutation of a case falls
    outside the bound in the rand family or breaks exactness in the grid family of the same case (at K ~ 10^4 the bound of a
    multi-segment weight gradient exceeds a pre-filled gradient of O(1): there the grid family alone sees `accumulate` overwriting),
    with one stated exception: `tap_mirrored` exchanges taps (1, 0) and (1, 2), which an image one pixel wide never meets."""
    cases = [c for c in DISTINCT if c.shape == shape]
    assert cases
    rejected = {}
    for c in cases:
        plain = R.emulate(c)
        R.check(c, plain, label="emulation")
        if shape not in R.SMALL or not T.ragged(shape) or c.dtype != "bf16" and c.o("C") != 64:
            continue
        key = (c.hook, c.dtype, tuple((k, v) for k, v in c.opts if k != "family"))
        for mut in R.MUTATIONS:
            if R.applicable(c, mut):
                rejected[key, mut] = rejected.get((key, mut), False) or not R.passes(c, R.emulate(c, mut))
            elif mut == "tap_mirrored" and c.o("ks", 3) == 3 and c.hook != "point":
                assert T.same_bits(R.emulate(c, mut), plain), c.name
    assert all(rejected.values()), [k for k, v in rejected.items() if not v]
    if shape in R.SMALL and T.ragged(shape):
        assert {m for _, m in rejected} == set(R.MUTATIONS) - ({"tap_mirrored"} if shape[2] < 2 else set()), shape


@pytest.mark.parametrize("shape", R.SHAPES, ids=T.sid)
def test_chain_emulation_passes_layer_by_layer_and_mutations_fail(shape):
    """The chains of test_trunk_gpu.py with every image rounded to bf16 as the kernel stores it: each layer inside the bound against
    fp64 on its stored inputs (grid family: equal); a residual taken from the layer's input, a mirrored tap, a halo read beyond W and a
    `>= 0` mask each fail at the ragged small shapes."""
    for c in R.chain_cases(shape):
        R.check_chain(c, R.emulate_chain(c), label="emulation")
        if T.ragged(shape) and shape in R.SMALL:
            for mut in ("res_from_layer_input", "tap_mirrored", "halo_reads_beyond_w", "mask_ge"):
                if mut == "tap_mirrored" and shape[2] < 2:
                    continue
                m = R.measure_chain(c, R.emulate_chain(c, mut))
                assert any(not v[0] <= 1.0 for v in m.values()), (c.name, mut)


def test_a_nan_an_untouched_sentinel_or_a_touched_neighbour_fails_the_check():
    c = R.case("conv", (1, 3, 5), mode=1, bias=False, mask="aux", mask_mode=1)
    good = R.emulate(c)
    assert R.passes(c, good)
    for bad in (float("nan"), T.SENTINEL):
        g = {"y": good["y"].clone()}
        g["y"][0, 5, 1, 2] = bad
        assert not R.passes(c, g)
    g = {"y": good["y"].clone()}
    g["y"][tuple((R.inputs_of(c)["aux"] <= 0).nonzero()[0])] = 1e-30      # a ReLU-masked element has the bound 0
    assert not R.passes(c, g)
    c = R.case("wgrad_cc", (1, 3, 5), ks=1, nseg=2, accumulate=1, i_off=64, I_total=128, gb=False)
    g = R.emulate(c)
    assert R.passes(c, g)
    g["gw"][3, 5, 0, 0] += 2.0 ** -20                       # the half the launch must leave alone
    assert not R.passes(c, g)
    c = R.case("wgrad_cc", (1, 9, 31), nseg=3, accumulate=1, family="grid")
    g = R.emulate(c)
    assert R.passes(c, g)
    g["gw"][0, 0, 1, 1] += 0.25                             # the grid family holds no slack at all
    assert not R.passes(c, g)


# --------------------------------------------------------------------------------------------------------------------
# the hooks' argument checks
# --------------------------------------------------------------------------------------------------------------------
def _lib():
    from vsrlab_amd import _lib
    return _lib.load()


def test_hooks_refuse_what_no_kernel_supports_before_any_launch():
    lib = _lib()
    X, W_, B, WP, Y, RES, AUX, SO, SB, GW, GB, SL = A
    n, h, w = 2, 8, 12
    segs = (ctypes.c_void_p * 9)(*[X + 4096 * i for i in range(9)])
    hole = (ctypes.c_void_p * 3)(X, 0, X + 8192)

    def conv(**k):
        a = dict(dtype=BF16, C=64, ks=3, mode=0, x=X, w=W_, bias=B, wpack=WP, y=Y, act=0, res=None, aux=None, mask=0, so=None, sb=None, make=0, unsh=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_conv(a["dtype"], a["C"], a["ks"], a["mode"], a["x"], a["w"], a["bias"], a["wpack"], a["y"], a["act"], 0.1, a["res"], a["aux"],
                                        a["mask"], a["so"], a["sb"], a["make"], a["unsh"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(C=48), dict(C=128), dict(ks=5), dict(ks=2), dict(mode=2), dict(x=None), dict(w=None), dict(wpack=None), dict(y=None), dict(act=3),
              dict(act=-1), dict(mask=1), dict(aux=AUX), dict(aux=AUX, mask=3), dict(sb=SB), dict(aux=AUX, mask=1, make=1), dict(unsh=1, h=7), dict(unsh=1, w_=11),
              dict(unsh=1, ks=1), dict(n=0), dict(h=0), dict(w_=0)):
        assert conv(**k) == BADARG, k
    for k in (dict(dtype=F32, act=1, so=SO), dict(C=32, act=1, so=SO), dict(C=16, aux=AUX, mask=1, sb=SB), dict(dtype=F32, aux=AUX, mask=1, sb=SB, make=1),
              dict(ks=1, act=1, so=SO), dict(so=SO), dict(act=1, so=SO, res=RES), dict(act=1, so=SO, aux=AUX, mask=1), dict(dtype=F32, unsh=1), dict(C=32, unsh=1),
              dict(unsh=1, aux=AUX, mask=1), dict(unsh=1, aux=AUX, mask=2, sb=SB)):
        assert conv(**k) == UNSUPPORTED, k                 # sign bits and phase planes: bf16 at 64 channels only; no kernel masks phase planes

    def stem(**k):
        a = dict(dtype=BF16, C=64, cat=1, feat=X, lr=Y, ns=3 * h * w, w=W_, bias=B, wpack=WP, y=RES, act=2, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_stem(a["dtype"], a["C"], a["cat"], a["feat"], a["lr"], a["ns"], a["w"], a["bias"], a["wpack"], a["y"], a["act"], 0.1,
                                        a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=3), dict(C=8), dict(cat=2), dict(lr=None), dict(w=None), dict(wpack=None), dict(y=None), dict(ns=3 * h * w - 1), dict(act=1), dict(cat=0),
              dict(n=0), dict(h=0), dict(w_=0)):
        assert stem(**k) == BADARG, k

    def sdg(**k):
        a = dict(dtype=BF16, C=64, cat=1, g0=X, w=W_, wpack=WP, dfeat=Y, dlr=RES, ns=3 * h * w, acc=1, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_stem_dgrad(a["dtype"], a["C"], a["cat"], a["g0"], a["w"], a["wpack"], a["dfeat"], a["dlr"], a["ns"], a["acc"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(C=24), dict(cat=-1), dict(g0=None), dict(w=None), dict(wpack=None), dict(dfeat=None, dlr=None), dict(cat=0), dict(ns=3 * h * w - 1),
              dict(acc=2), dict(n=0), dict(h=0), dict(w_=0)):
        assert sdg(**k) == BADARG, k

    def point(**k):
        a = dict(dtype=BF16, C=64, back=0, a=X, b=Y, w=W_, bias=B, wpack=WP, y0=RES, y1=None, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_point(a["dtype"], a["C"], a["back"], a["a"], a["b"], a["w"], a["bias"], a["wpack"], a["y0"], a["y1"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(C=0), dict(back=2), dict(a=None), dict(b=None), dict(w=None), dict(wpack=None), dict(y0=None), dict(y1=AUX), dict(back=1),
              dict(back=1, b=None, bias=None), dict(back=1, bias=None, y1=AUX), dict(n=0), dict(h=0), dict(w_=0)):
        assert point(**k) == BADARG, k

    def wg(**k):
        a = dict(dtype=BF16, C=64, ks=3, x=segs, dy=segs, nseg=3, gw=GW, it=64, io=0, gb=GB, acc=0, slab=SL, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_wgrad_cc(a["dtype"], a["C"], a["ks"], a["x"], a["dy"], a["nseg"], a["gw"], a["it"], a["io"], a["gb"], a["acc"], a["slab"],
                                            a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(C=48), dict(ks=2), dict(x=None), dict(dy=None), dict(nseg=0), dict(nseg=9), dict(nseg=-1), dict(x=hole), dict(dy=hole), dict(gw=None),
              dict(slab=None), dict(it=63), dict(it=127, io=64), dict(io=-1, it=128), dict(acc=2), dict(n=0), dict(h=0), dict(w_=0)):
        assert wg(**k) == BADARG, k

    def swg(**k):
        a = dict(dtype=BF16, C=64, cat=1, lr=segs, xns=3 * h * w, g0=segs, nseg=3, feat=segs, g0f=segs, nf=2, gw=GW, gb=GB, acc=1, slab=SL, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_stem_wgrads(a["dtype"], a["C"], a["cat"], a["lr"], a["xns"], a["g0"], a["nseg"], a["feat"], a["g0f"], a["nf"], a["gw"], a["gb"],
                                               a["acc"], a["slab"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(C=48), dict(cat=2), dict(lr=None), dict(g0=None), dict(nseg=0), dict(nseg=9), dict(nf=4), dict(nf=-1), dict(cat=0), dict(feat=None),
              dict(g0f=None), dict(lr=hole), dict(feat=hole), dict(xns=3 * h * w - 1), dict(gw=None), dict(slab=None), dict(acc=-1), dict(n=0), dict(h=0), dict(w_=0)):
        assert swg(**k) == BADARG, k

    layers = (ctypes.c_uint * 16)(1, 2, R.NONE, R.NONE, 7, 20, 30, 0, 2, 3, 1, R.NONE, R.NONE, 21, 31, 1)
    now = (ctypes.c_uint * 8)(1, 2, R.NONE, R.NONE, R.NONE, R.NONE, R.NONE, 0)
    wl = (ctypes.c_void_p * 2)(W_, W_ + 4096)

    def chain(**k):
        a = dict(dtype=BF16, C=64, base=X, sync=Y, layers=layers, nl=2, w=wl, mode=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_trunk_chain(a["dtype"], a["C"], a["base"], a["sync"], a["layers"], a["nl"], a["w"], a["mode"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(C=48), dict(base=None), dict(base=X + 16), dict(sync=None), dict(layers=None), dict(nl=0), dict(nl=65), dict(mode=2),
              dict(layers=now, nl=1), dict(n=0), dict(h=0), dict(w_=0)):
        assert chain(**k) == BADARG, k
    for k in (dict(dtype=F32), dict(C=32), dict(C=16)):
        assert chain(**k) == UNSUPPORTED, k                # chains: the persistent 64-channel bf16 kernel only
