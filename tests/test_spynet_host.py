"""CPU side of the SPyNet harness (tests/spynet_common.py, csrc/spynet_hooks.hip):

* the fp64 restatements that test_spynet_gpu.py measures the kernels against are pinned at 1e-10 to torch fp64 autograd on the oracle's own
  SPyNet pieces: the ConvReLU stack; ``flow_warp`` with border padding (``F.grid_sample`` too: its ``clip_coordinates_set_grad``); the x2
  ``align_corners=True`` upsample times 2; the /32 resize with the u / v rescale; ``avg_pool2d``; the normalisation;
* the criterion is dry-run: over every GPU case an fp32 evaluation -- the 7x7 sums in reversed order, every sample coordinate computed in fp32
  by the kernel's formula -- is inside the bound (grid family: EQUAL to the reference or its bf16 rounding), and fourteen deliberately
  wrong evaluations are rejected at every small shape where they are observable, each at two shapes at least; where a mutation is
  not observable (spynet_common.MUTATION_NOTES) it changes no bit;
* the hooks refuse what no kernel supports, with the library's status codes, before any launch (the pointers are fake and never
  dereferenced); tools/spynet_hooks_hostcheck.hip records what the accepted calls hand to the launchers (built plain here; `make
  hooks_hostcheck` runs it under ASan / UBSan)."""
import pytest
import torch
import torch.nn.functional as F

import hr_tail_common as T
import spynet_common as S
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
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 2, 2), (1, 4, 34)], ids=T.sid)
def test_the_conv_relu_stack_and_its_gradients_are_pinned_to_autograd_on_the_oracle(shape):
    """The five layers of a level, ReLU behind each: forward layer by layer, the data gradients masked by the stored input of the layer
    (the previous ReLU's output), the last layer's gradient through spynet_dres's mask, and the weight and bias gradients."""
    n, h, w = shape
    sd = {}
    for j in range(5):
        sd[f"basic_module.0.basic_module.{j}.conv.0.weight"] = (T.draw(40 + j, S.CO[j], S.CI[j], 7, 7).double() / (7 * S.CI[j] ** 0.5)).requires_grad_(True)
        sd[f"basic_module.0.basic_module.{j}.conv.0.bias"] = (_randn(50 + j, S.CO[j]) * 0.1).requires_grad_(True)
    x0 = T.draw(60, n, 8, h, w).double().requires_grad_(True)
    fup, cot = _randn(61, n, 2, h, w), _randn(62, n, 2, h, w)
    xs, pre = [x0], []
    for j in range(5):
        q = F.conv2d(xs[-1], sd[f"basic_module.0.basic_module.{j}.conv.0.weight"], sd[f"basic_module.0.basic_module.{j}.conv.0.bias"], padding=3)
        q.retain_grad()
        pre.append(q)
        y = F.relu(q)
        y.retain_grad()
        xs.append(y)
    assert _close(xs[-1].detach(), O._spynet_level(sd, "", 0, x0).detach())      # the stack written out is the oracle's
    ((fup + xs[-1]) * cot).sum().backward()
    k = lambda hook, **o: S.case(hook, shape, **o)
    wb = lambda j: (sd[f"basic_module.0.basic_module.{j}.conv.0.weight"], sd[f"basic_module.0.basic_module.{j}.conv.0.bias"])
    for j in range(5):
        wt, b = wb(j)
        got = S._ops7(k("conv", j=j, act=1, pres=int(j == 4)), dict(x=xs[j].detach(), w=wt.detach(), bias=b.detach(), pres=fup))["y"]
        assert _close(got, (xs[j + 1].detach() + fup) if j == 4 else xs[j + 1].detach())
    # flow = flow_up + ReLU(conv5): the cotangent of conv5's pre-activation is spynet_dres(dflow, res = the stored ReLU output)
    dres = S._ops_planar(S.case("dres", shape), dict(d=cot, res=xs[5].detach()))["y"]
    assert _close(dres[:, :2], pre[4].grad) and not bool(dres[:, 2:].any())
    dy = pre[4].grad
    zero = lambda j: dict(gw0=torch.zeros(S.CO[j], S.CI[j], 7, 7, dtype=torch.float64), gb0=torch.zeros(S.CO[j], dtype=torch.float64))
    for j in range(4, -1, -1):
        wt, b = wb(j)
        g = S._ops7(k("wgrad", j=j), dict(x=xs[j].detach(), dy=dy, **zero(j)))
        assert _close(g["gw"], wt.grad) and _close(g["gb"], b.grad)
        if j > 0:
            dy = S._ops7(k("dgrad", j=j, aux=1), dict(dy=dy, w=wt.detach(), aux=xs[j].detach()))["dx"]
            assert _close(dy, pre[j - 1].grad)
        else:
            assert _close(S._ops7(k("dgrad", j=0), dict(dy=dy, w=wt.detach()))["dx"], x0.grad)
    # the canonical network: no ReLU behind the last conv, no mask in spynet_dres
    wt, b = wb(4)
    assert _close(S._ops7(k("conv", j=4, act=0, pres=1), dict(x=xs[4].detach(), w=wt.detach(), bias=b.detach(), pres=fup))["y"], pre[4].detach() + fup)
    assert _close(S._ops_planar(S.case("dres", shape, res=0), dict(d=cot, res=xs[5].detach()))["y"][:, :2], cot)


def _grid_sample_border(img, flow):
    n, c, h, w = img.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=img.dtype), torch.arange(w, dtype=img.dtype), indexing="ij")
    gx = 2.0 * (xs + flow[:, 0]) / max(w - 1, 1) - 1.0
    gy = 2.0 * (ys + flow[:, 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(img, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=True)


@pytest.mark.parametrize("pairs", S.PAIRS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
@pytest.mark.parametrize("size", [(2, 2), (2, 6), (6, 2), (4, 4), (8, 16), (10, 14)], ids=T.sid)
def test_prepare_and_its_adjoint_are_pinned_to_autograd(size, pairs):
    """x16 = cat([ref, flow_warp(supp, flow_up, border), flow_up]) with flow_up = 2 x the align_corners=True upsample, for the pairs of
    basicvsr.py:32-35 (pair_mode 0) and for [refs, supps] (pair_mode 1): the values against the oracle's flow_warp and F.grid_sample; the
    gradients towards the flow below and towards the frames against autograd through F.grid_sample (clip_coordinates_set_grad), also
    without the frames' gradient and -- level 0 -- without a flow."""
    h, w = size
    c = S.case("prepare", (1, h, w), **pairs)
    P, Fr = S.npairs(c), S.nframes(c)
    c = S.case("prepare", (P, h, w), **pairs)
    frames = _randn(1, Fr, 3, h, w).requires_grad_(True)
    flow_prev = (_randn(2, P, 2, h // 2, w // 2) * 1.5).requires_grad_(True)
    dx16, dflow_l = _randn(3, P, 8, h, w), _randn(4, P, 2, h, w)
    if pairs["pair_mode"]:
        ref, supp = frames[:P], frames[P:]
    else:
        n, t = pairs["n"], pairs["t"]
        lrs = frames.view(n, t, 3, h, w)
        l1, l2 = lrs[:, :-1].reshape(-1, 3, h, w), lrs[:, 1:].reshape(-1, 3, h, w)
        ref, supp = torch.cat([l1, l2]), torch.cat([l2, l1])      # backward flows first (ref = frame i), then forward (ref = frame i + 1)
    fu = F.interpolate(flow_prev, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
    warped = _grid_sample_border(supp, fu)
    assert _close(warped.detach(), O.flow_warp(supp.detach(), fu.detach(), "border"))
    x16 = torch.cat([ref, warped, fu], 1)
    ((x16 * dx16).sum() + (fu * dflow_l).sum()).backward()
    got = S._prepare(c, dict(frames=frames.detach(), flow_prev=flow_prev.detach()))
    assert _close(got["flow_up"], fu.detach()) and _close(got["x16"][:, :8], x16.detach()) and not bool(got["x16"][:, 8:].any())
    t = dict(frames=frames.detach(), flow_up=fu.detach(), dx16=dx16, dflow_l=dflow_l, dprev0=_randn(5, P, 2, h // 2, w // 2), dframes0=_randn(6, Fr, 3, h, w))
    both = S._prepare_bwd(S.case("prepare_bwd", (P, h, w), **pairs), t)
    assert _close(both["dflow_prev"], flow_prev.grad + t["dprev0"]) and _close(both["dframes"], frames.grad + t["dframes0"])
    only = S._prepare_bwd(S.case("prepare_bwd", (P, h, w), dframes=0, **pairs), t)
    assert set(only) == {"dflow_prev"} and _close(only["dflow_prev"], both["dflow_prev"])
    # level 0: flow_up = 0, nothing below
    fr0 = frames.detach().clone().requires_grad_(True)
    sel = lambda v: ((v[:P], v[P:]) if pairs["pair_mode"] else (lambda l: (torch.cat([l[:, :-1].reshape(-1, 3, h, w), l[:, 1:].reshape(-1, 3, h, w)]),
                                                                           torch.cat([l[:, 1:].reshape(-1, 3, h, w), l[:, :-1].reshape(-1, 3, h, w)])))(v.view(pairs["n"], pairs["t"], 3, h, w)))
    r0, s0 = sel(fr0)
    z = torch.zeros(P, 2, h, w, dtype=torch.float64)
    x0 = torch.cat([r0, _grid_sample_border(s0, z), z], 1)
    (x0 * dx16).sum().backward()
    c0 = S.case("prepare", (P, h, w), level0=1, **pairs)
    g0 = S._prepare(c0, dict(frames=frames.detach(), flow_prev=None))
    assert _close(g0["x16"][:, :8], x0.detach()) and not bool(g0["flow_up"].any())
    b0 = S._prepare_bwd(S.case("prepare_bwd", (P, h, w), level0=1, **pairs), t)
    assert set(b0) == {"dframes"} and _close(b0["dframes"], fr0.grad + t["dframes0"])


@pytest.mark.parametrize("src,dst", S.RESIZES + [((5, 7), (32, 32))], ids=lambda v: T.sid(v))
def test_resizes_pool_and_normalisation_are_pinned_to_autograd(src, dst):
    (h, w), (hu, wu) = src, dst
    mean, std = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64), torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)
    k = lambda hook: S.case(hook, (2, h, w), hu=hu, wu=wu)
    x = _randn(1, 2, 3, h, w).requires_grad_(True)
    y = (F.interpolate(x, size=(hu, wu), mode="bilinear", align_corners=False) - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    d, out0 = _randn(2, 2, 3, hu, wu), _randn(3, 2, 3, h, w)
    (y * d).sum().backward()
    assert _close(S._ops_planar(k("resize_norm"), dict(x=x.detach(), mean=mean, std=std))["y"], y.detach())
    assert _close(S._ops_planar(k("resize_norm_bwd"), dict(d=d, out0=out0, mean=mean, std=std))["y"], x.grad + out0)
    # the flow at the /32 size back to (h, w), u scaled by w / wu, v by h / hu (spynet.py:83-91; the oracle's spynet_forward)
    fl = _randn(4, 2, 2, hu, wu).requires_grad_(True)
    out = F.interpolate(fl, size=(h, w), mode="bilinear", align_corners=False) * torch.tensor([w / wu, h / hu], dtype=torch.float64).view(1, 2, 1, 1)
    d, out0 = _randn(5, 2, 2, h, w), _randn(6, 2, 2, hu, wu)
    (out * d).sum().backward()
    assert _close(S._ops_planar(k("flow_out"), dict(x=fl.detach()))["y"], out.detach())
    assert _close(S._ops_planar(k("flow_out_bwd"), dict(d=d, out0=out0))["y"], fl.grad + out0)
    # avg_pool2d at the /32 size, and the fp32 add
    p = _randn(7, 6, hu, wu).requires_grad_(True)
    q = F.avg_pool2d(p, 2, 2)
    d, out0 = _randn(8, 6, hu // 2, wu // 2), _randn(9, 6, hu, wu)
    (q * d).sum().backward()
    assert _close(S._ops_planar(S.case("avgpool2", (6, hu, wu)), dict(x=p.detach()))["y"], q.detach())
    assert _close(S._ops_planar(S.case("avgpool2_bwd", (6, hu, wu)), dict(d=d, out0=out0))["y"], p.grad + out0)
    assert _close(S._ops_planar(S.case("add", (6, hu, wu)), dict(a=out0, b=p.detach()))["y"], out0 + p.detach())


# --------------------------------------------------------------------------------------------------------------------
# the criterion
# --------------------------------------------------------------------------------------------------------------------
DISTINCT = S.distinct(S.gpu_cases())
LARGE = (S.BIG, S.DEEP, S.WG_MANY)


def test_the_case_list_covers_every_launch_shape_and_dtype():
    cs = S.gpu_cases()
    for hook in S.CONV_HOOKS:
        mine = [c for c in cs if c.hook == hook]
        assert {c.shape for c in mine} == set(S.conv_shapes(hook)) and {c.o("j") for c in mine} == set(range(5))
        for s in S.SMALL + [S.BIG]:
            assert {(c.dtype, c.o("family")) for c in mine if c.shape == s} == {(d, f) for d in ("bf16", "fp32") for f in ("rand", "grid")}, (hook, s)
    assert {(c.dtype, c.o("family")) for c in cs if c.shape == S.DEEP} == {("bf16", "grid")} and {c.hook for c in cs if c.shape == S.DEEP} == {"conv", "dgrad"}
    assert all(c.o("aux") for c in cs if c.shape == S.DEEP and c.hook == "dgrad")
    assert {(c.hook, c.o("family"), c.o("accumulate")) for c in cs if c.shape == S.WG_MANY} == {("wgrad", "grid", 1)}
    conv = [c for c in cs if c.hook == "conv" and c.o("j") == 4]
    assert {(c.o("act"), c.o("pres", 0)) for c in conv if c.shape == (1, 1, 1)} == {(1, 1), (0, 1), (1, 0), (0, 0)}
    dg = [c for c in cs if c.hook == "dgrad" and c.shape == (1, 2, 2)]
    assert {(c.o("j"), c.o("aux", 0)) for c in dg} >= {(0, 0), (1, 1), (2, 1), (3, 1), (4, 1), (2, 0)}
    wg = [c for c in cs if c.hook == "wgrad" and c.shape == (2, 13, 37)]
    assert {c.o("accumulate") for c in wg} == {0, 1} and {c.o("gb", True) for c in wg} == {True, False}
    pb = [c for c in cs if c.hook == "prepare_bwd"]
    assert {(c.o("level0", 0), c.o("dframes", 1)) for c in pb} == {(1, 1), (0, 1), (0, 0)}
    for hook in ("prepare", "prepare_bwd"):
        mine = [c for c in cs if c.hook == hook]
        assert {c.shape[1:] for c in mine if c.o("level0", 0)} == set(S.LEVEL0) and {c.shape[1:] for c in mine if not c.o("level0", 0)} == set(S.LEVELS)
        assert {(c.o("pair_mode"), c.shape[0]) for c in mine} == {(0, 2), (0, 8), (1, 1), (1, 3)}
    assert {c.o("res", 1) for c in cs if c.hook == "dres"} == {0, 1}
    for hook in ("resize_norm", "resize_norm_bwd", "flow_out", "flow_out_bwd"):
        assert {(c.shape[1:], (c.o("hu"), c.o("wu"))) for c in cs if c.hook == hook} == set(S.RESIZES)
    assert {c.hook for c in cs} == set(S.CONV_HOOKS + S.PLANAR_OPS + ("prepare", "prepare_bwd", "dres"))


def test_the_emulation_is_inside_the_bound_and_every_mutation_is_rejected_where_it_is_observable():
    """Over every distinct small GPU case: the unmutated fp32 emulation passes check() (grid family: bit-equality with the reference or its
    bf16 rounding).  Each applicable mutation of a case is rejected in the rand or in the grid family of that case (a ReLU on a last layer
    whose two outputs happen to be positive at (1,1,1) is seen by the other family).  A mutation that spynet_common.applicable() calls
    not observable at a shape changes no bit there.  Every mutation is rejected at two shapes at least."""
    rejected, shapes = {}, {}
    for c in DISTINCT:
        if c.shape in LARGE:
            continue
        plain = S.emulate(c)
        S.check(c, plain, label="emulation")
        if c.dtype != "bf16":
            continue
        key = (c.hook, c.shape, tuple((k, v) for k, v in c.opts if k != "family"))
        for mut in S.MUTATIONS:
            if S.applicable(c, mut):
                rejected[key, mut] = rejected.get((key, mut), False) or not S.passes(c, S.emulate(c, mut))
            else:
                assert T.same_bits(S.emulate(c, mut), plain), (c.name, mut, "not observable here, yet it changes the result")
    assert all(rejected.values()), [k for k, v in rejected.items() if not v]
    for (key, mut), _ in rejected.items():
        shapes.setdefault(mut, set()).add(key[1][1:] if key[0] not in S.CONV_HOOKS else key[1])
    assert set(shapes) == set(S.MUTATIONS) and all(len(v) >= 2 for v in shapes.values()), {k: len(v) for k, v in shapes.items()}
    # what is observable where, as MUTATION_NOTES states it
    small = set(S.SMALL)
    assert shapes["tap_mirrored"] == small - {(1, 1, 1)} and shapes["halo_cut_to_2"] == small - {(1, 1, 1), (1, 2, 2)}
    assert shapes["eighth_tap_leaks"] == small - {(1, 1, 1), (1, 2, 2), (1, 4, 4)} and shapes["drop_last_column"] == small
    assert shapes["align_corners_false"] == set(S.LEVELS) - {(2, 2)} and shapes["clip_mask_ignored"] == set(S.LEVELS) == shapes["flow_up_2x_missing"]
    assert shapes["uv_scales_swapped"] == {(13, 37), (31, 33), (40, 72)} and shapes["pair_swapped"] == set(S.LEVEL0 + S.LEVELS)


@pytest.mark.parametrize("shape", LARGE, ids=T.sid)
def test_the_emulation_is_inside_the_bound_at_the_large_shapes(shape):
    """(3,80,352) in both families; the deep shape and the weight gradient's several-tiles shape in the grid family, where the emulation has
    to EQUAL the reference -- at the deep shape an fp32 F.conv2d, itself exact there."""
    cases = [c for c in DISTINCT if c.shape == shape and c.dtype == "bf16"]
    assert cases
    for c in cases:
        S.check(c, S.emulate(c), label="emulation")


def test_a_nan_an_untouched_sentinel_or_a_touched_neighbour_fails_the_check():
    c = S.case("dgrad", (1, 3, 5), j=2, aux=1, family="rand")
    good = S.emulate(c)
    assert S.passes(c, good)
    for bad in (float("nan"), T.SENTINEL):
        g = {"dx": good["dx"].clone()}
        g["dx"][0, 5, 1, 2] = bad
        assert not S.passes(c, g)
    g = {"dx": good["dx"].clone()}
    g["dx"][tuple((S.inputs_of(c)["aux"] <= 0).nonzero()[0])] = 1e-30      # a ReLU-masked element has the bound 0
    assert not S.passes(c, g)
    c = S.case("prepare", (3, 6, 2), "fp32", pair_mode=1, P=3)
    g = S.emulate(c)
    assert S.passes(c, g)
    g["x16"][1, 0, 2, 1] += 2.0 ** -20                       # the reference frame is copied: bound 0 in the fp32 build
    assert not S.passes(c, g)
    g = S.emulate(c)
    g["x16"][1, 9, 2, 1] = 1e-30                             # the eight channels behind the input stay zero
    assert not S.passes(c, g)
    c = S.case("wgrad", (1, 9, 31), j=4, accumulate=1, family="grid")
    g = S.emulate(c)
    assert S.passes(c, g)
    g["gw"][0, 0, 3, 3] += 0.25                              # the grid family holds no slack at all
    assert not S.passes(c, g)


def test_the_coordinate_term_is_what_the_docstring_counts():
    """delta of src_index and warp_coord on the magnitudes at hand: 3 roundings of (d + 0.5) scale, 2 of d scale, 5 m + d / 2."""
    i0, i1, l1, delta = S._src_index(37, 64, 64, 37, False, torch.float64)
    d = torch.arange(37, dtype=torch.float64)
    assert torch.allclose(delta, 3 * 2.0 ** -24 * (d + 0.5) * (64 / 37), rtol=1e-14, atol=0) and int(i0[0]) == 0 and int(i1[-1]) == 63
    i0, i1, l1, delta = S._src_index(8, 4, 3, 7, True, torch.float64)
    assert torch.allclose(delta, 2 * 2.0 ** -24 * torch.arange(8, dtype=torch.float64) * (3 / 7), rtol=1e-14, atol=0) and float(l1[0]) == 0 and int(i0[-1]) in (2, 3)
    i0, i1, l1, delta = S._src_index(2, 1, 0, 1, True, torch.float64)      # from a 1 x 1 flow: the constant, no coordinate error
    assert not bool(delta.any()) and not bool(l1.any()) and not bool(i1.any())
    base, flow = torch.tensor([3.0], dtype=torch.float64), torch.tensor([-7.5], dtype=torch.float64)
    assert float(S._warp_delta(base, flow, 9)) == 2.0 ** -24 * (5 * 4.5 + 4) and float(S._warp_delta(base, flow, 1)) == 0.0
    assert float(S._warp_coord(base, flow, 1)) == 0.0 and abs(float(S._warp_coord(base, flow, 2)) + 4.5) < 1e-12      # dim - 1 = 0 and = 1


# --------------------------------------------------------------------------------------------------------------------
# the hooks' argument checks
# --------------------------------------------------------------------------------------------------------------------
def _lib():
    from vsrlab_amd import _lib
    return _lib.load()


def test_hooks_refuse_what_no_kernel_supports_before_any_launch():
    lib = _lib()
    X, W_, B, WP, Y, PRES, AUX, GW, GB, SL, FU, DP = A
    n, h, w = 2, 8, 12

    def conv(**k):
        a = dict(dtype=BF16, j=1, x=X, w=W_, bias=B, wpack=WP, y=Y, act=1, pres=None, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_spy_conv(a["dtype"], a["j"], a["x"], a["w"], a["bias"], a["wpack"], a["y"], a["act"], a["pres"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(j=-1), dict(j=5), dict(x=None), dict(w=None), dict(wpack=None), dict(y=None), dict(act=2), dict(act=-1), dict(n=0), dict(h=0), dict(w_=0)):
        assert conv(**k) == BADARG, k
    for k in (dict(pres=PRES), dict(j=0, pres=PRES), dict(j=3, pres=PRES, dtype=F32)):
        assert conv(**k) == UNSUPPORTED, k                 # pres: the planar last layer only

    def dgrad(**k):
        a = dict(dtype=BF16, j=1, dy=X, w=W_, wpack=WP, dx=Y, aux=AUX, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_spy_dgrad(a["dtype"], a["j"], a["dy"], a["w"], a["wpack"], a["dx"], a["aux"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=3), dict(j=5), dict(dy=None), dict(w=None), dict(wpack=None), dict(dx=None), dict(n=0), dict(h=-1), dict(w_=0)):
        assert dgrad(**k) == BADARG, k
    for k in (dict(j=0), dict(j=0, dtype=F32)):
        assert dgrad(**k) == UNSUPPORTED, k                # layer 0's input is no activation: nothing masks its gradient

    def wgrad(**k):
        a = dict(dtype=BF16, j=2, x=X, dy=Y, gw=GW, gb=GB, acc=1, slab=SL, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_spy_wgrad(a["dtype"], a["j"], a["x"], a["dy"], a["gw"], a["gb"], a["acc"], a["slab"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(j=-2), dict(x=None), dict(dy=None), dict(gw=None), dict(slab=None), dict(acc=2), dict(acc=-1), dict(n=0), dict(h=0), dict(w_=0)):
        assert wgrad(**k) == BADARG, k

    def prep(**k):
        a = dict(dtype=BF16, fr=X, fp=Y, fu=FU, x16=WP, n=1, t=2, P=2, pm=0, h=h, w_=w, lv0=0)
        a.update(k)
        return lib.vsr_debug_spy_prepare(a["dtype"], a["fr"], a["fp"], a["fu"], a["x16"], a["n"], a["t"], a["P"], a["pm"], a["h"], a["w_"], a["lv0"], None)

    for k in (dict(dtype=2), dict(fr=None), dict(fu=None), dict(x16=None), dict(fp=None), dict(lv0=1), dict(lv0=2), dict(pm=2), dict(P=3), dict(t=1, P=0), dict(n=0),
              dict(h=7), dict(w_=11), dict(h=0), dict(pm=1, P=0)):
        assert prep(**k) == BADARG, k

    def pbwd(**k):
        a = dict(dtype=BF16, dx=X, dl=Y, fr=W_, fu=FU, dp=DP, df=GW, n=1, t=2, P=2, pm=0, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_spy_prepare_bwd(a["dtype"], a["dx"], a["dl"], a["fr"], a["fu"], a["dp"], a["df"], a["n"], a["t"], a["P"], a["pm"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(dx=None), dict(fr=None), dict(dp=None, df=None), dict(dl=None), dict(fu=None), dict(dp=None), dict(dp=None, fu=None), dict(h=7),
              dict(w_=11), dict(P=3), dict(pm=3), dict(h=0)):
        assert pbwd(**k) == BADARG, k

    for k in (dict(dtype=2), dict(d=None), dict(out=None), dict(P=0), dict(h=0), dict(w_=0)):
        a = dict(dtype=BF16, d=X, res=Y, out=WP, P=3, h=h, w_=w)
        a.update(k)
        assert lib.vsr_debug_spy_dres(a["dtype"], a["d"], a["res"], a["out"], a["P"], a["h"], a["w_"], None) == BADARG, k

    def planar(**k):
        a = dict(op=0, a=X, b=Y, out=WP, mean=B, std=GB, planes=2, h=h, w_=w, hu=32, wu=32)
        a.update(k)
        return lib.vsr_debug_spy_planar(a["op"], a["a"], a["b"], a["out"], a["mean"], a["std"], a["planes"], a["h"], a["w_"], a["hu"], a["wu"], None)

    for k in (dict(op=-1), dict(op=7), dict(a=None), dict(out=None), dict(mean=None), dict(std=None), dict(op=1, std=None), dict(planes=0), dict(planes=2 ** 31), dict(h=0),
              dict(hu=0), dict(op=4, wu=0), dict(op=5, hu=-1), dict(op=2, h=7), dict(op=3, w_=11), dict(op=6, b=None)):
        assert planar(**k) == BADARG, k


def test_hostcheck_program_passes_without_sanitizers(tmp_path):
    """tools/spynet_hooks_hostcheck.hip (the hooks against stubbed launches; `make hooks_hostcheck` runs it under ASan / UBSan) built plain
    and run: every refusal before any pack or launch; per layer j and dtype what Ctx::spy_conv, spy_dgrad and spy_wgrad hand to
    vsr_launch_conv, vsr_launch_wgrad and vsr_launch_wgrad_reduce -- template sizes, cout_real, the mask mode, strides, x_coff / x_ctotal of
    the fp32 64-channel split --; and the arguments of the ten elementwise launchers in their own order."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    r = subprocess.run(["make", "-C", os.path.join(root, "vsrlab_amd", "csrc"), "spynet_hostcheck", "HOSTCHECK_SAN=", f"HOSTCHECK_OUT={tmp_path}/hostcheck"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "spynet hostcheck OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
