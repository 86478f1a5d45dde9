"""CPU side of the flow-warp harness (tests/flow_warp_common.py, csrc/warp_hooks.hip):

* the fp64 restatement that test_flow_warp_gpu.py measures the kernels against -- forward, the adjoint into the warped tensor, ``d flow``,
  zeros and border padding -- is pinned at 1e-10 to torch autograd on the oracle's ``flow_warp``, in both input families; ``d flow`` in the
  grid family, where positions sit on integers and on the first and last pixel centre, to autograd on ``F.grid_sample`` itself (the oracle's
  ``clamp`` keeps the gradient on the closed interval; ATen zeroes it there).  With a zero flow the border-mode flow gradient is exactly 0
  on the frame's border;
* the fp32 restatement of ``warp_coord`` stays inside the derived ``delta_p`` on every case;
* the criterion is dry-run: over every GPU case the fp32 emulation is inside the bound (grid family: EQUAL to the reference or its bf16
  rounding), and each of the ten deliberately wrong evaluations is rejected by at least one case; a NaN, a value left at the sentinel, a
  written band and a written gap each fail;
* the hooks refuse what no kernel supports before any launch: tools/warp_hooks_hostcheck.hip against the recording launch layer (built
  plain here; `make hooks_hostcheck` runs it under ASan / UBSan), and the library's own entries on fake pointers."""
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import hr_tail_common as T
import flow_warp_common as W
from oracle import basicvsr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -2
F32, BF16 = 0, 1
A = [0x10000000 + 0x1000000 * i for i in range(8)]        # 256-byte aligned, never dereferenced
PIN = [((2, 13, 37), "rand"), ((1, 9, 31), "rand"), ((2, 1, 45), "rand"), ((1, 9, 1), "rand"), ((1, 1, 1), "rand"), ((2, 9, 33), "grid"), ((1, 5, 129), "grid")]


def _close(a, b, tol=1e-10):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _grid_sample_warp(x, flow, mode):
    """The reference project's flow_warp, on F.grid_sample: mesh grid + flow, normalised by max(dim - 1, 1), align_corners=True."""
    n, _, h, w = x.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=x.dtype), torch.arange(w, dtype=x.dtype), indexing="ij")
    gx = 2.0 * (xs + flow[:, 0]) / max(w - 1, 1) - 1.0
    gy = 2.0 * (ys + flow[:, 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack([gx, gy], dim=3), mode="bilinear", padding_mode=mode, align_corners=True)


@pytest.mark.parametrize("shape,family", PIN, ids=lambda v: T.sid(v) if isinstance(v, tuple) else v)
@pytest.mark.parametrize("border", [0, 1], ids=["zeros", "border"])
def test_the_reference_is_pinned_to_autograd(shape, family, border):
    C, mode = 16, "border" if border else "zeros"
    k = lambda hook, **o: W.case(hook, shape, C=C, family=family, **o)
    t = {n: v.double() for n, v in W.inputs_of(k("fwd")).items()}
    x, flow = t["x"].clone().requires_grad_(True), t["flow"].clone().requires_grad_(True)
    y = O.flow_warp(x, flow, mode)
    (y * t["g"]).sum().backward()
    assert _close(W.reference(k("fwd", border=border))[0]["out"][0], y.detach())
    assert _close(W.reference(k("scatter", border=border, top=0))[0]["out"][0], x.grad)
    assert _close(W.reference(k("scatter", border=border, top=1))[0]["out"][0], x.grad + t["top"])
    if not border:
        assert _close(W.reference(k("gather", top=0))[0]["out"][0], x.grad)
        assert _close(W.reference(k("gather", top=1))[0]["out"][0], x.grad + t["top"])
    ref_dflow = W.reference(k("flowgrad", border=border))[0]["dflow"][0]
    if family == "rand":
        assert _close(ref_dflow, flow.grad)
    x2, flow2 = t["x"].clone(), t["flow"].clone().requires_grad_(True)
    y2 = _grid_sample_warp(x2, flow2, mode)
    assert _close(y2.detach(), y.detach())
    (y2 * t["g"]).sum().backward()
    assert _close(ref_dflow, flow2.grad)


def test_a_zero_flow_has_no_border_mode_flow_gradient_on_the_frames_border():
    """Border mode, zero flow: the position is exactly x, and ATen zeroes d flow_x on the first and last column, d flow_y on the first and
    last row.  The reference does; the closed gate (what warp_bwd_flow_kernel used to apply) returns -g * in[W - 1] on the last column."""
    shape = (2, 9, 33)
    n, h, w = shape
    c = W.case("flowgrad", shape, C=64, family="grid", border=1)
    t = W.inputs_of(c)
    (ya, xa), (yb, xb) = W.zero_blocks(shape)
    assert bool((t["flow"][-1, :, ya, xa] == 0).all()) and bool((t["flow"][-1, :, yb, xb] == 0).all()) and ya.start == 0 and xa.start == 0 and yb.stop == h and xb.stop == w
    r = W.reference(c)[0]["dflow"][0]
    x, flow = t["x"].double(), t["flow"].double().requires_grad_(True)
    (_grid_sample_warp(x, flow, "border") * t["g"].double()).sum().backward()
    assert _close(flow.grad, r)
    for d in (r, flow.grad):
        assert bool((d[-1, 0, ya, 0] == 0).all()) and bool((d[-1, 0, yb, w - 1] == 0).all())           # d flow_x on the first and the last column
        assert bool((d[-1, 1, 0, xa] == 0).all()) and bool((d[-1, 1, h - 1, xb] == 0).all())           # d flow_y on the first and the last row
        assert bool((d[-1, 0, ya, 1:xa.stop] != 0).any()) and bool((d[-1, 1, 1:ya.stop, xa] != 0).any())
    closed = W._ops(c, {k: (v.double() if k != "flow" else v) for k, v in t.items()}, torch.float64, "border_gate_closed")["dflow"]
    want = -(t["g"].double() * t["x"].double())[-1, :, yb, w - 1].sum(0)
    assert torch.equal(closed[-1, 0, yb, w - 1], want) and bool((want != 0).any())


# --------------------------------------------------------------------------------------------------------------------
# the criterion
# --------------------------------------------------------------------------------------------------------------------
ALL = W.gpu_cases()
DISTINCT = W.distinct(ALL)


def test_the_case_list_covers_every_hook_shape_width_and_dtype():
    for shape, fam, C in W.PLACES:
        for hook in W.HOOKS:
            got = {(c.dtype, c.o("nmul")) for c in ALL if c.hook == hook and c.shape == shape and c.o("C") == C and c.o("family") == fam}
            assert got == {(d, m) for d in ("bf16", "fp32") for m in (1, 3)}, (hook, shape, fam, C, got)
    assert {s for s, f, C in W.PLACES if f == "rand" and C == 64} == set(W.RAND_SHAPES) and set(T.SHAPES) < set(W.RAND_SHAPES)
    assert {s for s, f, C in W.PLACES if f == "grid" and C == 64} == set(W.GRID_SHAPES)
    assert all((s[1] - 1) & (s[1] - 2) == 0 and (s[2] - 1) & (s[2] - 2) == 0 for s in W.GRID_SHAPES)          # H - 1 and W - 1 powers of two
    for C in (16, 32):
        assert {f for s, f, c in W.PLACES if c == C} == {"rand", "grid"}
    for hook in ("fwd", "scatter", "flowgrad"):
        assert {c.o("border") for c in ALL if c.hook == hook} == {0, 1}
    assert {c.o("top") for c in ALL if c.hook == "gather"} == {0, 1} == {c.o("top") for c in ALL if c.hook == "scatter"}
    over = W.over_cap_cases()
    assert {c.hook for c in over} == set(W.HOOKS) and all(c.dtype == "bf16" for c in over)
    n, h, w = W.OVER_CHUNKS
    assert n * h * w * 8 > 4096 * 256
    n, h, w = W.OVER_PIXELS
    assert n * h * w > 4096 * 256
    assert sum(W.has_sink(s) for s in W.RAND_SHAPES) >= 3


def test_the_grid_flows_hold_the_values_the_discrete_behaviour_hangs_on():
    for shape in W.GRID_SHAPES:
        f = W.inputs_of(W.case("fwd", shape, C=64, family="grid"))["flow"]
        assert bool((f * 4 == (f * 4).round()).all()) and float(f.abs().max()) == 4.75
        for v in (0.0, 4.0, -4.0, 4.25, -4.25):
            assert bool((f == v).any()), (shape, v)
        n, h, w = shape
        px, py = W.positions(f, h, w, torch.float64)
        for p, dim in ((px, w), (py, h)):       # on the first and the last pixel centre, one step outside, across a tile edge
            assert bool((p == 0).any()) and bool((p == dim - 1).any()) and bool(((p >= -1) & (p < 0)).any()) and bool(((p > dim - 1) & (p <= dim)).any())
        assert bool(((px.floor() % 32 == 31) & (px > px.floor())).any()) and (h <= 8 or bool(((py.floor() % 8 == 7) & (py > py.floor())).any()))


@pytest.mark.parametrize("c", [c for c in DISTINCT if c.dtype == "bf16"] , ids=lambda c: c.name)
def test_the_fp32_coordinate_stays_inside_delta_p(c):
    n, h, w = c.shape
    flow = W.inputs_of(c)["flow"]
    p32, p64, dp = W.positions(flow, h, w, torch.float32), W.positions(flow, h, w, torch.float64), W.delta_p(flow, h, w, 0)
    for a, b, d, dim in zip(p32, p64, dp, (w, h)):
        err = (a.double() - b).abs()
        assert bool((err <= d).all()), (c.name, float((err / d.clamp_min(1e-300)).max()))
        if c.o("family") == "grid":
            assert float(err.max()) == 0
        elif dim > 1:
            assert bool((a.floor().double() == b.floor()).all())
    if c.o("family") == "rand":
        assert float(max(d.max() for d in dp)) < 1 / 64


@pytest.mark.parametrize("place", W.PLACES, ids=lambda p: f"{T.sid(p[0])}-{p[1]}-c{p[2]}")
def test_same_precision_emulation_is_inside_the_bound(place):
    """Every distinct GPU case's emulation (fp32 on the fp32 coordinate, rounded to bf16 where the build stores) passes check(): in the
    grid family that is equality with the fp64 reference or its bf16 rounding."""
    shape, fam, C = place
    cases = [c for c in DISTINCT if c.shape == shape and c.o("family") == fam and c.o("C") == C]
    assert {c.hook for c in cases} == set(W.HOOKS)
    for c in cases:
        W.check(c, W.emulate(c), label="emulation")


def test_every_mutation_is_rejected_by_some_case():
    """The ten mutations over every distinct case but those of the largest shape: each is rejected by at least one case, by the hooks it
    can touch, and where it has to show (the grid family for the far threshold and the border gate)."""
    rejected = {}
    for c in DISTINCT:
        if c.shape in (T.SHAPES[-1], W.OVER_CHUNKS, W.OVER_PIXELS):
            continue
        for mut in W.MUTATIONS:
            if not W.passes(c, W.emulate(c, mut)):
                rejected.setdefault(mut, []).append(c.name)
    for mut in W.MUTATIONS:
        print(f"FLOW_WARP_MUTATION {mut}: rejected by {len(rejected.get(mut, []))} cases")
    assert set(rejected) == set(W.MUTATIONS), sorted(set(W.MUTATIONS) - set(rejected))
    hooks = lambda mut: {n.split("[")[0] for n in rejected[mut]}
    assert hooks("nstride_ignored") == set(W.HOOKS) and hooks("weights_swapped") == set(W.HOOKS) and hooks("tap_test_inclusive") == set(W.HOOKS)
    assert hooks("dim1_uses_flow") == set(W.HOOKS) and hooks("border_gate_closed") == {"flowgrad"} and hooks("dtop_dropped") == {"scatter", "gather"}
    for mut in ("halo_radius_4", "hit_cap_truncates", "far_share_dropped", "far_threshold_open"):
        assert hooks(mut) == {"gather"}, mut
    assert all("family=grid" in n for n in rejected["far_threshold_open"]) and all("border=1" in n for n in rejected["border_gate_closed"])
    assert any("family=grid" in n for n in rejected["border_gate_closed"])


@pytest.mark.parametrize("c", W.over_cap_cases(), ids=lambda c: c.name)
def test_the_over_the_cap_cases_pass_in_emulation(c):
    W.check(c, W.emulate(c), label="emulation")


def test_a_nan_a_sentinel_a_written_band_and_a_written_gap_fail():
    c = W.case("gather", (2, 13, 37), C=16, family="rand", top=1, nmul=3)
    good = W.emulate(c)
    assert W.passes(c, good)
    for bad in (float("nan"), T.SENTINEL):
        g = dict(good, out=good["out"].clone())
        g["out"][1, 5, 7, 20] = bad
        assert not W.passes(c, g)
    assert not W.passes(c, dict(good, _far=good["_far"] + 1))
    cg = W.case("fwd", (2, 9, 33), "fp32", C=16, family="grid", border=1)
    g = W.emulate(cg)
    assert W.passes(cg, g)
    g["out"][0, 3, 4, 5] += 2.0 ** -20                       # the grid family's bound is 0
    assert not W.passes(cg, g)
    cpu = torch.device("cpu")
    band = T.Guarded(64, torch.float32, cpu, T.SENTINEL)
    assert band.bands_untouched()
    band.buf[band.lo + 64] = 0.0
    assert not band.bands_untouched()
    n, h, w = 2, 3, 5
    gap = T.Planar(n, 2, h, w, 3 * 2 * h * w, cpu, T.SENTINEL)
    gap.view.copy_(torch.zeros(n, 2, h, w))
    gap.take()
    gap.view.copy_(torch.zeros(n, 2, h, w))
    gap.g.body[2 * h * w] = 0.0                              # the first float behind image 0: what a kernel on the stride 2HW writes
    with pytest.raises(AssertionError):
        gap.take()


# --------------------------------------------------------------------------------------------------------------------
# the hooks' argument checks
# --------------------------------------------------------------------------------------------------------------------
def test_hostcheck_program_passes_without_sanitizers(tmp_path):
    """tools/warp_hooks_hostcheck.hip (the hooks against recording stubs; `make hooks_hostcheck` runs it under ASan / UBSan) built plain and
    run: every refusal before any launch; every accepted call hands its pointers, the width, flow_nstride and the padding mode to the
    launcher, the scatter hook to vsr_launch_warp_bwd and then vsr_launch_add_cast on the same accumulator."""
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "vsrlab_amd", "csrc"), "warp_hostcheck", "HOSTCHECK_SAN=", f"HOSTCHECK_OUT={tmp_path}/hostcheck"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "warp hostcheck OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_hooks_refuse_null_pointers_bad_sizes_and_other_widths_before_any_launch():
    from vsrlab_amd import _lib
    lib = _lib.load()
    X, FL, OUT, ACC, TOP, S_, FC, DF = A
    n, h, w = 2, 8, 12
    ns = 2 * h * w

    def fwd(**k):
        a = dict(dt=BF16, C=64, x=X, fl=FL, ns=ns, out=OUT, border=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_warp_fwd(a["dt"], a["C"], a["x"], a["fl"], a["ns"], a["out"], a["border"], a["n"], a["h"], a["w_"], None)

    def scatter(**k):
        a = dict(dt=BF16, C=64, g=X, fl=FL, ns=ns, acc=ACC, top=TOP, out=OUT, border=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_warp_scatter(a["dt"], a["C"], a["g"], a["fl"], a["ns"], a["acc"], a["top"], a["out"], a["border"], a["n"], a["h"], a["w_"], None)

    def gather(**k):
        a = dict(dt=BF16, C=64, g=X, fl=FL, ns=ns, top=TOP, S=S_, fc=FC, out=OUT, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_warp_gather(a["dt"], a["C"], a["g"], a["fl"], a["ns"], a["top"], a["S"], a["fc"], a["out"], a["n"], a["h"], a["w_"], None)

    def flowgrad(**k):
        a = dict(dt=BF16, C=64, x=X, g=TOP, fl=FL, ns=ns, df=DF, border=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_warp_flowgrad(a["dt"], a["C"], a["x"], a["g"], a["fl"], a["ns"], a["df"], a["border"], a["n"], a["h"], a["w_"], None)

    common = (dict(dt=2), dict(dt=-1), dict(fl=None), dict(ns=ns - 1), dict(ns=0), dict(n=0), dict(h=0), dict(w_=-1))
    for fn, extra in ((fwd, (dict(x=None), dict(out=None), dict(border=2), dict(border=-1))),
                      (scatter, (dict(g=None), dict(acc=None), dict(out=None), dict(border=2))),
                      (gather, (dict(g=None), dict(S=None), dict(fc=None), dict(out=None))),
                      (flowgrad, (dict(x=None), dict(g=None), dict(df=None), dict(border=3)))):
        for k in common + extra:
            assert fn(**k) == BADARG, (fn.__name__, k)
        for C in (0, 8, 24, 48, 128):
            assert fn(C=C) == UNSUPPORTED, (fn.__name__, C)
        assert fn(C=48, fl=None) == BADARG                   # a bad argument is reported before an unsupported width
    assert lib.vsr_debug_warp_add_cast(BF16, 64, None, None, OUT, n, h, w, None) == BADARG
    assert lib.vsr_debug_warp_add_cast(BF16, 64, X, None, None, n, h, w, None) == BADARG
    assert lib.vsr_debug_warp_add_cast(3, 64, X, None, OUT, n, h, w, None) == BADARG
    assert lib.vsr_debug_warp_add_cast(BF16, 64, X, None, OUT, n, 0, w, None) == BADARG
    assert lib.vsr_debug_warp_add_cast(BF16, 40, X, None, OUT, n, h, w, None) == UNSUPPORTED
    # the two older gather entries are the new hook at flow_nstride = 2HW: the same refusals
    for fn, tail in ((lib.vsr_debug_warp_bwd_gather, ()), (lib.vsr_debug_warp_bwd_gather_c, (64,))):
        fn.restype = _lib.c_int
        fn.argtypes = [_lib.c_int] + [_lib.c_void_p] * 6 + [_lib.c_int] * (3 + len(tail)) + [_lib.c_void_p]
        assert fn(BF16, None, FL, None, S_, FC, OUT, n, h, w, *tail, None) == BADARG
        assert fn(BF16, X, FL, None, S_, FC, OUT, n, h, 0, *tail, None) == BADARG
        assert fn(2, X, FL, None, S_, FC, OUT, n, h, w, *tail, None) == BADARG
    assert lib.vsr_debug_warp_bwd_gather_c(BF16, X, FL, None, S_, FC, OUT, n, h, w, 48, None) == UNSUPPORTED
