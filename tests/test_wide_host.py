"""CPU tests of the GAN side's launch-by-launch pin (no GPU): the fp64 restatements of tests/wide_common.py against torch's own
definitions and autograd at 1e-10, the criterion on an fp32 emulation with another summation order, the rejection of every wrong
variant in wide_common.MUTATIONS at every small shape where it is observable, the hooks' refusals (before any pack or launch, so no
device is touched), the host-only grid and plan entries, and tools/wide_hooks_hostcheck.hip (built plain here; `make hooks_hostcheck`
runs it under ASan / UBSan)."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import wide_common as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _r(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize("mode", (0, 1, 2, 3))
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 5), (2, 5, 7), (1, 9, 4)], ids=W.sid)
def test_the_assembled_conv_is_the_definition(shape, mode):
    """The sum over 64-channel slices (and, stride 2, over the four parity views of 2x2-tap convolutions / into the four output phases)
    equals conv2d / conv2d(stride=2) / conv_transpose2d / conv_transpose2d(stride=2), and the latter two are autograd's data gradients."""
    n, h, w = shape
    cout, cin, ks = 128, 192, 4 if mode in (1, 3) else 3
    wt = _r(1, cout, cin, ks, ks)
    s = 2 if mode == 1 else 1
    x = _r(2, n, cout if mode >= 2 else cin, h * s, w * s)
    want = W.conv_def(x, wt, mode)
    _close(W.conv_views(x, wt, mode), want)
    _close(W.conv_views(x, wt, mode, rev=True), want)
    if mode >= 2:
        so = 2 if mode == 3 else 1
        xin = torch.zeros(n, cin, h * so, w * so, dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(xin, wt, stride=so, padding=1), xin, x)
        _close(want, g)


@pytest.mark.parametrize("views", (1, 4))
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 5), (2, 5, 7)], ids=W.sid)
def test_the_assembled_weight_gradient_is_autograds(shape, views):
    n, h, w = shape
    s = 2 if views == 4 else 1
    x, dy = _r(3, n, 64, h * s, w * s), _r(4, n, 128, h, w)
    _close(W.wgrad_views(x, dy, views), W.wgrad_def(x, dy, views))
    _close(W.wgrad_views(x, dy, views, rev=True), W.wgrad_def(x, dy, views))


def test_the_epilogue_order():
    """v = acc + bias -> LeakyReLU -> y_act -> + res -> * (aux > 0 ? 1 : slope), spelled out element by element."""
    c = W.case("conv", (1, 2, 3), "fp32", mode=0, cin=64, cout=64, act=W.ACT_LEAKY, bias=1, y_act=1, res=1, aux=1)
    acc, bias, res = _r(5, 1, 64, 2, 3), _r(6, 64), _r(7, 1, 64, 2, 3)
    aux = W.draw_aux(8, 1, 2, 3).double()
    out = W.epilogue(c, acc, dict(bias=bias, res=res, aux=aux))
    for i in range(acc.numel()):
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), acc.shape))
        v = float(acc[idx]) + float(bias[idx[1]])
        v = v if v > 0 else W.SLOPE * v
        assert float(out["y_act"][idx]) == v
        v = v + float(res[idx])
        v = v if float(aux[idx]) > 0 else W.SLOPE * v
        assert float(out["y"][idx]) == v
    # slope 0: what the mask zeroes is +0, also for a negative value
    c0 = W.case("conv", (1, 2, 3), "fp32", mode=2, cin=64, cout=64, aux=1, slope=0.0)
    y = W.epilogue(c0, -acc.abs() - 1, dict(aux=aux))["y"]
    z = ~(aux > 0)
    assert bool((y[z] == 0).all()) and not bool(torch.signbit(y[z]).any()) and bool((y[~z] < 0).all())


@pytest.mark.parametrize("hw", W.UP2_SOURCES[:6], ids=W.sid)
def test_up2_and_its_adjoint(hw):
    """The separable (1/4, 3/4) form with clamped neighbours is F.interpolate(scale_factor=2, bilinear, align_corners=False), the U-Net step
    is up2(a + b), and the gather with the folded border weight is autograd's adjoint (an inner product test besides)."""
    h, w = hw
    a, b, d = _r(9, 2, 8, h, w), _r(10, 2, 8, h, w), _r(11, 2, 8, 2 * h, 2 * w)
    _close(W.up2_sep(a + b), W.up2_def(a + b))
    c = W.case("up2_fwd", (2, h, w), "fp32", C=8, b=1)
    _close(W._ops(c, dict(a=a, b=b), assembled=True)["out"], F.interpolate(a + b, scale_factor=2, mode="bilinear", align_corners=False))
    _close(W.up2_sep_adjoint(d), W.up2_adjoint_def(d))
    assert abs(float((W.up2_sep(a) * d).sum() - (a * W.up2_sep_adjoint(d)).sum())) < 1e-9
    const = torch.full((1, 8, h, w), 0.3, dtype=torch.float64)
    _close(W.up2_def(const), torch.full((1, 8, 2 * h, 2 * w), 0.3, dtype=torch.float64))


@pytest.mark.parametrize("hw", W.POOL_INPUTS[:5], ids=W.sid)
def test_pool_adjoint_routes_to_the_first_maximum(hw):
    """On inputs with ties in most windows (the grid family), autograd through F.max_pool2d(., 2, 2) routes to the FIRST maximum in
    row-major order, and rows / columns the floor drops get nothing."""
    h, w = hw
    a = W.pool_input(12, 2, 8, h, w).double()
    dp = _r(13, 2, 8, h // 2, w // 2)
    win = torch.stack([a[:, :, q >> 1:2 * (h // 2):2, (q & 1):2 * (w // 2):2] for q in range(4)], -1)
    ties = (win == win.max(-1, keepdim=True).values).sum(-1) > 1
    assert float(ties.float().mean()) > 0.5
    want = W.pool_route_def(a, dp)
    assert torch.equal(W.pool_route_first(a, dp), want)
    assert not torch.equal(W.pool_route_first(a, dp, "pool_last_max"), want)
    assert bool((want[:, :, 2 * (h // 2):] == 0).all()) and bool((want[:, :, :, 2 * (w // 2):] == 0).all())


def test_pm_layout_round_trip_keeps_every_bit():
    t = W._specials(W.draw(14, 2, 16, 3, 37))
    for tdt in (torch.bfloat16, torch.float32):
        pm = W.to_pm(t, tdt)
        assert pm.shape == (2, 3, 2, 2, 32, 8) and bool(torch.isnan(pm[:, :, 1, :, 5:, :].float()).all())
        back = W.from_pm(pm, 37)
        assert torch.equal(back.view(torch.int32), t.view(torch.int32))
    # element (n, c, y, x) sits at ((y * WS + x / 32) * C/8 + c / 8) * 256 + (x % 32) * 8 + c % 8 of image n (csrc/common.h: pm_off)
    flat = W.to_pm(t, torch.float32).flatten()
    for (n, c, y, x) in [(0, 0, 0, 0), (1, 13, 2, 36), (0, 9, 1, 31), (1, 7, 0, 32)]:
        off = n * 3 * 2 * 16 * 32 + ((y * 2 + x // 32) * 2 + c // 8) * 256 + (x % 32) * 8 + c % 8
        assert float(flat[off]) == float(t[n, c, y, x])


def test_the_emulation_passes_the_criterion():
    for c in W.small_cases():
        W.check(c, W.emulate(c), label="emu")


@pytest.mark.parametrize("mut", W.MUTATIONS)
def test_every_wrong_variant_is_rejected(mut):
    """Through the check the GPU tests use, at every small case where the variant is observable; each variant is observable somewhere."""
    hit = 0
    for c in W.small_cases():
        if not W.applicable(c, mut):
            continue
        hit += 1
        assert not W.passes(c, W.emulate(c, mut)), (c.name, mut, "passes the criterion")
    assert hit >= 2, (mut, hit)


def test_the_gpu_tests_geometries_are_the_issues():
    ids = [g[0] for g in W.conv_geometries()]
    assert len(ids) == len(set(ids)) == 2 + 1 + 6 + 1 + 3 + 3 + 6 + 3
    # the launches with 64 output rows: conv_wide2's K-split form
    ks = [g for g, o in W.conv_geometries() if W.launch_ncob(W.case("conv", (1, 1, 1), **o))[0] == 1]
    assert ks == ["m0_leaky_128_64_yact_res", "m2_relumask_128_64", "m3_res_mask_128_64"]


# --------------------------------------------------------------------------------------------------------------------
# the library's host-side entries (no launch happens: every call below returns before one, or is host only)
# --------------------------------------------------------------------------------------------------------------------
def _lib():
    from vsrlab_amd import _lib as L
    return L, L.load()


def test_hooks_refuse_before_any_launch():
    """NULL pointers, sizes, modes, channel counts that are no multiple of 64, views other than 1 or 4, scratch that is too small: refused
    with the status, before the hook dereferences or launches anything (this machine has no device to launch on)."""
    L, lib = _lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    BAD, UNS, WSP = -1, -2, -4
    big = 1 << 40
    conv = lambda **k: lib.vsr_debug_wide_conv(*[k.get(a, d) for a, d in (("dtype", 1), ("mode", 0), ("cout", 128), ("cin", 64), ("x", p), ("w", p), ("bias", None),
                                                                              ("wpack", p), ("ne", big), ("y", p), ("act", 0), ("slope", 0.2), ("y_act", None),
                                                                              ("res", None), ("aux", None), ("max_wg", 0), ("N", 1), ("H", 8), ("W", 8), ("st", None))])
    assert conv(dtype=2) == BAD and conv(mode=4) == BAD and conv(mode=-1) == BAD and conv(cout=96) == BAD and conv(cin=0) == BAD and conv(cin=72) == BAD
    assert conv(x=None) == BAD and conv(w=None) == BAD and conv(wpack=None) == BAD and conv(y=None) == BAD and conv(act=3) == BAD
    assert conv(N=0) == BAD and conv(H=0) == BAD and conv(W=-1) == BAD and conv(max_wg=-1) == BAD
    assert conv(ne=128 * 64 * 9 - 1) == WSP and conv(dtype=0, ne=128 * 64 * 9 - 1) == WSP and conv(mode=1, ne=4 * 4 * 8192 - 1) == WSP
    assert conv(dtype=0, max_wg=3) == UNS and conv(dtype=0, N=40000, cout=128) == UNS
    wg = lambda **k: lib.vsr_debug_wide_wgrad(*[k.get(a, d) for a, d in (("dtype", 1), ("views", 1), ("xC", 128), ("dyC", 64), ("x", p), ("dy", p), ("gw", p), ("slab", p),
                                                                            ("nf", big), ("N", 1), ("H", 8), ("W", 8), ("st", None))])
    assert wg(dtype=3) == BAD and wg(views=2) == BAD and wg(views=0) == BAD and wg(xC=100) == BAD and wg(dyC=32) == BAD
    assert wg(x=None) == BAD and wg(dy=None) == BAD and wg(gw=None) == BAD and wg(slab=None) == BAD and wg(H=0) == BAD
    assert wg(nf=2 * lib.vsr_conv3x3_c64_wgrad_slab_floats() - 1) == WSP
    assert wg(views=4, xC=512, dyC=512) == UNS                   # 256 pairs x 8 pixel parts: more partials than a slab buffer holds
    assert lib.vsr_debug_wide_up2_fwd(1, None, None, p, 1, 2, 2, 128, None) == BAD and lib.vsr_debug_wide_up2_fwd(1, p, None, None, 1, 2, 2, 128, None) == BAD
    assert lib.vsr_debug_wide_up2_fwd(1, p, None, p, 1, 2, 2, 12, None) == BAD and lib.vsr_debug_wide_up2_fwd(1, p, None, p, 70000, 2, 2, 128, None) == UNS
    assert lib.vsr_debug_wide_up2_bwd(1, p, p, None, p, 0.2, 1, 2, 2, 128, None) == BAD          # din alone: no engine form
    assert lib.vsr_debug_wide_up2_bwd(1, p, None, p, None, 0.2, 1, 2, 2, 128, None) == BAD and lib.vsr_debug_wide_up2_bwd(1, None, p, p, p, 0.2, 1, 2, 2, 128, None) == BAD
    assert lib.vsr_debug_wide_mask(1, p, p, p, 0.2, 12, None) == BAD and lib.vsr_debug_wide_mask(1, p, None, p, 0.2, 16, None) == BAD
    assert lib.vsr_debug_vgg_pool(1, 0, p, p, p, 1, 2, 2, 64, None) == BAD and lib.vsr_debug_vgg_pool(1, 1, p, None, p, 1, 2, 2, 64, None) == BAD
    assert lib.vsr_debug_vgg_pool(1, 0, p, None, p, 1, 1, 2, 64, None) == BAD and lib.vsr_debug_vgg_pool(1, 2, p, None, p, 1, 2, 2, 64, None) == BAD
    assert lib.vsr_debug_vgg_tap(1, p, p, 2, 0.5, p, p, 1, 2, 2, 64, None) == BAD and lib.vsr_debug_vgg_tap(1, p, p, 1, 0.5, None, p, 1, 2, 2, 64, None) == BAD
    assert lib.vsr_debug_vgg_tap(1, p, None, 1, 0.5, p, p, 1, 2, 2, 64, None) == BAD and lib.vsr_debug_vgg_tap(1, p, p, 1, 0.5, p, p, 1, 2, 2, 60, None) == BAD
    assert lib.vsr_debug_wide2_set_max_wg(-1) == BAD
    out = (ctypes.c_int * 3)()
    assert lib.vsr_debug_wide_grid(0, 1, 1, 8, 8, 0, 256, out) == BAD and lib.vsr_debug_wide_grid(2, 3, 1, 8, 8, 0, 256, out) == BAD
    assert lib.vsr_debug_wide_grid(2, 1, 1, 8, 8, 0, 256, None) == BAD


def test_the_grid_of_a_conv_wide2_launch():
    """vsr_debug_wide_grid is the launcher's own grid choice (host only): columns = phases x 128-channel blocks (64-channel blocks of the
    K-split form), workgroups per column = CUs / columns, at most the tiles, at most the cap -- the launch's own, else the process-wide
    one of vsr_debug_wide2_set_max_wg."""
    L, lib = _lib()
    g = lambda ncob, step, shape, cap=0: W.grid_of(lib, ncob, step, shape, cap, 256)
    assert g(2, 1, (3, 80, 352)) == (256, 1, 330) and g(8, 1, (3, 80, 352)) == (64, 4, 330)
    assert g(1, 1, (1, 72, 136)) == (45, 1, 45) and g(1, 2, (1, 72, 136)) == (45, 4, 45) and g(4, 2, (1, 8, 32)) == (1, 8, 1)
    assert g(2, 1, (1, 40, 200), 3) == (3, 1, 35) and g(2, 1, (3, 24, 70), 4) == (4, 1, 27) and g(2, 1, (1, 8, 32), 3) == (1, 1, 1)
    try:
        assert lib.vsr_debug_wide2_set_max_wg(3) == 0
        assert g(4, 1, (1, 18, 34)) == (3, 2, 6)                 # conv_4 of a (72, 136) frame: 512 -> 256 at (18, 34)
        assert g(4, 1, (1, 18, 34), 2) == (2, 2, 6)              # a launch's own cap wins
    finally:
        assert lib.vsr_debug_wide2_set_max_wg(0) == 0
    assert g(4, 1, (1, 18, 34)) == (6, 2, 6)


def test_the_discriminator_plan_hook():
    """vsr_debug_disc_plan copies DPlan::build's offsets out: 256-byte aligned, increasing in the plan's order, the activations sized for
    the batch and the backward scratch for one frame, the total vsr_disc_workspace_bytes'."""
    L, lib = _lib()
    for (n, h, w, dt) in [(1, 16, 40, 1), (2, 16, 40, 0), (1, 8, 8, 1)]:
        d = L.DiscDesc(n, h, w, 64, dt)
        off = (ctypes.c_longlong * 30)()
        assert lib.vsr_debug_disc_plan(ctypes.byref(d), 1, off, 30) == 0
        o = list(off)
        assert all(v % 256 == 0 for v in o) and o[:29] == sorted(o[:29]) and len(set(o[:29])) == 29
        assert o[29] == lib.vsr_disc_workspace_bytes(ctypes.byref(d), 1)
        es = 2 if dt == 1 else 4
        pm = lambda hh, ww, c: hh * ((ww + 31) // 32) * 32 * c * es
        up = lambda v: (v + 255) & ~255
        assert o[1] - o[0] == up(n * pm(h, w, 64)) and o[4] - o[3] == up(n * pm(h // 8, w // 8, 512)) and o[14] - o[13] == up(pm(h, w, 64))
        assert lib.vsr_debug_disc_plan(ctypes.byref(d), 0, off, 30) == 0 and list(off)[13:29] == [-1] * 16
        assert list(off)[29] == lib.vsr_disc_workspace_bytes(ctypes.byref(d), 0) and list(off)[:13] == o[:13]
        assert lib.vsr_debug_disc_plan(ctypes.byref(d), 1, off, 29) == -1 and lib.vsr_debug_disc_plan(None, 1, off, 30) == -1
    bad = L.DiscDesc(1, 12, 40, 64, 1)
    assert lib.vsr_debug_disc_plan(ctypes.byref(bad), 1, off, 30) == -2


def test_hostcheck_program_passes_without_sanitizers(tmp_path):
    """tools/wide_hooks_hostcheck.hip (the hooks against recording stubs; `make hooks_hostcheck` runs it under ASan / UBSan) built plain and
    run: every refusal before any pack or launch; what the accepted calls hand to vsr_launch_conv_wide (steps, slices, output blocks,
    Hy / Wy, max_wg) and to the pack; vsr_launch_wgrad_pairs' ksplit for every layer geometry at 1, 8 and 200 tiles; the pair-by-pair
    fp32 path's views, slices and blocks."""
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "vsrlab_amd", "csrc"), "wide_hostcheck", "HOSTCHECK_SAN=", f"HOSTCHECK_OUT={tmp_path}/hostcheck"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "wide hostcheck OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
