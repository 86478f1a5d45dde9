"""CPU side of the reconstruction-tail harness (tests/hr_tail_common.py, csrc/hr_tail_hooks.hip):

* the fp64 restatements that test_hr_tail_gpu.py measures the kernels against are pinned at 1e-10 to torch autograd on the oracle's
  ``pixel_shuffle_pack`` and on conv_last as ``basicvsr_forward`` writes it, and to tests/golden/pixel_shuffle_pack.npz;
* the criterion is dry-run: over every GPU case an fp32 evaluation in another summation order (rounded to bf16 where the bf16 build
  stores) is inside the bound, and five deliberately wrong evaluations are outside it at every ragged case;
* the hooks refuse null pointers and bad sizes before any launch (the pointers here are fake and never dereferenced)."""
import pytest
import torch
import torch.nn.functional as F

import hr_tail_common as T
from helpers import golden, rand
from oracle import basicvsr_oracle as O

BADARG, UNSUPPORTED = -1, -2
F32, BF16 = 0, 1
A = [0x10000000 + 0x1000000 * i for i in range(12)]        # 16-byte aligned, never dereferenced


def _close(a, b, tol=1e-10):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _d(*ts):
    return [t.double() for t in ts]


# --------------------------------------------------------------------------------------------------------------------
# the references
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 4, 34)], ids=T.sid)
def test_pixel_shuffle_gradients_are_pinned_to_autograd_on_the_oracle(shape):
    n, h, w = shape
    p, dy, wt = _d(T.draw_aux(1, n, h, w), T.draw(2, n, 64, 2 * h, 2 * w), T.draw(3, 256, 64, 3, 3))
    b = torch.randn(256, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    leaves = {"upconv.weight": wt.clone().requires_grad_(True), "upconv.bias": b.clone().requires_grad_(True)}
    pl = p.clone().requires_grad_(True)
    x = F.leaky_relu(pl, T.SLOPE)                          # the layer's input is LeakyReLU(point_conv): its mask comes from p
    y = O.pixel_shuffle_pack(leaves, "", x)
    (y * dy).sum().backward()
    c = T.case("ps_dgrad", shape, mask="aux")
    assert _close(T._ops(c, dict(dy=dy, w=wt, aux=p))["dx"], pl.grad)
    plain = T._ops(T.case("ps_dgrad", shape), dict(dy=dy, w=wt, aux=p))
    assert _close(plain["dx"] * T.mask_factor(p, T.SLOPE), pl.grad)
    assert _close(plain["_s1"], F.conv_transpose2d(dy[:, :, 0::2, 0::2], wt[0::4], padding=1))      # the partial sums the bound uses
    assert _close(plain["_s3"] - plain["_s2"], F.conv_transpose2d(dy[:, :, 1::2, 0::2], wt[2::4], padding=1))
    assert _close(plain["dx"] - plain["_s3"], F.conv_transpose2d(dy[:, :, 1::2, 1::2], wt[3::4], padding=1))
    g = T._ops(T.case("ps_wgrads", shape), dict(x=x.detach(), dy=dy))
    assert _close(g["gw"], leaves["upconv.weight"].grad) and _close(g["gb"], leaves["upconv.bias"].grad)
    # the forward, phase by phase, and the phase-plane layout
    planes = torch.stack([T._conv(x.detach(), wt[z::4]) + b[z::4].view(1, -1, 1, 1) for z in range(4)])
    assert _close(T.shuffle_planes(planes), y.detach())
    assert torch.equal(T.unshuffle_planes(y.detach()), torch.stack([F.pixel_unshuffle(y.detach(), 2)[:, z::4] for z in range(4)]))
    assert torch.equal(T.shuffle_planes(T.unshuffle_planes(dy)), dy)
    assert torch.equal(T.unshuffle_planes(dy)[1], dy[:, :, 0::2, 1::2]) and torch.equal(T.unshuffle_planes(dy)[2], dy[:, :, 1::2, 0::2])


def test_pixel_shuffle_restatement_against_the_reference_golden():
    g = golden("pixel_shuffle_pack")
    sd = O.keyed_state_dict({"upconv.weight": (64, 16, 3, 3), "upconv.bias": (64,)})
    x = rand(g["seed_x"], 2, 16, 7, 9, lo=-1, hi=1).double()
    wt, b = sd["upconv.weight"].double(), sd["upconv.bias"].double()
    planes = torch.stack([F.conv2d(x, wt[z::4], b[z::4], padding=1) for z in range(4)])
    y = T.shuffle_planes(planes)
    assert float((y - g["y"].double()).abs().max() / g["y"].abs().max()) < 1e-5      # (the golden is the reference's fp32 output)
    assert _close(y, O.pixel_shuffle_pack({k: v.double() for k, v in sd.items()}, "", x))


@pytest.mark.parametrize("shape,scale", [((2, 8, 12), 4), ((1, 6, 10), 2), ((1, 1, 1), 0), ((1, 5, 33), 0)], ids=str)
def test_conv_last_is_pinned_to_autograd(shape, scale):
    """sr = conv_last.2(LeakyReLU(p)) + bilinear(lr) as basicvsr_forward has it: forward, data gradient (mask from p), weight and bias
    gradient -- and the planar -> 64 restatement as the data gradient of a 64 -> pc convolution."""
    n, h, w = shape
    p, dsr, wt = _d(T.draw_aux(5, n, h, w), T.draw(6, n, 3, h, w), T.draw(7, 3, 64, 3, 3))
    b = torch.randn(3, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    lr = torch.rand(n, 3, h // scale, w // scale, dtype=torch.float64, generator=torch.Generator().manual_seed(9)) if scale else None
    pl, wl, bl = p.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    c0 = F.leaky_relu(pl, T.SLOPE)
    sr = F.conv2d(c0, wl, bl, padding=1)
    if scale:
        sr = sr + F.interpolate(lr, scale_factor=scale, mode="bilinear", align_corners=False)
    (sr * dsr).sum().backward()
    t = dict(x=c0.detach(), w=wt, bias=b, base=lr)
    assert _close(T._ops(T.case("last2_fwd", shape, co=3, scale=scale), t)["y"], sr.detach())
    assert _close(T._ops(T.case("last2_dgrad", shape, mask="aux"), dict(dsr=dsr, w=wt, aux=p))["dx"], pl.grad)
    assert _close(T._ops(T.case("last2_dgrad", shape, mask="none"), dict(dsr=dsr, w=wt, aux=p))["dx"], F.conv_transpose2d(dsr, wt, padding=1))
    g = T._ops(T.case("last2_wgrad", shape), dict(x=c0.detach(), dy=dsr))
    assert _close(g["gw"], wl.grad) and _close(g["gb"], bl.grad)
    for pc in (1, 2):
        wl2 = wt[:pc].clone().requires_grad_(True)
        (F.conv2d(c0.detach(), wl2, padding=1) * dsr[:, :pc]).sum().backward()
        assert _close(T._ops(T.case("last2_wgrad", shape, pc=pc), dict(x=c0.detach(), dy=dsr))["gw"], wl2.grad)
    # planar -> 64 with the data-gradient weights, no activation, mask from p: the same gradient
    y = T._ops(T.case("planar_c64", shape, pc=3, act=0, bias=False, mask="aux"), dict(src=dsr, w=T._dgrad_w(wt), aux=p))["y"]
    assert _close(y, pl.grad)
    # ... and as a forward layer: LeakyReLU(conv + bias)
    w64, b64 = T.draw(10, 64, 3, 3, 3).double(), torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    y = T._ops(T.case("planar_c64", shape, pc=3), dict(src=dsr, w=w64, bias=b64))["y"]
    assert _close(y, F.leaky_relu(F.conv2d(dsr, w64, b64, padding=1), T.SLOPE))
    # the 64 -> 64 convolution behind the phase planes, both weight modes
    x64, w6464 = T.draw(12, n, 64, 2 * h, 2 * w).double(), T.draw(13, 64, 64, 3, 3).double()
    u = T._ops(T.case("unshuffle", shape, mode=1, bias=False), dict(x=x64, w=w6464))["planes"]
    assert _close(T.shuffle_planes(u), F.conv_transpose2d(x64, w6464, padding=1))
    u = T._ops(T.case("unshuffle", shape, mode=0), dict(x=x64, w=w6464, bias=b64))["planes"]
    assert _close(T.shuffle_planes(u), F.conv2d(x64, w6464, b64, padding=1))


def test_mask_convention_at_zero_and_subnormals():
    aux = torch.tensor([0.0, -0.0, T.SUBNORMAL, -T.SUBNORMAL, 1.0, -1.0], dtype=torch.float64, requires_grad=True)
    F.leaky_relu(aux, T.SLOPE).sum().backward()
    assert torch.equal(T.mask_factor(aux.detach(), T.SLOPE), aux.grad)
    assert T.mask_factor(aux.detach(), T.SLOPE).tolist() == [T.SLOPE, T.SLOPE, 1.0, T.SLOPE, 1.0, T.SLOPE]
    a = T.draw_aux(3, 1, 3, 5)
    assert torch.equal(T.bf16_round(a), a)                  # the subnormals and both zeros are bf16 values
    for v in (0.0, T.SUBNORMAL, -T.SUBNORMAL):
        assert int((a == v).sum()) > 0
    assert int(((a == 0) & torch.signbit(a)).sum()) > 0 and int(((a == 0) & ~torch.signbit(a)).sum()) > 0


# --------------------------------------------------------------------------------------------------------------------
# the criterion
# --------------------------------------------------------------------------------------------------------------------
DISTINCT = T.distinct(T.gpu_cases())


def test_the_case_list_covers_every_hook_shape_and_dtype():
    hooks = {"last2_fwd", "last2_dgrad", "planar_c64", "last2_wgrad", "unshuffle", "ps_dgrad", "ps_wgrads"}
    for s in T.SHAPES:
        for h in hooks:
            dts = {c.dtype for c in T.gpu_cases() if c.hook == h and c.shape == s}
            assert dts == ({"bf16"} if h in ("last2_dgrad", "unshuffle") else {"bf16", "fp32"}), (h, s, dts)
    assert any(c.shape == T.BIG_DGRAD for c in T.gpu_cases())
    assert any((c.shape[2] // c.o("scale")) % 2 == 1 for c in T.gpu_cases() if c.o("scale", 0))      # an odd LR width under the skip


@pytest.mark.parametrize("shape", T.SHAPES + [T.SKIP_SHAPES[1], T.BIG_DGRAD], ids=T.sid)
def test_same_precision_emulation_is_inside_the_bound_and_mutations_are_outside(shape):
    """Per shape (the references are computed once per operation): every distinct GPU case's emulation passes check(); at a ragged
    shape every applicable mutation of it fails, with one stated exception: `tap_mirrored` exchanges taps (1, 0) and (1, 2), which an
    image one pixel wide never meets (there the mutated evaluation must be EQUAL to the plain one)."""
    cases = [c for c in DISTINCT if c.shape == shape]
    assert cases
    n_mut = 0
    for c in cases:
        plain = T.emulate(c)
        T.check(c, plain, label="emulation")
        if not T.ragged(shape):
            continue
        for mut in T.MUTATIONS:
            if T.applicable(c, mut):
                assert not T.passes(c, T.emulate(c, mut)), (c.name, mut)
                n_mut += 1
            elif mut == "tap_mirrored":
                assert T.same_bits(T.emulate(c, mut), plain), c.name
    assert n_mut > 0 or not T.ragged(shape)


def test_a_nan_or_an_untouched_sentinel_fails_the_check():
    c = T.case("last2_dgrad", (1, 3, 5), mask="aux")
    good = T.emulate(c)
    assert T.passes(c, good)
    for bad in (float("nan"), T.SENTINEL):
        g = {"dx": good["dx"].clone()}
        g["dx"][0, 5, 1, 2] = bad
        assert not T.passes(c, g)
    c = T.case("last2_dgrad", (1, 3, 5), mask="aux", mode=1)      # ReLU mask: a masked element has the bound 0 and must be exactly 0
    g = T.emulate(c)
    assert T.passes(c, g)
    idx = (T.inputs_of(c)["aux"] <= 0).nonzero()[0]
    g["dx"][tuple(idx)] = 1e-30
    assert not T.passes(c, g)


# --------------------------------------------------------------------------------------------------------------------
# the hooks' argument checks
# --------------------------------------------------------------------------------------------------------------------
def _lib():
    from vsrlab_amd import _lib
    return _lib, _lib.load()


def _exported_vsr_symbols(path):
    """The defined `vsr_` functions of an ELF64 shared library's dynamic symbol table (.dynsym / .dynstr), read directly."""
    import struct
    data = open(path, "rb").read()
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1          # 64-bit, little-endian
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for sec in secs:
        if sec[1] != 11:                                                    # SHT_DYNSYM
            continue
        off, size, link, entsize = sec[4], sec[5], sec[6], sec[9]
        stroff = secs[link][4]
        for k in range(size // entsize):
            st_name, st_info, _, st_shndx, _, _ = struct.unpack_from("<IBBHQQ", data, off + k * entsize)
            if st_shndx != 0 and (st_info & 15) == 2:                       # defined, STT_FUNC
                end = data.index(b"\0", stroff + st_name)
                name = data[stroff + st_name:end].decode()
                if name.startswith("vsr_"):
                    names.add(name)
    return names


def test_the_hooks_are_additions_to_an_unchanged_abi():
    """The library's exported `vsr_` symbols, enumerated from its dynamic symbol table: before the hooks it exported 74 -- the 67 of
    include/vsrlab_hip.h (= EXPORTS) and 7 vsr_debug_* entries (OTHER_DEBUG_EXPORTS) -- and now exactly those plus the 7
    reconstruction-tail hooks (81), the 7 propagation-trunk hooks (88), the 7 SPyNet hooks (95), the 10 entries of the GAN side's pin
    (105: seven launch hooks, the discriminator's plan, the grid of a conv_wide2 launch and the setter of its test cap) and the 5
    flow-warp hooks (110), by name: nothing else, nothing missing.  The ABI number stays."""
    L, lib = _lib()
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vsrlab_hip.h")).read()
    declared = set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header))
    assert declared == set(L.EXPORTS) and len(L.EXPORTS) == 67 and lib.vsr_abi_version() == 4
    tail = {"vsr_debug_tail_" + k for k in ("last2_fwd", "last2_dgrad", "planar_c64", "last2_wgrad", "conv_unshuffle", "ps_dgrad", "ps_wgrads")}
    trunk = {"vsr_debug_trunk_" + k for k in ("conv", "stem", "stem_dgrad", "point", "wgrad_cc", "stem_wgrads", "chain")}
    spy = {"vsr_debug_spy_" + k for k in ("conv", "dgrad", "wgrad", "prepare", "prepare_bwd", "dres", "planar")}
    wide = {"vsr_debug_wide_" + k for k in ("conv", "wgrad", "up2_fwd", "up2_bwd", "mask", "grid")} | {"vsr_debug_vgg_pool", "vsr_debug_vgg_tap",
                                                                                                         "vsr_debug_disc_plan", "vsr_debug_wide2_set_max_wg"}
    warp = {"vsr_debug_warp_" + k for k in ("fwd", "scatter", "gather", "flowgrad", "add_cast")}
    assert len(wide) == 10
    assert len(L.OTHER_DEBUG_EXPORTS) == 7 and set(L.DEBUG_SIGNATURES) == tail | trunk | spy | wide | warp and len(tail | trunk | spy | wide | warp) == 36
    assert not set(L.DEBUG_SIGNATURES) & declared and not set(L.DEBUG_SIGNATURES) & set(L.OTHER_DEBUG_EXPORTS)
    got = _exported_vsr_symbols(L.LIB_PATH)
    before = set(L.EXPORTS) | set(L.OTHER_DEBUG_EXPORTS)
    assert got - set(L.DEBUG_SIGNATURES) == before, (sorted(got - set(L.DEBUG_SIGNATURES) - before), sorted(before - got))
    assert got - before == set(L.DEBUG_SIGNATURES) and len(got) == 81 + 7 + 7 + 10 + 5
    for name in L.DEBUG_SIGNATURES:
        assert getattr(lib, name).argtypes == L.DEBUG_SIGNATURES[name][1]


def test_hostcheck_program_passes_without_sanitizers(tmp_path):
    """tools/hr_tail_hooks_hostcheck.hip and tools/trunk_hooks_hostcheck.hip (the hooks against stubbed launches; `make hooks_hostcheck`
    runs them, and the SPyNet, wide and flow-warp programs, under ASan / UBSan) built plain and run.  The trunk program: every refusal before any pack or launch, and what the accepted
    calls hand to vsr_launch_conv, vsr_launch_wgrad, vsr_launch_wgrad_reduce and vsr_launch_conv3x3_chain (segment counts, strides, i_off,
    accumulate, layer offsets).  The tail program: every refusal before any pack or launch, every accepted call's ConvArgs as given, and -- the one check of it that
    no GPU test can make -- wgrad_launch() passes a 1- or 2-plane cotangent's plane count on to vsr_launch_last2_wgrad (it used to
    pass none, and the kernel read three planes: the surplus never reaches gw, so the values cannot show it)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    r = subprocess.run(["make", "-C", os.path.join(root, "vsrlab_amd", "csrc"), "hooks_hostcheck", "HOSTCHECK_SAN=",
                        f"HOSTCHECK_OUT={tmp_path}/hostcheck"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "\nhostcheck OK" in "\n" + r.stdout and "trunk hostcheck OK" in r.stdout and "warp hostcheck OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_hooks_refuse_null_pointers_and_bad_sizes_before_any_launch():
    _, lib = _lib()
    X, W_, B, WP, BP, Y, AUX, SC, DX, GW, GB, SL = A
    n, h, w = 2, 8, 12

    def fwd(**k):
        a = dict(dtype=BF16, x=X, w=W_, bias=B, wpack=WP, bpack=BP, y=Y, yns=3 * h * w, pres=None, base=None, bns=0, bh=0, bw=0, sc=0, co=3, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_last2_fwd(a["dtype"], a["x"], a["w"], a["bias"], a["wpack"], a["bpack"], a["y"], a["yns"], a["pres"], a["base"],
                                            a["bns"], a["bh"], a["bw"], a["sc"], a["co"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(x=None), dict(w=None), dict(wpack=None), dict(y=None), dict(bpack=None), dict(n=0), dict(h=0), dict(w_=-1), dict(co=0),
              dict(co=5), dict(yns=3 * h * w - 1), dict(base=AUX, bh=2, bw=3, sc=3, bns=18), dict(base=AUX, bh=2, bw=4, sc=4, bns=24),
              dict(base=AUX, bh=2, bw=3, sc=4, bns=17), dict(base=AUX, bh=0, bw=3, sc=4, bns=18), dict(base=AUX, bh=4, bw=6, sc=4, bns=72)):
        assert fwd(**k) == BADARG, k

    def dgrad(**k):
        a = dict(dsr=X, ns=3 * h * w, w=W_, aux=AUX, src=1, sc=SC, mode=2, dx=DX, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_last2_dgrad(a["dsr"], a["ns"], a["w"], a["aux"], a["src"], a["sc"], a["mode"], 0.1, a["dx"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dsr=None), dict(w=None), dict(dx=None), dict(n=0), dict(h=0), dict(w_=0), dict(ns=3 * h * w - 1), dict(src=3), dict(src=-1),
              dict(aux=None), dict(src=2, aux=None), dict(src=2, sc=None), dict(mode=0), dict(mode=3)):
        assert dgrad(**k) == BADARG, k

    def planar(**k):
        a = dict(dtype=BF16, src=X, ns=3 * h * w, pc=3, w=W_, bias=B, wpack=WP, y=Y, act=2, aux=None, mode=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_planar_c64(a["dtype"], a["src"], a["ns"], a["pc"], a["w"], a["bias"], a["wpack"], a["y"], a["act"], 0.1, a["aux"], a["mode"],
                                             a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=-1), dict(src=None), dict(w=None), dict(wpack=None), dict(y=None), dict(pc=2), dict(pc=0), dict(pc=4), dict(ns=3 * h * w - 1), dict(act=1),
              dict(act=3), dict(mode=2), dict(aux=AUX, mode=0), dict(aux=AUX, mode=3), dict(n=0), dict(h=0), dict(w_=0)):
        assert planar(**k) == BADARG, k

    def wgrad(**k):
        a = dict(dtype=BF16, x=X, dy=Y, ns=3 * h * w, pc=3, gw=GW, gb=GB, slab=SL, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_last2_wgrad(a["dtype"], a["x"], a["dy"], a["ns"], a["pc"], a["gw"], a["gb"], a["slab"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(x=None), dict(dy=None), dict(gw=None), dict(slab=None), dict(pc=0), dict(pc=4), dict(ns=3 * h * w - 1), dict(pc=1, ns=h * w - 1),
              dict(n=0), dict(h=0), dict(w_=0)):
        assert wgrad(**k) == BADARG, k

    def unsh(**k):
        a = dict(dtype=BF16, x=X, w=W_, bias=B, mode=0, wpack=WP, y=Y, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_conv_unshuffle(a["dtype"], a["x"], a["w"], a["bias"], a["mode"], a["wpack"], a["y"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(x=None), dict(w=None), dict(wpack=None), dict(y=None), dict(mode=2), dict(h=7), dict(w_=11), dict(n=0), dict(h=0), dict(w_=0)):
        assert unsh(**k) == BADARG, k

    def psd(**k):
        a = dict(dtype=BF16, dy=X, w=W_, wpack=WP, dx=DX, aux=None, mode=0, src=0, sc=None, dyp=0, dxp=0, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_ps_dgrad(a["dtype"], a["dy"], a["w"], a["wpack"], a["dx"], a["aux"], a["mode"], a["src"], a["sc"], a["dyp"], a["dxp"],
                                           a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(dy=None), dict(w=None), dict(wpack=None), dict(dx=None), dict(src=3), dict(src=1, mode=2), dict(src=1, aux=AUX, mode=0),
              dict(src=2, aux=AUX, mode=2), dict(dyp=2), dict(dxp=-1), dict(dxp=1, h=7), dict(dxp=1, w_=11), dict(n=0), dict(h=0), dict(w_=0)):
        assert psd(**k) == BADARG, k
    for k in (dict(dtype=F32, dyp=1), dict(dtype=F32, dxp=1), dict(dtype=F32, src=2, aux=AUX, mode=2, sc=SC), dict(dxp=1, src=1, aux=AUX, mode=2),
              dict(dxp=1, dyp=1, src=2, aux=AUX, mode=2, sc=SC)):
        assert psd(**k) == UNSUPPORTED, k                  # the fp32 recipe has the strided form and the aux mask only; no kernel masks phase planes

    def psw(**k):
        a = dict(dtype=BF16, x=X, dy=Y, dyp=0, gw=GW, gb=GB, slab=SL, n=n, h=h, w_=w)
        a.update(k)
        return lib.vsr_debug_tail_ps_wgrads(a["dtype"], a["x"], a["dy"], a["dyp"], a["gw"], a["gb"], a["slab"], a["n"], a["h"], a["w_"], None)

    for k in (dict(dtype=2), dict(x=None), dict(dy=None), dict(gw=None), dict(slab=None), dict(dyp=2), dict(n=0), dict(h=0), dict(w_=0)):
        assert psw(**k) == BADARG, k
