"""The GAN side's launches, one at a time, against the fp64 restatements of tests/wide_common.py: every output element inside the bound
stated there (grid family: equal to the reference rounded as the build stores it), every input's padding pixels NaN, every output
between sentinel bands, nothing that a ReLU mask zeroes -0, every case bit-identical on a repeat (no launch here uses atomics).  The
launches go through the ``vsr_debug_wide_*`` / ``vsr_debug_vgg_*`` hooks (csrc/wide_hooks.hip), i.e. through the WideCtx members
(csrc/wide_recipes.h), the launchers and the weight packs that disc_engine.hip and perceptual_engine.hip use;
test_hooks_on_the_engines_stored_inputs_give_the_engines_bits is the evidence that they are the engine's launches.  Both builds run
every case: bf16 reaches pack_wide2_kernel, conv_wide2_kernel<false> and <true> (K-split: the launches with 64 output rows) and the
pair-batched weight gradient; fp32 reaches pack_wide_kernel, conv_wide_kernel<float> and the pair-by-pair wgrad_block.

Shapes (N, H, W) of the conv domain, tiles 8 rows x 32 pixels: (1,1,1) and (1,2,5) -- the discriminator's coarsest levels for an 8 x 8
and a 16 x 40 frame, images smaller than the halo --; (1,8,32) exactly one tile; the ragged (2,13,37), (1,3,66), (1,9,31), (1,17,100).
conv_wide2's tile-to-tile path (DMA ring across tiles, the two drains around an epilogue, the K-split exchange through the idle tile
buffer) needs several tiles per workgroup: (1,40,200) with max_wg 3 (35 tiles, 11-12 per workgroup), (3,24,70) with max_wg 4 (a
workgroup's stride crosses image boundaries), and (3,80,352) without a cap (330 tiles on 256 workgroups); each asserts its tiles per
workgroup through vsr_debug_wide_grid.  DESIGN.md 10c has the hook -> recipe -> kernel -> test table."""
import pytest
import torch

import wide_common as W

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp32")
FAMILIES = ("rand", "grid")


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _run_all(cases, dev, dtypes=DTYPES):
    """Every case in every dtype (the dtype innermost: the two builds share one cached reference); bit-identical on a repeat."""
    got = {}
    for c0 in cases:
        for dt in dtypes:
            c = W.Case(c0.hook, c0.shape, dt, c0.opts)
            got[c] = W.run_hip(c, dev)
            W.check(c, got[c])
            assert W.same_bits(got[c], W.run_hip(c, dev)), (c.name, "differs on a repeat")
    return got


GEOMETRIES = W.conv_geometries()


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.sid)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_conv(geo, shape):
    """WideCtx::wide on the weight image of its mode, at every geometry the two engines launch: the discriminator's 3x3 layers
    (LeakyReLU; conv_6 with y_act + res), VGG's (bias + ReLU; conv5_4 without), the 4x4 stride-2 layers over their parity views, the
    discriminator's plain 3x3 data gradients, VGG's with the ReLU mask (slope 0: +0), and the four output phases of the stride-2 data
    gradient with res + aux on the phase-strided destination."""
    _run_all([W.case("conv", shape, family=fam, **geo[1]) for fam in FAMILIES], _gpu())


@pytest.mark.parametrize("shape,max_wg", W.MANY, ids=lambda v: W.sid(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("geo", W.MANY_GEOMETRIES, ids=[g[0] for g in W.MANY_GEOMETRIES])
def test_conv_many_tiles_per_workgroup(geo, shape, max_wg):
    """conv_wide2 with the workgroups per column capped by the launch's own max_wg: one geometry per kernel form (one slice, two slices,
    K-split, four parity views, K-split with phases), at least 3 tiles per workgroup (asserted on the launcher's grid)."""
    dev = _gpu()
    from vsrlab_amd import _lib
    cases = [W.case("conv", shape, family=fam, max_wg=max_wg, **geo[1]) for fam in FAMILIES]
    nwx, cols, tiles = W.grid_of(_lib.load(), *W.launch_ncob(cases[0]), shape, max_wg)
    assert nwx == max_wg and tiles // nwx >= 3, (nwx, cols, tiles)
    _run_all(cases, dev, ("bf16",))


def test_conv_many_tiles_without_a_cap():
    """64 -> 128 at (3,80,352): 330 tiles on min(CUs, 330) workgroups of one column, no cap: the engines' own grid."""
    dev = _gpu()
    from vsrlab_amd import _lib
    cases = [W.case("conv", W.UNCAPPED, family=fam, **W.MANY_GEOMETRIES[0][1]) for fam in FAMILIES]
    nwx, cols, tiles = W.grid_of(_lib.load(), 2, 1, W.UNCAPPED, 0)
    assert cols == 1 and tiles == 330 and nwx < tiles, (nwx, cols, tiles)
    _run_all(cases, dev, ("bf16",))


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.sid)
@pytest.mark.parametrize("geo", W.WGRAD_GEOMETRIES, ids=lambda g: "v%d_%d_%d" % g)
def test_wgrad(geo, shape):
    """WideCtx::wgrad_layer into a pre-filled gradient: bf16 every (view, cout block, cin slice) pair in one launch of
    wgrad3x3_c64_pc_kernel + wgrad_reduce_pairs_kernel (at (1,1,1) seven of eight pixel parts hold no tile; the slab buffer is filled with a
    sentinel), fp32 pair by pair through wgrad_block (+ wgrad_reduce_s2_kernel's scatter into the 4x4 gradient)."""
    views, xC, dyC = geo
    _run_all([W.case("wgrad", shape, views=views, xC=xC, dyC=dyC, family=fam) for fam in FAMILIES], _gpu())


@pytest.mark.parametrize("geo", [(1, 128, 64), (4, 64, 128)], ids=lambda g: "v%d_%d_%d" % g)
def test_wgrad_several_tiles_per_part(geo):
    views, xC, dyC = geo
    _run_all([W.case("wgrad", W.WG_MANY, views=views, xC=xC, dyC=dyC, family=fam) for fam in FAMILIES], _gpu())


@pytest.mark.parametrize("C", (128, 256, 512))
@pytest.mark.parametrize("hw", W.UP2_SOURCES, ids=W.sid)
def test_up2(hw, C):
    """vsr_launch_up2_fwd with b and without, vsr_launch_up2_bwd with (din, dmask) and with dmask alone, at 1 x 1 and 1 x k sources (every
    neighbour clamped) upward; slope 0.2 and 0 (then what the mask zeroes is +0).  An up2 of a constant image is that constant, bit for bit."""
    dev = _gpu()
    h, w = hw
    for n in (1, 2):
        cs = []
        for fam in FAMILIES:
            cs += [W.case("up2_fwd", (n, h, w), C=C, b=1, family=fam), W.case("up2_fwd", (n, h, w), C=C, b=0, family=fam),
                   W.case("up2_bwd", (n, h, w), C=C, din=1, family=fam), W.case("up2_bwd", (n, h, w), C=C, din=0, family=fam),
                   W.case("up2_bwd", (n, h, w), C=C, din=0, slope=0.0, family=fam)]
        _run_all(cs, dev)
    for dt in DTYPES:
        c = W.case("up2_fwd", (1, h, w), dt, C=C, b=0)
        const = torch.full((1, C, h, w), 0.30078125)
        got = W.run_hip(c, dev, given=dict(a=const))
        assert W.same_bits(got, dict(out=torch.full((1, C, 2 * h, 2 * w), 0.30078125))), (c.name, "an up2 of a constant is not that constant")


@pytest.mark.parametrize("C", (64, 512))
@pytest.mark.parametrize("shape", W.SHAPES, ids=W.sid)
def test_mask(shape, C):
    """vsr_launch_mask_pm at slope 0.2 and at 0 (what it zeroes is +0), m with +-0 and +-2^-133 on the first and last column."""
    cs = [W.case("mask", shape, C=C, slope=sl, family=fam) for fam in FAMILIES for sl in (W.SLOPE, 0.0)]
    _run_all(cs, _gpu())


@pytest.mark.parametrize("C", (64, 512))
@pytest.mark.parametrize("hw", W.POOL_INPUTS, ids=W.sid)
def test_vgg_pool(hw, C):
    """maxpool2_fwd_kernel: equal to F.max_pool2d bit for bit; maxpool2_bwd_kernel: g <- (g + route(dp)) (a > 0) with ties in most windows
    (the first maximum in row-major order), rows and columns the floor drops masked all the same."""
    dev = _gpu()
    h, w = hw
    for n in (1, 2):
        got = _run_all([W.case("pool_fwd", (n, h, w), C=C, family="grid"), W.case("pool_bwd", (n, h, w), C=C, family="grid"),
                        W.case("pool_bwd", (n, h, w), C=C, family="rand")], dev)
        for c, v in got.items():
            if c.hook == "pool_fwd":
                want = torch.nn.functional.max_pool2d(W.inputs_of(c)["a"], 2, 2)
                assert W.same_bits(v, dict(out=want)), (c.name, "differs from max_pool2d in bits")


@pytest.mark.parametrize("C", (64, 512))
@pytest.mark.parametrize("hw", W.POOL_INPUTS, ids=W.sid)
def test_vgg_tap(hw, C):
    """tap_l1_kernel + tap_sum_kernel: sum |s - h| per image over real pixels, scale sign(s - h) written over h (a quarter of the elements
    with s == h exactly: 0), with and without the gradient.  An image's sum has the same bits alone and second in a batch."""
    dev = _gpu()
    h, w = hw
    got = _run_all([W.case("tap", (2, h, w), C=C, grad=g, family=fam) for fam in FAMILIES for g in (1, 0)], dev)
    for c, v in got.items():
        if c.o("grad") == 1:
            t = W.inputs_of(c)
            alone = W.Case(c.hook, (1, h, w), c.dtype, c.opts)
            one = W.run_hip(alone, dev, given=dict(s=t["s"][1:2].contiguous(), h=t["h"][1:2].contiguous()))
            assert torch.equal(one["sums"].view(torch.int64), v["sums"][1:2].view(torch.int64)), (c.name, "an image's sum depends on its batch")


# --------------------------------------------------------------------------------------------------------------------
# the hooks are the engine's launches
# --------------------------------------------------------------------------------------------------------------------
_ACT = ("f0", "f1", "f2", "f3", "u3", "a4", "u4", "a5", "u5", "a6", "s6", "o7", "o8")
_BWD = ("d_o8", "d_o7", "G6", "dc6", "du5", "ds5", "dc5", "du4", "ds4", "dc4", "du3", "dc3", "dc2", "dc1", "dc0", "slab")
# name -> (channels, level: the tensor is (h >> level, w >> level))
_GEOM = dict(f0=(64, 0), f1=(128, 1), f2=(256, 2), f3=(512, 3), u3=(512, 2), a4=(256, 2), u4=(256, 1), a5=(128, 1), u5=(128, 0), a6=(64, 0), s6=(64, 0),
             G6=(64, 0), dc6=(64, 0), du5=(128, 0), ds5=(128, 1), dc5=(128, 1), du4=(256, 1), ds4=(256, 2), dc4=(256, 2), du3=(512, 2), dc3=(512, 3),
             dc2=(256, 2), dc1=(128, 1), dc0=(64, 0))
_SHAPES = [(64, 3, 3, 3), (64,), (128, 64, 4, 4), (256, 128, 4, 4), (512, 256, 4, 4), (256, 512, 3, 3), (128, 256, 3, 3), (64, 128, 3, 3), (64, 64, 3, 3),
           (64, 64, 3, 3), (1, 64, 3, 3), (1,)]


def _disc_engine(lib, dev, dtype, img, cot, params):
    """vsr_disc_forward(need_backward=1) + vsr_disc_backward on a caller-held workspace; the stored tensors by name (planar fp32, CPU; the
    backward scratch is the last frame's), the 12 gradients."""
    import ctypes
    from vsrlab_amd import _lib as L
    from vsrlab_amd import functional as VF
    n, _, h, w = img.shape
    dt = VF.DT_BF16 if dtype == "bf16" else VF.DT_F32
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    es = 2 if dtype == "bf16" else 4
    d = L.DiscDesc(n, h, w, 64, dt)
    off = (ctypes.c_longlong * 30)()
    assert lib.vsr_debug_disc_plan(ctypes.byref(d), 1, off, 30) == 0
    off = dict(zip(_ACT + _BWD + ("total",), list(off)))
    ws = torch.zeros(off["total"], dtype=torch.uint8, device=dev)
    st = VF._stream()
    out = torch.empty(n, 1, h, w, device=dev)
    dimg = torch.empty(n, 3, h, w, device=dev)
    grads = [torch.zeros_like(p) for p in params]
    imgd, cotd = img.to(dev).contiguous(), cot.to(dev).contiguous()
    assert lib.vsr_disc_forward(ctypes.byref(d), VF._ptr_array(params), 12, imgd.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), 1, st) == 0
    assert lib.vsr_disc_backward(ctypes.byref(d), VF._ptr_array(grads), 12, imgd.data_ptr(), cotd.data_ptr(), dimg.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    W.T._sync()
    stored = {}
    for name, (C, lv) in _GEOM.items():
        nn, hh, ww = (n if name in _ACT else 1), h >> lv, w >> lv
        shape = (nn, hh, (ww + 31) // 32, C // 8, 32, 8)
        numel = int(torch.tensor(shape).prod())
        v = ws[off[name]:off[name] + numel * es].view(tdt).view(shape)
        stored[name] = W.from_pm(v.cpu(), ww)
    return stored, [g.cpu() for g in grads]


@pytest.mark.parametrize("n", (1, 2))
@pytest.mark.parametrize("dtype", DTYPES)
def test_hooks_on_the_engines_stored_inputs_give_the_engines_bits(dtype, n):
    """(n,3,16,40) frames.  Every wide launch of disc_forward and (for the last frame) of disc_backward, re-run through its hook on what
    the engine stored as the launch's input (read at vsr_debug_disc_plan's offsets), gives the engine's stored output bit for bit -- f1, f2,
    f3, u3, a4, u4, a5, u5, a6, s6; dc6, du5, ds5, dc5, du4, ds4, dc4, du3, dc3, dc2, dc1, dc0 -- and the hooks' weight gradients, added
    frame by frame in the engine's order, are the engine's g[2..7].  Each of these tensors is also inside the bound of the fp64
    restatement of its layer applied to the stored input, layer by layer.  The scratch of an earlier frame comes from the engine run on
    that frame alone, whose activations are first shown to be the batch's, bit for bit."""
    dev = _gpu()
    from vsrlab_amd import _lib
    lib = _lib.load()
    h, w = 16, 40
    params = [(W.bf16_round(W.draw(700 + i, *s) / (max(int(torch.tensor(s[1:]).prod()), 1) ** 0.5))).to(dev) for i, s in enumerate(_SHAPES)]
    g = torch.Generator().manual_seed(5)
    img = torch.rand(n, 3, h, w, generator=g)
    cot = torch.rand(n, 1, h, w, generator=g) * 2 - 1
    S, G = _disc_engine(lib, dev, dtype, img, cot, params)
    wt = [p.cpu() for p in params]

    def hook(want, c, given, key="y", store=None):
        got = W.run_hip(c, dev, given=given)
        for k, name in ([(key, want)] if isinstance(want, str) else want):
            assert W.same_bits({k: got[k]}, {k: (store or S)[name]}), (c.name, k, "the hook's bits are not the engine's")
        W.check(c, got, given=given)
        return got

    conv = lambda shape, **o: W.case("conv", shape, dtype, **o)
    # ---- forward, the whole batch ----
    for k, (src, dst, ci, co) in enumerate([("f0", "f1", 64, 128), ("f1", "f2", 128, 256), ("f2", "f3", 256, 512)]):
        hook(dst, conv((n, h >> (k + 1), w >> (k + 1)), mode=1, cin=ci, cout=co, act=W.ACT_LEAKY), dict(x=S[src], w=wt[2 + k]))
    hook("u3", W.case("up2_fwd", (n, h // 8, w // 8), dtype, C=512, b=0), dict(a=S["f3"]), "out")
    hook("a4", conv((n, h // 4, w // 4), mode=0, cin=512, cout=256, act=W.ACT_LEAKY), dict(x=S["u3"], w=wt[5]))
    hook("u4", W.case("up2_fwd", (n, h // 4, w // 4), dtype, C=256, b=1), dict(a=S["a4"], b=S["f2"]), "out")
    hook("a5", conv((n, h // 2, w // 2), mode=0, cin=256, cout=128, act=W.ACT_LEAKY), dict(x=S["u4"], w=wt[6]))
    hook("u5", W.case("up2_fwd", (n, h // 2, w // 2), dtype, C=128, b=1), dict(a=S["a5"], b=S["f1"]), "out")
    hook([("y", "s6"), ("y_act", "a6")], conv((n, h, w), mode=0, cin=128, cout=64, act=W.ACT_LEAKY, y_act=1, res=1), dict(x=S["u5"], w=wt[7], res=S["f0"]))

    # ---- backward: frame by frame, against the scratch of the engine on frame f alone (the last frame's: the batch's own) ----
    gw = {k: torch.zeros_like(wt[k]) for k in range(2, 8)}
    for f in range(n):
        if f == n - 1:
            Sf = {k: (v[f:f + 1] if k in _ACT else v) for k, v in S.items()}
        else:
            Sf, _ = _disc_engine(lib, dev, dtype, img[f:f + 1], cot[f:f + 1], params)
            for k in _ACT[:11]:
                assert W.same_bits(dict(v=Sf[k]), dict(v=S[k][f:f + 1])), (k, "a frame's activations depend on its batch")
        bh = lambda want, c, given, key="y", Sf=Sf: hook(want, c, given, key, Sf)

        def wg(k, views, xname, dyname, lv):
            c = W.case("wgrad", (1, h >> lv, w >> lv), dtype, views=views, xC=wt[k].shape[1], dyC=wt[k].shape[0])
            given = dict(x=Sf[xname], dy=Sf[dyname], gw0=gw[k])
            got = W.run_hip(c, dev, given=given)
            W.check(c, got, given=given)
            gw[k] = got["gw"]

        bh("dc6", W.case("mask", (1, h, w), dtype, C=64), dict(g=Sf["G6"], m=Sf["a6"]), "out")
        bh("du5", conv((1, h, w), mode=2, cout=64, cin=128), dict(x=Sf["dc6"], w=wt[7]))
        wg(7, 1, "u5", "dc6", 0)
        bh([("din", "ds5"), ("dmask", "dc5")], W.case("up2_bwd", (1, h // 2, w // 2), dtype, C=128, din=1), dict(dout=Sf["du5"], m=Sf["a5"]))
        bh("du4", conv((1, h // 2, w // 2), mode=2, cout=128, cin=256), dict(x=Sf["dc5"], w=wt[6]))
        wg(6, 1, "u4", "dc5", 1)
        bh([("din", "ds4"), ("dmask", "dc4")], W.case("up2_bwd", (1, h // 4, w // 4), dtype, C=256, din=1), dict(dout=Sf["du4"], m=Sf["a4"]))
        bh("du3", conv((1, h // 4, w // 4), mode=2, cout=256, cin=512), dict(x=Sf["dc4"], w=wt[5]))
        wg(5, 1, "u3", "dc4", 2)
        bh("dc3", W.case("up2_bwd", (1, h // 8, w // 8), dtype, C=512, din=0), dict(dout=Sf["du3"], m=Sf["f3"]), "dmask")
        bh("dc2", conv((1, h // 8, w // 8), mode=3, cout=512, cin=256, res=1, aux=1), dict(x=Sf["dc3"], w=wt[4], res=Sf["ds4"], aux=Sf["f2"]))
        wg(4, 4, "f2", "dc3", 3)
        bh("dc1", conv((1, h // 4, w // 4), mode=3, cout=256, cin=128, res=1, aux=1), dict(x=Sf["dc2"], w=wt[3], res=Sf["ds5"], aux=Sf["f1"]))
        wg(3, 4, "f1", "dc2", 2)
        bh("dc0", conv((1, h // 2, w // 2), mode=3, cout=128, cin=64, res=1, aux=1), dict(x=Sf["dc1"], w=wt[2], res=Sf["G6"], aux=Sf["f0"]))
        wg(2, 4, "f0", "dc1", 1)
    for k in range(2, 8):
        assert W.same_bits(dict(g=gw[k]), dict(g=G[k])), (k, "the hooks' weight gradient, added over the frames, is not the engine's")
