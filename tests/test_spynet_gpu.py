"""SPyNet's launches, one at a time, against the fp64 restatements of tests/spynet_common.py: every output element inside the bound stated
there (grid family: equal to the reference, or to its bf16 rounding), every input's padding pixels NaN, every output between sentinel
bands.  The launches go through the ``vsr_debug_spy_*`` hooks (csrc/spynet_hooks.hip), i.e. through the Ctx members, the launchers and
the weight packs spynet_engine.hip uses; test_hooks_in_the_order_of_spynet_run_give_the_engines_bits is the evidence that they are the
engine's launches.  Both builds run every case; the fp32 build runs conv_mfma.hip's / wgrad_mfma.hip's generic ks = 7 kernels and the
two-half weight gradient of the 64-channel layer.

Shapes (N, H, W) of the three 7x7 hooks, tiles 8 rows x 32 pixels: the engine's own coarse levels (1,1,1), (1,2,2), (1,4,4), (2,8,16) --
images smaller than the kernels' halo --; the tail's ragged list; (3,80,352), 330 tiles on 256 workgroups: a QTileIter crosses an image
boundary; (4,200,330), 1100 tiles (grid family, bf16, forward and masked data gradient): the resident layers' tile buffers and both
buffers of the streamed ones are re-used several times; (3,72,200) for the weight gradient (grid family, accumulate): several tiles per
workgroup of every kernel row.

Which case reaches which code in the bf16 build ("SPyNet, launch by launch" has the table): conv j = 0..4 -> C7<16,2> (tap
pairs, resident), C7<32,4> (streamed), C7<64,2> (two passes, streamed), C7<32,1> (resident), C7<16,1,PLANAR> (tap pairs, resident, +
pres); dgrad j = 0..4 -> C7<32,1>, C7<64,2>, C7<32,4>, C7<16,2>, C7<16,1>, with the q_relu_mask arm for j > 0; wgrad j = 0..4 ->
W7<16,32>, W7<32,64>, W7<64,32>, W7<32,16>, W7<16,16>."""
import pytest
import torch

import hr_tail_common as T
import spynet_common as S

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _run_all(cases, dev, dtypes=("bf16", "fp32"), repeat=True):
    """Every case in every dtype (the dtype innermost: the two builds share one cached reference); bit-identical on a repeat."""
    got = {}
    for c0 in cases:
        for dt in dtypes:
            c = S.Case(c0.hook, c0.shape, dt, c0.opts)
            got[c] = S.run_hip(c, dev)
            S.check(c, got[c])
            if repeat and c.hook not in S.ATOMIC:
                assert S.same_bits(got[c], S.run_hip(c, dev)), (c.name, "differs on a repeat")
    return got


def _conv_cases(make, shape, j):
    return [c for fam in S.families(shape, "bf16") for c in make(shape, "bf16", fam) if c.o("j") == j]


def _no_negative_zero(c, got, key, masked):
    """What a ReLU mask zeroes is +0."""
    assert not bool((torch.signbit(got[key]) & masked & (got[key] == 0)).any()), (c.name, "a masked element is -0")


@pytest.mark.parametrize("j", range(5))
@pytest.mark.parametrize("shape", S.conv_shapes("conv"), ids=T.sid)
def test_conv(shape, j):
    """Ctx::spy_conv(j) on Ctx::pack_spy(j, ., 0): bias + ReLU; the last layer planar fp32 with and without ReLU and pres."""
    _run_all(_conv_cases(S.conv_cases, shape, j), _gpu(), S.dtypes(shape))


@pytest.mark.parametrize("j", range(5))
@pytest.mark.parametrize("shape", S.conv_shapes("dgrad"), ids=T.sid)
def test_dgrad(shape, j):
    """Ctx::spy_dgrad(j) on Ctx::pack_spy(j, ., 1): plain (j = 0, 2, 4) and ReLU-masked from aux with +-0 and +-2^-133 on the first and the
    last column (j > 0): `> 0` passes, everything else is +0."""
    got = _run_all(_conv_cases(S.dgrad_cases, shape, j), _gpu(), S.dtypes(shape))
    for c, v in got.items():
        if c.o("aux", 0):
            _no_negative_zero(c, v, "dx", ~(S.inputs_of(c)["aux"] > 0))


@pytest.mark.parametrize("j", range(5))
@pytest.mark.parametrize("shape", S.conv_shapes("wgrad"), ids=T.sid)
def test_wgrad(shape, j):
    """Ctx::spy_wgrad(j): overwriting and accumulating into a pre-filled gradient, gb given and NULL (then untouched); the reduction order
    is fixed: bit-identical on a repeat."""
    _run_all(_conv_cases(S.wgrad_cases, shape, j), _gpu())


@pytest.mark.parametrize("size", S.LEVEL0 + S.LEVELS, ids=T.sid)
def test_level_launches(size):
    """At one level size, for P from pair_mode 0 with (n, t) = (1, 2), (2, 3) and pair_mode 1 with P = 1, 3: vsr_launch_spynet_prepare (level
    0: no flow below; else the x2 align_corners=True upsample, from a 1 x 1 flow at (2,2)) and vsr_launch_spynet_prepare_bwd in the
    engine's three forms (level 0 into the frames; above, with and without them); vsr_launch_spynet_dres with res (+-0, +-2^-133 on the
    first and last column) and without; vsr_launch_add_f32; vsr_launch_avgpool2 and its adjoint.  The atomic adjoint is held to the bound only, the rest are also bit-identical on a repeat."""
    got = _run_all(S.level_cases(size, "bf16"), _gpu())
    for c, v in got.items():
        if c.hook == "dres" and c.o("res", 1):
            res = S.inputs_of(c)["res"]
            _no_negative_zero(c, v, "y", torch.cat([~(res > 0), torch.ones(res.shape[0], 14, *res.shape[2:], dtype=torch.bool)], 1))


@pytest.mark.parametrize("src,dst", S.RESIZES, ids=lambda v: T.sid(v))
def test_resizes(src, dst):
    """vsr_launch_resize_norm / _bwd and vsr_launch_flow_out / _bwd from (h, w) to the /32 size and back.  The identity (32,64) is exact:
    flow_out returns its input's bits, resize_norm (x - mean) / std as fp32 computes it."""
    dev = _gpu()
    got = _run_all(S.resize_cases(src, dst, "bf16"), dev)
    if src == dst:
        for c, v in got.items():
            t = S.inputs_of(c)
            if c.hook == "flow_out":
                assert S.same_bits(v, dict(y=t["x"])), c.name
            if c.hook == "resize_norm":
                assert S.same_bits(v, dict(y=(t["x"] - t["mean"].view(1, 3, 1, 1)) / t["std"].view(1, 3, 1, 1))), c.name


@pytest.mark.parametrize("last_relu", (1, 0))
@pytest.mark.parametrize("dtype", ("bf16", "fp32"))
def test_hooks_in_the_order_of_spynet_run_give_the_engines_bits(dtype, last_relu):
    """N = 1, 64 x 64.  The forward driven through the hooks in the order of spynet_run -- resize_norm, five avgpool2, per level prepare + five
    convs (the last with pres = flow_up; on the saving path without, then add_f32), flow_out -- equals vsr_spynet_forward_ex bit for bit
    at every level_out, without and with need_backward (the saving path), and with last_relu vsr_spynet_forward's flow."""
    dev = _gpu()
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    dt = VF.DT_BF16 if dtype == "bf16" else VF.DT_F32
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    st = VF._stream()
    h = w = 64
    params = []
    for l in range(6):
        for j in range(5):
            params += [(T.draw(500 + 10 * l + j, S.CO[j], S.CI[j], 7, 7) / (7.0 * S.CI[j] ** 0.5)).to(dev), (T.draw(600 + 10 * l + j, S.CO[j]) * 0.1).to(dev)]
    params += [torch.tensor([0.485, 0.456, 0.406], device=dev), torch.tensor([0.229, 0.224, 0.225], device=dev)]
    g = torch.Generator().manual_seed(77)
    ref, supp = torch.rand(1, 3, h, w, generator=g).to(dev), torch.rand(1, 3, h, w, generator=g).to(dev)
    P = lambda t: None if t is None else t.data_ptr()

    def engine(need_bwd):
        ws = torch.empty(lib.vsr_spynet_workspace_bytes(1, h, w, dt, need_bwd), dtype=torch.uint8, device=dev)
        outs = [torch.full((1, 2, h >> (5 - l), w >> (5 - l)), float("nan"), device=dev) for l in range(6)]
        rc = lib.vsr_spynet_forward_ex(1, h, w, dt, VF._ptr_array(params), 62, P(ref), P(supp), last_relu, VF._ptr_array(outs), P(ws), ws.numel(), need_bwd, st)
        assert rc == 0, rc
        T._sync()
        return outs

    def hooks(save):
        ok = lambda rc: None if rc == 0 else pytest.fail(f"a hook returned {rc}")
        planar = lambda op, a, b, out, planes, hh, ww, hu=0, wu=0: ok(lib.vsr_debug_spy_planar(op, P(a), P(b), P(out), P(params[60]), P(params[61]), planes, hh, ww, hu, wu, st))
        pyr = [torch.empty(2, 3, h >> (5 - l), w >> (5 - l), device=dev) for l in range(6)]
        planar(0, torch.cat([ref, supp]).contiguous(), None, pyr[5], 2, h, w, h, w)
        for l in range(5, 0, -1):
            planar(2, pyr[l], None, pyr[l - 1], 6, h >> (5 - l), w >> (5 - l))
        wpack = torch.empty(49 * 64 * 64, dtype=tdt, device=dev)
        fprev, outs = None, []
        for l in range(6):
            hl, wl = h >> (5 - l), w >> (5 - l)
            pmbuf = lambda C: torch.zeros(1, hl, (wl + 31) // 32, C // 8, 32, 8, dtype=tdt, device=dev)
            fup, fcur, x = torch.empty(1, 2, hl, wl, device=dev), torch.empty(1, 2, hl, wl, device=dev), pmbuf(16)
            ok(lib.vsr_debug_spy_prepare(dt, P(pyr[l]), P(fprev), P(fup), P(x), 0, 0, 1, 1, hl, wl, int(l == 0), st))
            for j in range(5):
                act = 1 if (j < 4 or last_relu) else 0
                wt, b = params[(l * 5 + j) * 2], params[(l * 5 + j) * 2 + 1]
                if j < 4:
                    y = pmbuf(S.CD[j])
                    ok(lib.vsr_debug_spy_conv(dt, j, P(x), P(wt), P(b), P(wpack), P(y), act, None, 1, hl, wl, st))
                    x = y
                elif save:
                    res = torch.empty(1, 2, hl, wl, device=dev)
                    ok(lib.vsr_debug_spy_conv(dt, j, P(x), P(wt), P(b), P(wpack), P(res), act, None, 1, hl, wl, st))
                    planar(6, fup, res, fcur, 2, hl, wl)
                else:
                    ok(lib.vsr_debug_spy_conv(dt, j, P(x), P(wt), P(b), P(wpack), P(fcur), act, P(fup), 1, hl, wl, st))
            out = torch.full((1, 2, hl, wl), float("nan"), device=dev)
            planar(4, fcur, None, out, 1, hl, wl, hl, wl)
            outs.append(out)
            fprev = fcur
        T._sync()
        return outs

    for need_bwd in (0, 1):
        want, got = engine(need_bwd), hooks(bool(need_bwd))
        for l in range(6):
            assert torch.equal(want[l].view(torch.int32), got[l].view(torch.int32)), (dtype, last_relu, need_bwd, "level", l, float((want[l] - got[l]).abs().max()))
        if last_relu:
            ws = torch.empty(lib.vsr_spynet_workspace_bytes(1, h, w, dt, need_bwd), dtype=torch.uint8, device=dev)
            flow = torch.full((1, 2, h, w), float("nan"), device=dev)
            rc = lib.vsr_spynet_forward(1, h, w, dt, VF._ptr_array(params), 62, P(ref), P(supp), P(flow), P(ws), ws.numel(), need_bwd, st)
            assert rc == 0, rc
            T._sync()
            assert torch.equal(flow.view(torch.int32), got[5].view(torch.int32)), (dtype, need_bwd, "vsr_spynet_forward")
