"""The reconstruction-tail kernels, one launch at a time, against the fp64 restatements of tests/hr_tail_common.py: every output
element inside the bound stated there, every input's padding pixels NaN, every output between sentinel bands.  The launches go
through the ``vsr_debug_tail_*`` hooks (csrc/hr_tail_hooks.hip), i.e. through the recipes and weight packs the engines use.

Shapes (N, H, W), tiles 8 rows x 32 pixels: (1,1,1); (1,8,32) one whole tile; (2,13,37); (1,3,66) a 2-pixel tail, W % 4 != 0;
(1,9,31); (1,17,100) ragged with W % 4 == 0; (3,80,352) 330 tiles: more than one per persistent workgroup, both LDS buffers re-used.
Pixel-shuffle cases take (H, W) as the layer's INPUT size (its gradient is 2H x 2W); `unshuffle` and the `dx_planes` data gradient,
whose output has to be even-sized, run at 2H x 2W.

Which case reaches which kernel (bf16 build; the fp32 build runs conv_mfma.hip's / wgrad_mfma.hip's generic kernels on the same cases):
  hr_tail.hip
    last2_dgrad_kernel<0, false>     test_last2_dgrad            mask=none
    last2_dgrad_kernel<1, false>     test_last2_dgrad            mask=aux  (+ (4,168,790): 2100 tiles on 2048 workgroups)
    last2_dgrad_kernel<2, false>     test_last2_dgrad            mask=bits (sign bits from vsr_launch_sign_bits_c64)
    last2_dgrad_kernel<0, true>      test_planar_c64             pc=3 (stem / conv_0: bias + LeakyReLU)
    last2_dgrad_kernel<1, true>      test_planar_c64             pc=1,mask=aux (conv_9's data gradient); pc=3,mask=aux
    c64_to_planar_kernel             test_last2_fwd              cout_real 1..4, bias, planar residual, destination stride
                                     test_last2_fwd_bilinear_skip   co=3,scale=4: the 3-channel fast path; the others: bil_src's path
    last2_wgrad_ring_kernel          test_last2_wgrad            W in {32, 100, 352} (W % 4 == 0, cotangent 16-byte aligned)
    last2_wgrad_kernel               test_last2_wgrad            W in {1, 37, 66, 31}; and W in {32, 100, 352} with the cotangent one
                                                                 float off its alignment (misalign=1)
  recipes.h
    ConvArgs::unshuffle              test_conv_unshuffle (Ctx::conv), test_ps_dgrad_dx_planes (Ctx::conv_ps_dgrad, residual in planes)
    dy_planes                        test_ps_dgrad dy_planes=1, test_ps_wgrads dy_planes=1
    dx_planes                        test_ps_dgrad_dx_planes
    strided forms                    test_ps_dgrad / test_ps_wgrads dy_planes=0 (what vsr_conv_layer_bwd runs)"""
import pytest
import torch

import hr_tail_common as T

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp32"]
shapes = pytest.mark.parametrize("shape", T.SHAPES, ids=T.sid)
dtypes = pytest.mark.parametrize("dtype", DTYPES)


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _run(c, dev):
    got = T.run_hip(c, dev)
    T.check(c, got)
    return got


@dtypes
@shapes
def test_last2_fwd(dtype, shape):
    """conv_last.2 / the pre-clean out conv / conv_9 forward: 64 -> 1..4 channels, planar fp32."""
    dev = _gpu()
    for c in T.fwd_cases(shape, dtype):
        _run(c, dev)


@dtypes
@pytest.mark.parametrize("shape", T.SKIP_SHAPES, ids=T.sid)
def test_last2_fwd_bilinear_skip(dtype, shape):
    """... + the bilinear skip of an LR frame of exactly H/scale x W/scale, scale 4 and 2; (2,12,36): the LR width 9 is odd."""
    dev = _gpu()
    for c in T.skip_cases(shape, dtype):
        _run(c, dev)


@pytest.mark.parametrize("shape", T.SHAPES + [T.BIG_DGRAD], ids=T.sid)
def test_last2_dgrad(shape):
    """conv_last.2's data gradient in its three mask modes; the mask from aux and from aux's sign bits give the same bits, at the exact
    zeros and subnormals of aux too."""
    dev = _gpu()
    cases = T.dgrad_cases(shape) if shape != T.BIG_DGRAD else [T.case("last2_dgrad", shape, mask="aux"), T.case("last2_dgrad", shape, mask="bits")]
    got = {c: _run(c, dev) for c in cases}
    assert T.same_bits(got[T.case("last2_dgrad", shape, mask="aux")], got[T.case("last2_dgrad", shape, mask="bits")])
    if shape != T.BIG_DGRAD:
        assert T.same_bits(got[T.case("last2_dgrad", shape, mask="aux")], got[T.case("last2_dgrad", shape, mask="aux", nstride_mul=2)])
        relu_aux = T.run_hip(T.case("last2_dgrad", shape, mask="aux", mode=1), dev)
        assert T.same_bits(relu_aux, got[T.case("last2_dgrad", shape, mask="bits", mode=1)])


@dtypes
@shapes
def test_planar_c64(dtype, shape):
    """planar fp32 (1 or 3 planes) -> 64 channels: the pre-clean stem, the discriminator's conv_0 and conv_9's data gradient."""
    dev = _gpu()
    for c in T.planar_cases(shape, dtype):
        _run(c, dev)


@dtypes
@shapes
def test_last2_wgrad(dtype, shape):
    """Weight and bias gradient of a 64 -> pc conv with a planar cotangent of pc = 1, 2, 3 planes, images 3HW and 6HW apart (frame 1 of a
    2-frame cotangent).  bf16: the ring kernel where W % 4 == 0, the plain kernel elsewhere and -- at the same widths -- with the
    cotangent one float off its 16-byte alignment.  Bit-identical on a repeat."""
    dev = _gpu()
    cases = T.wgrad_cases(shape, dtype)
    if dtype == "bf16" and shape[2] % 4 == 0:
        cases += [T.case("last2_wgrad", shape, dtype, pc=3, misalign=1), T.case("last2_wgrad", shape, dtype, pc=1, misalign=1, nstride_mul=2)]
    for c in cases:
        got = _run(c, dev)
        if c.o("pc") == 3:
            assert T.same_bits(got, T.run_hip(c, dev)), c.name


@shapes
def test_conv_unshuffle(shape):
    """Ctx::conv(..., unshuffle = true): a 64 -> 64 3x3 of a 2H x 2W image written as four phase planes (forward and data-gradient weights)."""
    dev = _gpu()
    for c in T.unshuffle_cases(shape):
        _run(c, dev)


@dtypes
@shapes
def test_ps_dgrad(dtype, shape):
    """Ctx::conv_ps_dgrad: no mask, LeakyReLU mask from aux and (bf16) from sign bits; dy strided and (bf16) phase-separated: same bits."""
    dev = _gpu()
    got = {c: _run(c, dev) for c in T.ps_dgrad_cases(shape, dtype)}
    if dtype == "bf16":
        k = lambda **o: T.case("ps_dgrad", shape, dtype, **o)
        assert T.same_bits(got[k()], got[k(dy_planes=1)])
        assert T.same_bits(got[k(mask="bits")], got[k(mask="bits", dy_planes=1)])
        assert T.same_bits(got[k(mask="aux")], got[k(mask="bits")])


@shapes
def test_ps_dgrad_dx_planes(shape):
    """dx written phase-separated (layer input 2H x 2W, as upsample.1 has it) equals the un-shuffle of the plain output bit for bit, with
    dy strided and phase-separated.  The plain output at 2H x 2W is itself checked against the reference at six of the seven shapes;
    at (3,160,704) -- outside the listed shapes, its fp64 reference takes the CPU about a minute -- only the bit-equality is asserted
    (the plain form at (3,80,352) is test_ps_dgrad's).  A mask together with dx_planes has no kernel: the hook refuses it
    (test_hr_tail_host.py)."""
    dev = _gpu()
    n, h, w = shape
    big = (n, 2 * h, 2 * w)
    plain = T.run_hip(T.case("ps_dgrad", big), dev)
    if n * h * w <= 2000:
        T.check(T.case("ps_dgrad", big), plain)
    for dyp in (0, 1):
        assert T.same_bits(plain, T.run_hip(T.case("ps_dgrad", big, dy_planes=dyp, dx_planes=1), dev)), dyp


@dtypes
@shapes
def test_ps_wgrads(dtype, shape):
    """Ctx::ps_wgrads with dy strided and phase-separated: each against the reference, and the same bits."""
    dev = _gpu()
    a, b = (_run(c, dev) for c in T.ps_wgrads_cases(shape, dtype))
    assert T.same_bits(a, b)
