"""The propagation trunk's launches, one at a time, against the fp64 restatements of tests/trunk_common.py: every output element inside
the bound stated there (grid family: equal to the reference, or to its bf16 rounding), every input's padding pixels NaN, every output
between sentinel bands.  The launches go through the ``vsr_debug_trunk_*`` hooks (csrc/trunk_hooks.hip), i.e. through the Ctx members
and weight packs the engines use.

Shapes (N, H, W), tiles 8 rows x 32 pixels: the tail's list -- (1,1,1); (1,8,32) one whole tile; (2,13,37); (1,3,66); (1,9,31);
(1,17,100); (3,80,352) 330 tiles on 256 persistent workgroups: some take a second tile and their TileIter crosses an image boundary --
and (1,40,1000), 5 x 32 tiles (conv, chain and wgrad_cc only): a workgroup's stride wraps tile rows, the second tile buffer and the
weight-gradient rings are re-used.  Mid-channel 16 and 32 run every hook but the chain at the six small shapes.

Which case reaches which code (bf16 build at 64 channels; fp32 and the narrower widths run conv_mfma.hip's / wgrad_mfma.hip's generic
kernels on the same cases):
  conv3x3_persist.hip  <RELU>, <LEAKY> + sign_out     test_conv, test_sign_bits_three_sources
                       <NONE, res> (in place too), <NONE>, <NONE, MASK_RELU>, <NONE, res, MASK_LEAKY>, <NONE, MASK_LEAKY>    test_conv
                       <NONE, MASK_RELU_BITS>, <NONE, res, MASK_LEAKY_BITS>, sign_bits_c64_kernel    test_sign_bits_three_sources
  conv3x3_chain.hip    CHAIN_RELU + sout, CHAIN_SKIP, CHAIN_MASK reading those words    test_chain
  conv_mfma.hip        two sources, one planar (stem), 1x1 two sources / nz = 2 (fusion), planar destination + pres in place    test_stem, test_stem_dgrad, test_point
  wgrad_mfma.hip       wgrad3x3_c64_pc_kernel: 1 / 3 / 8 segments, accumulate, i_off / I_total; the 1x1 shape; planar X    test_wgrad_cc, test_stem_wgrads"""
import pytest
import torch

import hr_tail_common as T
import trunk_common as R

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp32")
FAMILIES = ("rand", "grid")
WIDTHS = [(s, 64) for s in R.SHAPES] + [(s, C) for C in (16, 32) for s in R.SMALL]
widths = pytest.mark.parametrize("shape,C", WIDTHS, ids=lambda v: T.sid(v) if isinstance(v, tuple) else f"c{v}")
widths_no_wide = pytest.mark.parametrize("shape,C", [v for v in WIDTHS if v[0] != R.WIDE], ids=lambda v: T.sid(v) if isinstance(v, tuple) else f"c{v}")


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _same(a, b, what):
    """Bit-identical outputs; on a mismatch, how many elements differ in value and how many only in the sign of a zero."""
    if R.same_bits(a, b):
        return
    rep = {k: (int((a[k] != b[k]).sum()), int(((a[k] == b[k]) & (torch.signbit(a[k]) != torch.signbit(b[k]))).sum())) for k in a if not k.startswith("_")}
    raise AssertionError((what, "output: (elements unequal in value, equal but for the sign of zero)", rep))


def _run_all(make, shape, C, dev):
    """Every case of `make` in both families and dtypes (the dtype innermost: the two builds share one cached reference)."""
    got = {}
    for fam in FAMILIES:
        for c0 in make(shape, "bf16", C, fam):
            for dt in DTYPES:
                c = R.Case(c0.hook, c0.shape, dt, c0.opts)
                got[c] = R.run_hip(c, dev)
                R.check(c, got[c])
    return got


@widths
def test_conv(shape, C):
    """Ctx::conv in the arms the engines run; the residual read in place gives the bits of the residual read from its own tensor."""
    got = _run_all(R.conv_cases, shape, C, _gpu())
    for c, v in got.items():
        if c.o("inplace"):
            other = R.Case(c.hook, c.shape, c.dtype, tuple(kv for kv in c.opts if kv[0] != "inplace"))
            if other in got:
                assert R.same_bits(v, got[other]), c.name


@pytest.mark.parametrize("shape", R.SHAPES, ids=T.sid)
def test_sign_bits_three_sources(shape):
    """bf16, 64 channels.  A forward launch (bias + ReLU; bias + LeakyReLU) writes its output and that output's sign bits.  The masked
    data gradient behind it -- ReLU': no residual; LeakyReLU': with the residual -- is then run with the mask from (1) those bits, (2)
    bits made by vsr_launch_sign_bits_c64 from the stored output, (3) aux = the stored output: bit-identical on every in-image element,
    and (3) inside the bound against fp64 with the mask from the stored output.  The same for (2) against (3) on a given activation
    with +-0 and +-2^-133 on the first and the last column."""
    dev = _gpu()
    for fam, act, extra in (("rand", 1, {}), ("grid", 1, {}), ("rand", 2, dict(res=1))):
        fwd = R.case("conv", shape, "bf16", C=64, family=fam, act=act, sign_out=1)
        out = R.run_hip(fwd, dev)
        R.check(fwd, out)
        given = dict(aux=out["y"])
        k = lambda src: R.case("conv", shape, "bf16", C=64, family=fam, mode=1, bias=False, mask=src, mask_mode=act, **extra)
        from_aux = R.run_hip(k("aux"), dev, given)
        R.check(k("aux"), from_aux, given=given)
        _same(from_aux, R.run_hip(k("bits"), dev, given, bits=out["_bits"]), (fwd.name, "bits written by the forward launch"))
        _same(from_aux, R.run_hip(k("made"), dev, given), (fwd.name, "bits made from the stored output"))
        if fam == "rand":
            _same(R.run_hip(k("aux"), dev), R.run_hip(k("made"), dev), (fwd.name, "a given activation"))


@widths_no_wide
def test_stem(shape, C):
    """Ctx::stem on cat([lr, feat]) (feat given and NULL), and on the planar frames alone with an image stride."""
    _run_all(R.stem_cases, shape, C, _gpu())


@widths_no_wide
def test_stem_dgrad(shape, C):
    """The stem's data gradients: towards feat, and towards the LR channels accumulating into the planar destination in place."""
    _run_all(R.stem_dgrad_cases, shape, C, _gpu())


@widths_no_wide
def test_point(shape, C):
    """The 1x1 fusion conv (two sources, LeakyReLU) and its two-destination data gradient."""
    _run_all(R.point_cases, shape, C, _gpu())


@widths
def test_wgrad_cc(shape, C):
    """Ctx::wgrad_cc, 3x3 and 1x1, over 1 / 3 / 8 segments, overwriting and accumulating into a pre-filled gradient, at i_off 0 and C of
    I_total = 2C (the other half bit-untouched); bit-identical on a repeat."""
    dev = _gpu()
    got = _run_all(R.wgrad_cc_cases, shape, C, dev)
    for c, v in got.items():
        if c.o("nseg") == 3 and c.o("family") == "grid":
            assert R.same_bits(v, R.run_hip(c, dev)), c.name


@widths_no_wide
def test_stem_wgrads(shape, C):
    """Ctx::stem_wgrads: planar X with an image stride, one feat segment fewer than LR segments, 1 / 2 / 3 / 8 frames."""
    _run_all(R.stem_wgrads_cases, shape, C, _gpu())


@pytest.mark.parametrize("shape", R.SHAPES, ids=T.sid)
def test_chain(shape):
    """vsr_launch_conv3x3_chain: a forward chain of 2 (and, small shapes, 3) residual blocks writing sign words, then the backward chain
    reading them, in one guarded allocation.  Every layer against fp64 on the images the GPU stored for its inputs, the mask from the
    stored activation (grid family: equal to the rounded reference).  The last block's masked gradient equals Ctx::conv's with aux =
    the stored activation bit for bit."""
    dev = _gpu()
    for c in R.chain_cases(shape):
        img = R.run_chain(c, dev)
        R.check_chain(c, img)
        nb = c.o("blocks")
        if nb == 2:
            t = R.inputs_of(c)
            one = R.case("conv", shape, "bf16", C=64, family=c.o("family", "rand"), mode=1, bias=False, mask="aux", mask_mode=1)
            y = R.run_hip(one, dev, dict(x=img[f"dx{nb}"], w=t["w"][2 * nb - 1], aux=img[f"a{nb - 1}"]))["y"]
            _same(dict(y=y), dict(y=img[f"da{nb - 1}"]), (c.name, "Ctx::conv with aux = the stored activation"))
