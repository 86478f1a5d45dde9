"""GPU checks of the fused JPEG round trip (csrc/jpeg_degrade.hip) behind ``functional.jpeg_compress`` and
``core.augmentations.RandomJPEGCompression``, against the integer oracle of tests/jpeg_common.py (pinned to the reference and to
libjpeg by tests/test_jpeg_host.py).  Every comparison is ``torch.equal``: the specification is integer arithmetic, so there is
no tolerance and no share of exempt pixels.  The cases and what each catches: ``jpeg_common.CASES``."""
import ctypes

import pytest
import torch

import jpeg_common as J
from attention_common import GUARD, SENTINEL, _guarded

pytestmark = pytest.mark.gpu

PAIRS = [(name, q) for name, (_, qs) in J.CASES.items() for q in qs]


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want():
    """per (case, quality): the oracle's bytes as fp32 (N, 3, H, W), computed once and left unchanged"""
    u8 = {name: J.to_u8(J.case_input(name)) for name in J.CASES}
    return {(name, q): torch.from_numpy(J.oracle(u8[name], q)).to(torch.float32) for name, q in PAIRS}


def _hip(x, q):
    from vsrlab_amd import functional as VF
    out = VF.jpeg_compress(x, q)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,q", PAIRS)
def test_equals_the_oracle_bit_for_bit(name, q, want):
    x = J.case_input(name).to(_dev())
    keep = x.clone()
    out = _hip(x, q)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous() and not out.requires_grad
    assert torch.equal(x, keep), "the input was modified"
    got = (out * 255).cpu()
    bad = int((got != want[name, q]).sum())
    print(f"{name} q={q}: {bad} of {got.numel()} values differ from the oracle")
    assert torch.equal(got, want[name, q])
    assert torch.equal(out.cpu(), want[name, q] / 255)


@pytest.mark.parametrize("shape", [(1, 3, 2, 3), (1, 3, 6, 5), (1, 3, 14, 4), (2, 3, 18, 66), (1, 3, 34, 7)])
def test_edge_sizes(shape):
    """even heights with one to seven chroma rows below the image, in the first tile row and in the second; chroma planes 2 and 3
    columns wide (replication against the triangle filter); a width one chroma sample into a second 64-pixel tile"""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g)
    assert torch.equal(_hip(x.to(_dev()), 30).cpu(), J.expected(x, 30))


def test_three_dimensional_input(want):
    x = J.case_input("odd").to(_dev())
    out = _hip(x[0], 49)
    assert out.shape == x.shape[1:] and torch.equal((out * 255).cpu(), want["odd", 49][0])


@pytest.mark.parametrize("name,q", [("halo", 10), ("odd", 95), ("even_30", 10), ("pixel", 1)])
def test_bf16_in_and_out(name, q):
    """the product x * 255 is rounded to bf16 before it is truncated, and the result k / 255 is rounded to bf16"""
    x = J.case_input(name, torch.bfloat16)
    out = _hip(x.to(_dev()), q)
    assert out.dtype == torch.bfloat16
    assert torch.equal(out.cpu(), J.expected(x, q))


def test_non_contiguous_inputs(want):
    x = J.case_input("halo").to(_dev())
    cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)              # a channels-last view
    assert not cl.is_contiguous()
    assert torch.equal((_hip(cl, 75) * 255).cpu(), want["halo", 75])
    big = torch.full((3, 5, 50, 83), 0.5, device=_dev())
    big[0:2, 1:4, 1:49, 2:82] = x
    view = big[0:2, 1:4, 1:49, 2:82]                                        # a sliced view: every stride differs from the dense one
    assert not view.is_contiguous()
    assert torch.equal((_hip(view, 75) * 255).cpu(), want["halo", 75])


def test_inputs_outside_the_unit_interval_are_clamped():
    g = torch.Generator().manual_seed(7)
    x = torch.rand(1, 3, 37, 53, generator=g) * 3 - 1                       # a third below 0, a third above 1
    out = _hip(x.to(_dev()), 75)
    assert torch.equal(out.cpu(), J.expected(x, 75))
    assert torch.equal(out.cpu(), J.expected(x.clamp(0, 1), 75))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,q", [("one_mb", 50), ("odd", 49), ("plus_one", 1), ("even_30", 95), ("pixel", 100), ("two_wide", 50)])
def test_guard_bands_through_the_c_abi(name, q, dt):
    """output and workspace lie in sentinel guard bands: a write outside either is caught"""
    from vsrlab_amd import _lib
    lib = _lib.load_jpeg()
    dev = _dev()
    x = J.case_input(name, dt)
    xd = x.to(dev)
    n, _, h, w = x.shape
    code = _lib.DT_BF16 if dt == torch.bfloat16 else _lib.DT_F32
    out_buf, out = _guarded(tuple(x.shape), dt, dev, SENTINEL)
    L4 = ctypes.c_longlong * 4
    desc = _lib.JpegDesc(n, h, w, q, code, code, L4(*xd.stride()), L4(*out.stride()))
    nbytes = int(lib.vsr_jpeg_workspace_bytes(desc))
    hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
    assert n * hp * wp * 3 // 2 <= nbytes <= n * hp * wp * 3 // 2 + 3 * 256, "the workspace is the byte planes: 1.5 bytes per padded pixel"
    ws_buf, ws = _guarded((nbytes,), torch.uint8, dev, 0x5a)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.vsr_jpeg_fwd(desc, ptr(xd), ptr(out), ptr(ws), nbytes, st) == 0
    torch.cuda.synchronize()
    for what, buf, fill in (("output", out_buf, SENTINEL), ("workspace", ws_buf, 0x5a)):
        for band in (buf[:GUARD], buf[-GUARD:]):
            assert bool((band == fill).all()), f"{name} {dt}: the guard band of the {what} was written"
    assert torch.equal(out.cpu(), J.expected(x, q))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_two_runs_are_identical(dt):
    x = J.case_input("batch", dt).to(_dev())
    assert torch.equal(_hip(x, 50), _hip(x, 50))


def test_module_equals_function(want):
    from vsrlab_amd.core.augmentations import RandomJPEGCompression
    x = J.case_input("halo").to(_dev())
    for m in (RandomJPEGCompression([75]), RandomJPEGCompression(75), RandomJPEGCompression([75, 75])):
        assert m.q == 75
        out = m(x.clone().requires_grad_(True))
        assert not out.requires_grad and out.dtype == x.dtype
        assert torch.equal(out, _hip(x, 75)) and torch.equal((out * 255).cpu(), want["halo", 75])
    out = RandomJPEGCompression(10)(x[1])
    assert out.shape == x.shape[1:] and torch.equal((out * 255).cpu(), want["halo", 10][1])


def test_a_cpu_tensor_is_refused():
    from vsrlab_amd import functional as VF
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.jpeg_compress(torch.zeros(1, 3, 16, 16), 50)
