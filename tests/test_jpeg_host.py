"""CPU checks of the JPEG round trip (core/augmentations.py, functional.jpeg_compress): the integer oracle of
tests/jpeg_common.py against the reference's recorded results and against a live PIL, its int32 safety, the quantiser's
reciprocal, the tables, and the package's constructor semantics, library exports and documentation.  Nothing here needs a GPU."""
import importlib
import os
import random
import re

import numpy as np
import pytest
import torch

import jpeg_common as J
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return golden("jpeg")


@pytest.mark.parametrize("name", list(J.CASES))
def test_oracle_equals_the_reference_exactly(name, gold):
    x = gold[f"{name}__x"]
    assert torch.equal(x, J.case_input(name)), "the keyed input is not the stored one"
    u8 = J.to_u8(x)
    for q in J.CASES[name][1]:
        assert np.array_equal(J.oracle(u8, q), gold[f"{name}__q{q}"].numpy()), (name, q)
        assert torch.equal(J.expected(x, q) * 255, gold[f"{name}__q{q}"].to(torch.float32)), (name, q)


def test_the_golden_covers_the_case_table(gold):
    want = {f"{n}__x" for n in J.CASES} | {f"{n}__q{q}" for n in J.CASES for q in J.CASES[n][1]}
    assert set(gold) == want
    assert set(J.CASES["one_mb"][1]) == set(J.QUALITIES) and all(len(v[1]) == 2 for k, v in J.CASES.items() if k != "one_mb")


@pytest.mark.skipif(not J.pil_has_jpeg(), reason="Pillow without JPEG support")
@pytest.mark.parametrize("name", list(J.CASES))
def test_oracle_equals_a_live_pil(name):
    x = J.case_input(name)
    for q in J.CASES[name][1]:
        assert torch.equal(J.expected(x, q), J.reference_path(x, q)), (name, q)


@pytest.mark.skipif(not J.pil_has_jpeg(), reason="Pillow without JPEG support")
def test_oracle_equals_a_live_pil_at_the_edge_rules():
    """the two rules that only edge sizes show: every H in 1..18 (even heights pad the chroma plane, not the pixels) by widths on both
    sides of the narrow-plane threshold (chroma 2 and 3 columns wide) and of a macroblock"""
    g = torch.Generator().manual_seed(11)
    for h in range(1, 19):
        for w in (1, 3, 4, 5, 17):
            x = torch.rand(1, 3, h, w, generator=g)
            q = (5, 30, 60, 90)[(h + w) % 4]
            assert torch.equal(J.expected(x, q), J.reference_path(x, q)), (h, w, q)


def _saturated(kind):
    if kind == "checker1":
        yy, xx = np.mgrid[0:32, 0:48]
        return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8), (1, 3, 32, 48)).copy()
    if kind == "checker8":
        yy, xx = np.mgrid[0:32, 0:48]
        a = ((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)
        return np.stack([a, 255 - a, a])[None]
    rng = np.random.default_rng(3)
    return (rng.integers(0, 2, size=(2, 3, 33, 47)) * 255).astype(np.uint8)


@pytest.mark.parametrize("kind", ["checker1", "checker8", "noise"])
def test_int32_is_enough(kind):
    """the same steps in wrapping int32 give the int64 result on the inputs with the largest intermediates"""
    u8 = _saturated(kind)
    for q in (1, 50, 100):
        assert np.array_equal(J.oracle(u8, q, itype=np.int32), J.oracle(u8, q)), (kind, q)


def test_the_quantisers_reciprocal_is_the_division():
    """csrc/jpeg_degrade.hip divides n = |c| + 4 Q by 8 Q as umulhi(n, floor(2^32 / (8 Q)) + 1): equal to the integer division for
    every Q in 1..255 and every n below 2^16 + 1020, which bounds what the oracle's quantiser sees (|c| < 2^16 is checked on the
    saturated inputs, whose coefficients are the largest an 8-bit image has)"""
    seen = [0]
    for kind in ("checker1", "checker8", "noise"):
        J.oracle(_saturated(kind), 50, max_abs=seen)
    flat = np.zeros((1, 3, 16, 16), np.uint8)
    J.oracle(flat, 50, max_abs=seen)                                       # the DC extreme: 64 samples of -128
    assert 8192 <= seen[0] < 1 << 16, seen
    n = np.arange((1 << 16) + 1020 + 1, dtype=np.uint64)
    for Q in range(1, 256):
        d = 8 * Q
        m = (1 << 32) // d + 1
        assert m < 1 << 32
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(d)), Q
    src = open(os.path.join(ROOT, "vsrlab_amd", "csrc", "jpeg_degrade.hip")).read()
    assert "(1ull << 32) / (unsigned)(8 * v)) + 1u" in src and "__umulhi((unsigned)(m + 4 * q)" in src, "the kernel's form changed: restate it here"


def test_quantisation_tables():
    l1, c1 = J.quant_tables(1)
    assert l1[0, 0] == 255 and (l1 == 255).all() and (c1 == 255).all()          # s = 5000: everything clamps to 255
    l50, c50 = J.quant_tables(50)
    assert np.array_equal(l50, J.LUMA_BASE) and np.array_equal(c50, J.CHROMA_BASE)
    l100, c100 = J.quant_tables(100)
    assert (l100 == 1).all() and (c100 == 1).all()                               # s = 0: everything clamps to 1
    l49, _ = J.quant_tables(49)
    assert l49[0, 0] == (16 * 102 + 50) // 100 and J.quant_tables(75)[0][0, 1] == (11 * 50 + 50) // 100
    for a, b in ((0, 1), (-5, 1), (101, 100), (1000, 100)):
        assert all(np.array_equal(x, y) for x, y in zip(J.quant_tables(a), J.quant_tables(b)))
    if J.pil_has_jpeg():
        import io
        from PIL import Image
        for q in (1, 50, 100):
            buf = io.BytesIO()
            Image.new("RGB", (16, 16)).save(buf, format="JPEG", quality=q)
            buf.seek(0)
            tabs = Image.open(buf).quantization
            for got, want in zip((tabs[0], tabs[1]), J.quant_tables(q)):            # as a multiset: the order PIL reports depends on its version
                assert sorted(got) == sorted(want.flatten().tolist()), q


def test_constructor_semantics():
    from vsrlab_amd.core.augmentations import RandomJPEGCompression
    random.seed(1234)
    want = [random.randint(20, 90) for _ in range(5)]
    random.seed(1234)
    assert [RandomJPEGCompression([20, 90]).q for _ in range(5)] == want        # one randint per construction
    m = RandomJPEGCompression((30, 95))
    assert all(m.q == q for q in [m.q] * 3)                                      # drawn once, not per call
    state = random.getstate()
    assert RandomJPEGCompression([42]).q == 42 and RandomJPEGCompression(42).q == 42
    assert random.getstate() == state                                           # a fixed quality draws nothing
    with pytest.raises(ValueError):
        RandomJPEGCompression([1, 2, 3])
    with pytest.raises(ValueError):
        RandomJPEGCompression([])
    assert len(list(RandomJPEGCompression(50).parameters())) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RandomJPEGCompression(50)(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError):
        RandomJPEGCompression(50)(torch.zeros(16, 16))


def test_functional_validation():
    from vsrlab_amd import functional as VF
    for bad in (torch.zeros(16, 16), torch.zeros(1, 4, 16, 16), torch.zeros(2, 1, 3, 16, 16), torch.zeros(0, 3, 16, 16)):
        with pytest.raises(ValueError):
            VF.jpeg_compress(bad, 50)
    with pytest.raises(ValueError):
        VF.jpeg_compress(torch.zeros(1, 3, 16, 16, dtype=torch.float16), 50)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.jpeg_compress(torch.zeros(3, 16, 16), 50)


def test_mirroring():
    from vsrlab_amd.core.augmentations import Mirroring
    x = torch.arange(4 * 3 * 2 * 2, dtype=torch.float32).reshape(4, 3, 2, 2)
    out = Mirroring.forward(x)                                                   # static, as in the reference
    assert out.shape == (8, 3, 2, 2) and torch.equal(out[:4], x) and torch.equal(out[4:], x.flip(0))
    assert torch.equal(Mirroring()(x), out) and torch.equal(out, out.flip(0))


def test_random_video_compression_is_absent_and_documented():
    aug = importlib.import_module("vsrlab_amd.core.augmentations")
    assert not hasattr(aug, "RandomVideoCompression")
    assert "RandomVideoCompression" in aug.__doc__ and "H.264" in aug.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "RandomVideoCompression" in readme and "RandomJPEGCompression" in readme
    from vsrlab_amd.compat import install_as_vsrlab
    install_as_vsrlab(force=True)
    assert importlib.import_module("vsrlab.core.augmentations") is aug


def test_library_exports_and_workspace():
    """the entry points live in a library of their own, which exports them and nothing else"""
    import ctypes
    from vsrlab_amd import _lib
    lib = _lib.load_jpeg()
    names = {"vsr_jpeg_workspace_bytes", "vsr_jpeg_fwd"}
    assert set(_lib.JPEG_EXPORTS) == names and not names & set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "vsrlab_jpeg.h")).read()
    assert set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header)) == names
    from test_hr_tail_host import _exported_vsr_symbols          # the dynamic symbol table, read from the ELF file
    assert _exported_vsr_symbols(_lib.JPEG_LIB_PATH) == names
    assert not any(hasattr(_lib.load(), n) for n in names)
    L4 = ctypes.c_longlong * 4
    mk = lambda n, h, w, xd=0, yd=0: _lib.JpegDesc(n, h, w, 75, xd, yd, L4(3 * h * w, h * w, w, 1), L4(3 * h * w, h * w, w, 1))
    # the byte planes and nothing else: 1.5 bytes per padded pixel, each plane rounded up to 256 bytes
    for n, h, w in [(1, 16, 16), (2, 48, 80), (1, 37, 53), (14, 540, 960), (1, 1, 1), (3, 32768, 32768)]:
        px = n * (-(-h // 16) * 16) * (-(-w // 16) * 16)
        assert px * 3 // 2 <= lib.vsr_jpeg_workspace_bytes(mk(n, h, w)) <= px * 3 // 2 + 3 * 256
    assert lib.vsr_jpeg_workspace_bytes(mk(1, 16, 16, 1, 1)) == lib.vsr_jpeg_workspace_bytes(mk(1, 16, 16))   # the dtypes do not matter
    for bad in (mk(0, 16, 16), mk(1, 0, 16), mk(1, 16, 32769), mk(65536, 16, 16), mk(1, 16, 16, 2, 0), mk(1, 16, 16, 0, 7)):
        assert lib.vsr_jpeg_workspace_bytes(bad) == 0
    assert lib.vsr_jpeg_fwd(mk(1, 16, 32769), None, None, None, 0, None) == -2          # refused before any pointer is looked at
    assert lib.vsr_jpeg_fwd(mk(0, 16, 16), None, None, None, 0, None) == -1
    assert lib.vsr_jpeg_fwd(mk(1, 16, 16), None, None, None, 0, None) == -1             # null pointers
