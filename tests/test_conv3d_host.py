"""CPU checks of the strided Conv3d and its modules: libvsrlab_conv3d.so's exports, struct layout and argument checks (every entry
refuses bad arguments before it touches the GPU), the constructors, state_dict keys and refusals of ConvST / ConvSTBlock /
PixelShufflePack3D / Upsample, and the restatement of tests/conv3d_common.py against the reference's recorded fp64 results
(tests/golden/conv3d.npz).  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import conv3d_common as CC
from helpers import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vsr_conv3d_workspace_bytes", "vsr_conv3d_fwd", "vsr_conv3d_bwd"}
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4


@pytest.fixture(scope="module")
def gold():
    return golden("conv3d")


def _gold_names(key):
    with np.load(os.path.join(GOLDEN, "conv3d.npz"), allow_pickle=False) as z:
        return [str(s) for s in z[key]]


def _gold_shapes(tag):
    return dict(zip(_gold_names(tag + "__keys"), (tuple(int(n) for n in s.split(",")) for s in _gold_names(tag + "__shapes"))))


def _module(name):
    from vsrlab_amd.core.modules.conv import ConvST, ConvSTBlock
    from vsrlab_amd.core.modules.upsampling import PixelShufflePack3D
    from vsrlab_amd.vsr.models.VRT.vrt import Upsample
    cls, args, _ = CC.MODULE_CASES[name]
    return {"ConvST": ConvST, "ConvSTBlock": ConvSTBlock, "PixelShufflePack3D": PixelShufflePack3D, "Upsample": Upsample}[cls](*args)


# ---- the library --------------------------------------------------------------------------------------------------------------------
def test_the_conv3d_library_loads_once_and_types_every_entry():
    from vsrlab_amd import _lib
    lib = _lib.load_conv3d()
    assert _lib.load_conv3d() is lib and lib is not _lib.load() and lib is not _lib.load_mixer()
    for name, (res, args) in _lib.CONV3D_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_library_exports_and_struct_layout():
    """the entry points live in a library of their own, which exports what its header declares and nothing else"""
    from vsrlab_amd import _lib
    lib = _lib.load_conv3d()
    assert set(_lib.CONV3D_EXPORTS) == NAMES and not NAMES & set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "vsrlab_conv3d.h")).read()
    assert set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert set(re.findall(r"^(?:int|size_t) (vsr_[a-z0-9_]+)\(", header, re.M)) == NAMES
    from test_hr_tail_host import _exported_vsr_symbols          # the dynamic symbol table, read from the ELF file
    assert _exported_vsr_symbols(_lib.CONV3D_LIB_PATH) == NAMES
    assert not any(hasattr(_lib.load(), n) for n in NAMES) and all(hasattr(lib, n) for n in NAMES)
    assert _lib.load().vsr_abi_version() == 4
    # the constants and the struct as the header lays them out
    const = {k: int(v) for k, v in re.findall(r"#define VSR_CONV3D_(\w+) (\d+)", header)}
    assert const == {"133": _lib.CONV3D_133, "311": _lib.CONV3D_311, "333": _lib.CONV3D_333, "ACT_NONE": _lib.CONV3D_ACT_NONE,
                     "ACT_LEAKY": _lib.CONV3D_ACT_LEAKY, "MAX_C": _lib.CONV3D_MAX_C} and const["MAX_C"] == 256
    body = re.search(r"typedef struct VsrConv3dDesc \{(.*?)\} VsrConv3dDesc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(n.strip().split("[")[0], ctype) for ctype, names in re.findall(r"(int|float|long long) ([^;]+);", body) for n in names.split(",")]
    want = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong * 3}
    assert [(n, want[t]) for n, t in fields] == list(_lib.Conv3dDesc._fields_)
    assert ctypes.sizeof(_lib.Conv3dDesc) == 96 and _lib.Conv3dDesc.slope.offset == 36 and _lib.Conv3dDesc.pixel_shuffle.offset == 40
    assert _lib.Conv3dDesc.x_stride.offset == 48 and _lib.Conv3dDesc.y_stride.offset == 72


def _desc(B=1, Cin=16, Cout=16, T=2, H=5, W=7, taps=0, dtype=0, act=0, slope=0.1, pixel_shuffle=0, xs=None, ys=None):
    from vsrlab_amd import _lib
    d = _lib.Conv3dDesc(B, Cin, Cout, T, H, W, taps, dtype, act, slope, pixel_shuffle)
    r = pixel_shuffle or 1
    cy = Cout // (r * r) if Cout > 0 else 1
    for i, v in enumerate(xs or (Cin * T * H * W, T * H * W, H * W)):
        d.x_stride[i] = v
    for i, v in enumerate(ys or (cy * T * H * W * r * r, T * H * W * r * r, H * W * r * r)):
        d.y_stride[i] = v
    return d


SHAPE_BADARG = (dict(B=0), dict(Cin=0), dict(Cout=-1), dict(T=0), dict(H=0), dict(W=-3), dict(dtype=2), dict(dtype=-1), dict(taps=3),
                dict(taps=-1), dict(act=2), dict(pixel_shuffle=1), dict(pixel_shuffle=4), dict(xs=(-1, 70, 35)), dict(ys=(560, -70, 35)))
SHAPE_UNSUPPORTED = (dict(Cin=257), dict(Cout=257), dict(Cout=18, pixel_shuffle=2), dict(act=1, slope=0.0), dict(act=1, slope=-0.1),
                     dict(B=2, xs=(1 << 62, 70, 35)), dict(B=3, ys=(1 << 62, 70, 35)), dict(B=1 << 20, T=1 << 20, H=1 << 12, W=1 << 12),
                     dict(B=1 << 16, T=1 << 15, H=8, W=32))                       # the last: 2^31 workgroups


def test_entries_reject_bad_arguments_before_touching_the_gpu():
    from vsrlab_amd import _lib
    lib = _lib.load_conv3d()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)
    big = 1 << 40

    def fwd(x=one, w=one, b=one, y=one, ws=one, nbytes=big, null_desc=False, **kw):
        return lib.vsr_conv3d_fwd(None if null_desc else ctypes.byref(_desc(**kw)), x, w, b, y, ws, nbytes, None)

    def bwd(x=one, w=one, y=one, dy=one, dx=one, dw=one, db=one, ws=one, nbytes=big, null_desc=False, **kw):
        return lib.vsr_conv3d_bwd(None if null_desc else ctypes.byref(_desc(**kw)), x, w, y, dy, dx, dw, db, ws, nbytes, None)

    for bad in (dict(null_desc=True), dict(x=None), dict(w=None), dict(y=None), dict(ws=None), dict(x=odd), dict(w=odd), dict(b=odd),
                dict(y=ctypes.c_void_p(257), dtype=1), dict(ws=ctypes.c_void_p(128))) + SHAPE_BADARG:
        assert fwd(**bad) == BADARG, bad
    for bad in (dict(null_desc=True), dict(x=None), dict(w=None), dict(dy=None), dict(ws=None), dict(y=None, act=1), dict(dy=odd), dict(dx=odd),
                dict(dw=odd), dict(db=odd), dict(x=ctypes.c_void_p(257), dtype=1), dict(ws=ctypes.c_void_p(128))) + SHAPE_BADARG:
        assert bwd(**bad) == BADARG, bad
    for bad in SHAPE_UNSUPPORTED:
        assert fwd(**bad) == UNSUPPORTED and bwd(**bad) == UNSUPPORTED, bad
    for bad in SHAPE_BADARG + SHAPE_UNSUPPORTED:
        for need_backward in (0, 1):
            assert lib.vsr_conv3d_workspace_bytes(ctypes.byref(_desc(**bad)), need_backward) == 0, bad
    assert lib.vsr_conv3d_workspace_bytes(None, 0) == 0 and lib.vsr_conv3d_workspace_bytes(None, 1) == 0
    for kw in (dict(), dict(dtype=1), dict(taps=2, Cin=3), dict(Cout=256, act=1, pixel_shuffle=2)):
        nf, nb = (lib.vsr_conv3d_workspace_bytes(ctypes.byref(_desc(**kw)), k) for k in (0, 1))
        assert nf > 0 and nb > nf and nf % 256 == 0 and nb % 256 == 0
        assert fwd(nbytes=nf - 1, **kw) == WORKSPACE and bwd(nbytes=nb - 1, **kw) == WORKSPACE, kw


def test_the_workspace_holds_what_the_header_says():
    """the packed weight, padded to 64 rows x 16 reduction channels per tap, in bf16 as a hi and a lo part; the backward adds dz only
    with an epilogue to undo"""
    from vsrlab_amd import _lib
    lib = _lib.load_conv3d()
    n = lambda need, **kw: lib.vsr_conv3d_workspace_bytes(ctypes.byref(_desc(**kw)), need)   # noqa: E731
    assert n(0, Cin=27, Cout=80, taps=0) == 2 * 2 * 9 * 2 * 64 * 8 * 4                         # 80 -> 2 blocks of 64, 27 -> 2 chunks of 16
    assert n(0, Cin=27, Cout=80, taps=0, dtype=1) == 2 * 2 * 9 * 2 * 2 * 64 * 8 * 2
    assert n(0, Cin=3, Cout=16, taps=2) == 27 * 2 * 64 * 8 * 4 and n(0, Cin=64, Cout=64, taps=1) == 4 * 3 * 2 * 64 * 8 * 4
    plain, act = n(1, Cin=64, Cout=64, dtype=1), n(1, Cin=64, Cout=64, dtype=1, act=1)
    assert act - plain == -(-(2 * 5 * 7 * 64 * 2) // 256) * 256


# ---- the modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.MODULE_CASES))
def test_modules_follow_the_reference(name):
    import torch.nn as nn
    model = _module(name)
    want = _gold_shapes("module_" + name)
    assert list(model.state_dict()) == list(want) == list(CC.module_shapes(name))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want == CC.module_shapes(name)
    model.load_state_dict(CC.module_params(name), strict=True)
    assert all(p.requires_grad and p.dtype == torch.float32 for p in model.parameters())
    holders = [m for m in model.modules() if any(True for _ in m.parameters(recurse=False))]
    assert holders and all(isinstance(m, nn.Conv3d) for m in holders)               # initialisation and checkpoints are the reference's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(CC.module_inputs(name)[0])


def test_module_constructors_and_children():
    import torch.nn as nn
    from vsrlab_amd.core.modules.conv import ConvST, ConvSTBlock
    from vsrlab_amd.core.modules.upsampling import PixelShufflePack3D
    from vsrlab_amd.vsr.models.VRT.vrt import Upsample
    st = ConvST(16, 32)
    assert st.conv_xy.kernel_size == (1, 3, 3) and st.conv_xy.padding == (0, 1, 1) and st.conv_xy.bias is None
    assert st.conv_t.kernel_size == (3, 1, 1) and st.conv_t.padding == (1, 0, 0) and st.conv_t.bias is None
    assert ConvSTBlock(2, 3, 16).conv_in.kernel_size == (3, 3, 3) and len(ConvSTBlock(2, 3, 16).block) == 2
    assert isinstance(PixelShufflePack3D(16, 16, 2).pixel_shuffle, nn.PixelShuffle)
    up = Upsample(4, 64)
    assert isinstance(up, nn.Sequential) and len(up) == 11
    assert [type(m).__name__ for m in up][:5] == ["Conv3d", "_Transpose_Dim12", "PixelShuffle", "_Transpose_Dim12", "LeakyReLU"]
    assert up[4].negative_slope == 0.1 and up[5].out_channels == 256 and up[10].out_channels == 64 and len(Upsample(1, 64)) == 1
    x = torch.zeros(2, 3, 4)
    assert up[1](x).shape == (2, 4, 3)


def test_what_the_kernels_do_not_cover_raises_at_construction():
    from vsrlab_amd.core.modules.conv import ConvST
    from vsrlab_amd.core.modules.upsampling import PixelShufflePack3D
    from vsrlab_amd.vsr.models.VRT.vrt import Upsample
    for kw in (dict(kernel_size=(5, 3, 3)), dict(kernel_size=(3, 5, 5)), dict(kernel_size=(3, 3, 2)), dict(stride=(1, 2, 2)), dict(stride=(2, 1, 1)),
               dict(padding=(0, 1, 1)), dict(padding=(1, 0, 0)), dict(padding=(1, 2, 2))):
        with pytest.raises(NotImplementedError, match="ConvST"):
            ConvST(16, 16, **kw)
    for upscale in (1, 3, 4):
        with pytest.raises(NotImplementedError, match="upscale 2"):
            PixelShufflePack3D(16, 16, upscale)
    with pytest.raises(AssertionError, match="power of 2"):
        Upsample(3, 64)


def test_conv3d_checks_its_arguments():
    from vsrlab_amd.core.conv3d_ops import conv3d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv3d(torch.zeros(1, 3, 2, 4, 4), torch.zeros(8, 3, 1, 3, 3))


def test_the_compat_mapping_resolves_the_new_modules():
    import importlib

    import vsrlab_amd
    vsrlab_amd.install_as_vsrlab(force=True)
    from vsrlab_amd.core.modules import conv, upsampling
    from vsrlab_amd.vsr.models.VRT import vrt
    assert importlib.import_module("vsrlab.core.modules.conv").ConvST is conv.ConvST
    assert importlib.import_module("vsrlab.core.modules.conv").ConvSTBlock is conv.ConvSTBlock
    assert importlib.import_module("vsrlab.core.modules.upsampling").PixelShufflePack3D is upsampling.PixelShufflePack3D
    assert importlib.import_module("vsrlab.vsr.models.VRT.vrt").Upsample is vrt.Upsample


# ---- the restatement against the reference's record --------------------------------------------------------------------------------------
def test_the_golden_is_small_and_fp64(gold):
    assert os.path.getsize(os.path.join(GOLDEN, "conv3d.npz")) < 128 * 1024
    assert all(v.dtype == torch.float64 for v in gold.values())


@pytest.mark.parametrize("i", range(len(CC.OP_CASES)))
def test_the_restated_layer_reproduces_the_reference(gold, i):
    got = CC.run_op_case(i, torch.float64)
    assert set(got) == {"out", "dx", "dw"} | ({"db"} if CC.OP_CASES[i].get("bias") else set())
    assert tuple(got["out"].shape) == CC.op_shapes(CC.OP_CASES[i])[1]
    for k, v in got.items():
        assert CC.golden_mismatch(gold, f"op{i}__{k}", v) <= 1e-12, (i, k)
    if i == 0:          # one frame: the outer temporal taps see only padding
        assert not got["dw"][:, :, 0].any() and not got["dw"][:, :, 2].any() and bool(got["dw"][:, :, 1].abs().min() > 0)


@pytest.mark.parametrize("name", list(CC.MODULE_CASES))
def test_the_restated_modules_reproduce_the_reference(gold, name):
    out, dx, grads = CC.run_module_case(name, torch.float64)
    assert CC.golden_mismatch(gold, f"{name}__out", out) <= 1e-12
    assert CC.golden_mismatch(gold, f"{name}__dx", dx) <= 1e-12
    assert list(grads) == list(CC.module_shapes(name))
    for k, g in grads.items():
        assert CC.golden_mismatch(gold, f"{name}__grad__{k}", g) <= 1e-12, k


def test_bf16_emulation_rounds_at_the_launch_boundaries_only():
    x, w, b, _ = CC.op_inputs(1)
    x = x.requires_grad_(True)
    y = CC.conv3d(x, w, b, time_major=True, store=CC.bf16_store)
    assert torch.equal(y, CC.bf16_store(y)) and not torch.equal(y, CC.conv3d(x, w, b, time_major=True))
    y.sum().backward()
    assert torch.equal(x.grad, CC.bf16_store(x.grad))


def test_documents_say_what_is_provided():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert all(n in readme for n in ("ConvST", "ConvSTBlock", "PixelShufflePack3D", "Upsample"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "11k" in design and "conv3d.hip" in design
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "libvsrlab_conv3d.so" in integration and "vsrlab_conv3d.h" in integration
    profiles = open(os.path.join(ROOT, "profiles", "README.md")).read()
    assert "conv3d_bench.json" in profiles and "conv3d_isa.md" in profiles
