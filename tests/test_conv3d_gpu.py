"""GPU checks of the strided Conv3d (csrc/conv3d.hip) -- through the C ABI of include/vsrlab_conv3d.h at the shapes of
tests/conv3d_common.py, and through ConvST / ConvSTBlock / PixelShufflePack3D / Upsample -- against the fp64 results of the
reference: the restatement of tests/conv3d_common.py in fp64, which tests/test_conv3d_host.py pins to the reference's record
(tests/golden/conv3d.npz) to 1e-12.

The criterion is tests/test_mixer_gpu.py's: relative L2 against the fp64 result; the HIP result's error may not exceed 1.5 x the error
of a CPU evaluation at the same precision against the same fp64 result -- the restatement in fp32, or in fp32 with bf16 storage
emulated at every launch boundary.  Floors: fp32 sqrt(K) 2^-24, bf16 2^-9, with K = Cin x taps, or the positions summed over for a
weight or bias gradient (a module case, a chain of launches: the longest such sum of the chain, see _module_K).  A gradient that is identically zero in fp64 must be exactly zero.  Every figure is printed before it is
asserted.  Every written operand and the workspace lie between guard bands, which a launch must leave as they were, and every
element of a written operand is written; a repeat gives the same bits."""
import ctypes
import math

import pytest
import torch

import conv3d_common as CC
from test_mixer_gpu import _floor, _judge

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
GUARD = 512                                             # bytes on either side
_refs = {}


def _cpu(kind, key, tag):
    """fp64 result, and the CPU evaluation at the precision `tag`, of a case: computed once and shared, never modified"""
    if (kind, key, tag) not in _refs:
        dtype, store = {"fp64": (torch.float64, None), "fp32": (torch.float32, None), "bf16": (torch.float32, CC.bf16_store)}[tag]
        if kind == "op":
            _refs[kind, key, tag] = CC.run_op_case(key, dtype, store)
        else:
            out, dx, grads = CC.run_module_case(key, dtype, store)
            _refs[kind, key, tag] = {"out": out, "dx": dx, **{"grad " + k: g for k, g in grads.items()}}
    return _refs[kind, key, tag]


class Guarded:
    """`nbytes` of device memory between two guard bands of a byte pattern"""

    def __init__(self, nbytes, fill):
        self.n = nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.before = self.raw.clone()

    def inner(self, dtype, shape):
        return self.raw[GUARD:GUARD + self.n].view(dtype).view(shape)

    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + GUARD)

    def check(self, what):
        assert torch.equal(self.raw[:GUARD], self.before[:GUARD]) and torch.equal(self.raw[GUARD + self.n:], self.before[GUARD + self.n:]), \
            f"{what}: a guard band was written"


def _operand(shape_mem, dtype):
    """an operand of all-ones bits (a NaN in fp32 and in bf16) between guard bands: (guard, the dense tensor in its memory order)"""
    g = Guarded(math.prod(shape_mem) * dtype.itemsize, 0xFF)
    return g, g.inner(dtype, shape_mem)


def _run_abi(i, tag):
    """case i through the C ABI: forward, then the full backward under the case's cotangent; everything checked for guard bands and
    unwritten elements"""
    from vsrlab_amd import _lib
    lib = _lib.load_conv3d()
    case, dtype = CC.OP_CASES[i], DTYPES[tag]
    x, w, b, cot = CC.op_inputs(i)
    tm = case["order"] == "t"
    # memory order: the case's own, or (view) the other one, of which the logical tensor is then a transposed view
    mem_tm = tm != bool(case.get("view"))
    to_mem = (lambda v: v.transpose(1, 2).contiguous()) if mem_tm != tm else (lambda v: v.contiguous())
    bct = (lambda v: v.transpose(1, 2)) if mem_tm else (lambda v: v)                      # memory tensor -> its (b,c,t,h,w) view
    xm, cm = to_mem(x).to(DEV).to(dtype), to_mem(cot).to(DEV).to(dtype)
    wd, bd = w.to(DEV), None if b is None else b.to(DEV)
    gy, ym = _operand(tuple(cm.shape), dtype)
    gdx, dxm = _operand(tuple(xm.shape), dtype)
    gdw, dw = _operand(tuple(w.shape), torch.float32)
    gdb, db = _operand((case["Cout"],), torch.float32)
    xv, yv = bct(xm), bct(ym)
    desc = _lib.Conv3dDesc(case["B"], case["Cin"], case["Cout"], case["T"], case["H"], case["W"], list(CC.TAPS).index(case["taps"]),
                           0 if tag == "fp32" else 1, 0 if case.get("slope") is None else 1, case.get("slope") or 0.0, case.get("shuffle", 0))
    for k in range(3):
        desc.x_stride[k], desc.y_stride[k] = xv.stride(k), yv.stride(k)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())                       # noqa: E731
    nf, nb = (lib.vsr_conv3d_workspace_bytes(ctypes.byref(desc), k) for k in (0, 1))
    assert nf > 0 and nb > 0
    wf, wb = Guarded(nf, 0xA5), Guarded(nb, 0xA5)
    assert wf.ptr().value % 256 == 0 and wb.ptr().value % 256 == 0
    assert lib.vsr_conv3d_fwd(ctypes.byref(desc), p(xm), p(wd), p(bd), gy.ptr(), wf.ptr(), nf, stream) == 0
    assert lib.vsr_conv3d_bwd(ctypes.byref(desc), p(xm), p(wd), gy.ptr(), p(cm), gdx.ptr(), gdw.ptr(), gdb.ptr() if b is not None else None,
                              wb.ptr(), nb, stream) == 0
    torch.cuda.synchronize()
    for g, name in ((gy, "y"), (gdx, "dx"), (gdw, "dw"), (gdb, "db"), (wf, "forward workspace"), (wb, "backward workspace")):
        g.check(f"op{i} {tag} {name}")
    back = (lambda v: v.transpose(1, 2)) if mem_tm != tm else (lambda v: v)                # memory order -> the case's logical order
    got = {"out": back(ym).clone(), "dx": back(dxm).clone(), "dw": dw.clone()}
    if b is not None:
        got["db"] = db.clone()
    else:
        assert bool(torch.isnan(db).all())                                                # a null db is skipped
    for k, v in got.items():
        assert not torch.isnan(v).any(), f"op{i} {tag} {k}: an element was not written"
    return got


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("i", range(len(CC.OP_CASES)))
def test_the_layer_matches_the_reference_through_the_c_abi(i, tag):
    case = CC.OP_CASES[i]
    got = _run_abi(i, tag)
    ref, cpu = _cpu("op", i, "fp64"), _cpu("op", i, tag)
    assert set(got) == set(ref)
    K = case["Cin"] * math.prod(CC.TAPS[case["taps"]])
    positions = case["B"] * case["T"] * case["H"] * case["W"]
    for k in got:
        _judge(f"op{i} {case['name']} {tag} {k}", got[k], ref[k], cpu[k], _floor(tag, positions if k in ("dw", "db") else K))
    again = _run_abi(i, tag)                            # no atomics: the same bits from run to run
    for k in got:
        assert torch.equal(got[k], again[k]), k


def _run_module(name, tag):
    from test_conv3d_host import _module
    model = _module(name)
    model.load_state_dict(CC.module_params(name), strict=True)
    model = model.to(DEV)
    x, cot = (v.to(DEV).to(DTYPES[tag]) for v in CC.module_inputs(name))
    x.requires_grad_(True)
    out = model(x)
    assert out.dtype == x.dtype and out.shape == cot.shape and out.is_contiguous()       # x's axis order and memory order
    (out * cot).sum().backward()
    assert all(p.grad.dtype == torch.float32 for p in model.parameters())
    return {"out": out.detach(), "dx": x.grad, **{"grad " + k: p.grad for k, p in model.named_parameters()}}


def _module_K(name):
    """One K per module case, as tests/test_mixer_gpu.py's _mixer_K takes it: the longest sum anywhere in the case -- the longest dot
    product of its layers (Cin x taps) or the most positions a parameter gradient sums over (the module's largest map).  A module is
    a chain of launches: every tensor but the first output carries the rounding of the launches before it, forward and backward, so
    a parameter gradient's error is not bounded by its own sum alone."""
    shapes = CC.module_shapes(name)
    cls, _, (b, d1, d2, h, w) = CC.MODULE_CASES[name]
    _, cot = CC.module_inputs(name)
    positions = b * (d2 if cls == "Upsample" else d1) * cot.shape[3] * cot.shape[4] // (4 if cls == "PixelShufflePack3D" else 1)
    return max(max(math.prod(s[1:]) for s in shapes.values() if len(s) == 5), positions)


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("name", list(CC.MODULE_CASES))
def test_modules_match_the_reference(name, tag):
    got = _run_module(name, tag)
    ref, cpu = _cpu("module", name, "fp64"), _cpu("module", name, tag)
    assert set(got) == set(ref) and len(got) == 2 + len(CC.module_shapes(name))
    for k in got:
        _judge(f"{name} {tag} {k}", got[k], ref[k], cpu[k], _floor(tag, _module_K(name)))
    again = _run_module(name, tag)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("tag", list(DTYPES))
def test_conv3d_reads_views_where_they_lie(tag):
    """a channel slice of a wider tensor and a transposed view give what their dense copies give, bit for bit, and the result lies
    in the view's memory order"""
    from vsrlab_amd.core.conv3d_ops import conv3d
    dtype = DTYPES[tag]
    wide = CC.rand(8101, 2, 3, 24, 6, 9, lo=-1.0).to(DEV).to(dtype)
    w, b = CC.rand(8102, 8, 16, 3, 3, 3, lo=-0.1, hi=0.1).to(DEV), CC.rand(8103, 8, lo=-0.1, hi=0.1).to(DEV)
    cot = CC.rand(8104, 2, 3, 8, 6, 9, lo=-1.0).to(DEV).to(dtype)

    def run(x, time_major, c):
        x = x.detach().requires_grad_(True)
        wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = conv3d(x, wl, bl, act="leaky_relu", slope=0.2, time_major=time_major)
        (y * c).sum().backward()
        return y.detach(), x.grad, wl.grad, bl.grad

    sliced = wide[:, :, 4:20]
    a, d = run(sliced, True, cot), run(sliced.contiguous(), True, cot)
    assert not sliced.is_contiguous() and a[0].is_contiguous()
    assert all(torch.equal(p, q) for p, q in zip(a, d))
    tr = sliced.contiguous().transpose(1, 2)                                             # (b, c, t, h, w) logically, (b, t, c, h, w) in memory
    e = run(tr, False, cot.transpose(1, 2))
    assert e[0].transpose(1, 2).is_contiguous() and torch.equal(e[0].transpose(1, 2), a[0]) and torch.equal(e[1].transpose(1, 2), a[1])
    assert torch.equal(e[2], a[2]) and torch.equal(e[3], a[3])


def test_refusals_on_the_gpu():
    from vsrlab_amd.core.conv3d_ops import conv3d
    x = torch.rand(1, 2, 3, 4, 4, device=DEV, requires_grad=True)
    w = torch.rand(4, 3, 3, 3, 3, device=DEV, requires_grad=True)
    y = conv3d(x, w, time_major=True)
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad(y.sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match="kernel"):
        conv3d(x, torch.rand(4, 3, 1, 1, 3, device=DEV), time_major=True)
    with pytest.raises(ValueError, match="channels"):
        conv3d(x, w)
    with pytest.raises(ValueError, match="multiple of 4"):
        conv3d(x, torch.rand(6, 3, 1, 3, 3, device=DEV), pixel_shuffle=2, time_major=True)
