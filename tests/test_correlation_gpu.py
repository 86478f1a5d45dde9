"""GPU checks of the fused local correlation (csrc/spatial_corr.hip) behind ``functional.spatial_correlation``,
``SpatialCorrelationSampler`` and ``compute_cost_volume``, against the fp64 restatements of tests/correlation_common.py (pinned
to the reference by tests/test_correlation_host.py).  The cases and what each catches: ``correlation_common.CASES``; case T spans
5 x 3 of the kernels' 8 x 32 tiles by output pixel and by input pixel alike (stride 1: the two tilings coincide)."""
import ctypes

import pytest
import torch

import correlation_common as CC
from attention_common import GUARD, SENTINEL, _guarded
from helpers import bf16_store, rel_err, rel_l2

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle():
    """per case: the fp64 restatement and its bf16-storage twin (out, d input1, d input2), computed once"""
    return {case: (CC.restate(case), CC.restate(case, store=bf16_store)) for case in CC.CASES}


def _hip(case, compute_dtype, grad=(True, True), via=None):
    from vsrlab_amd import functional as VF
    _, patch, stride, padding, dil = CC.CASES[case]
    a, b, cot = (t.to(_dev()) for t in CC.case_inputs(case, torch.float32))
    a.requires_grad_(grad[0]), b.requires_grad_(grad[1])
    if via is None:
        out = VF.spatial_correlation(a, b, patch, stride, padding, dil, compute_dtype=compute_dtype)
    else:
        out = via(a, b)
    if any(grad):
        (out * cot.reshape(out.shape)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), a.grad, b.grad


def _errors(got, want):
    return rel_err(got[0], want[0]), rel_l2(got[1], want[1]), rel_l2(got[2], want[2])


@pytest.mark.parametrize("case", list(CC.CASES))
def test_fp32_against_the_fp64_restatement(case, oracle):
    exact, _ = oracle[case]
    got = _hip(case, "fp32")
    assert tuple(got[0].shape) == tuple(exact[0].shape) and got[0].dtype == torch.float32
    e = _errors(got, exact)
    print(f"{case} fp32: out max-rel {e[0]:.3e}, d input1 rel-L2 {e[1]:.3e}, d input2 rel-L2 {e[2]:.3e}")
    assert max(e) < 1e-3, e


@pytest.mark.parametrize("case", list(CC.CASES))
def test_bf16_is_at_the_noise_floor_of_bf16_storage(case, oracle):
    exact, twin = oracle[case]
    e, floor = _errors(_hip(case, "bf16"), exact), _errors(twin, exact)
    print(f"{case} bf16: out max-rel {e[0]:.3e} (restatement {floor[0]:.3e}), d input1 rel-L2 {e[1]:.3e} ({floor[1]:.3e}), "
          f"d input2 rel-L2 {e[2]:.3e} ({floor[2]:.3e})")
    for got, fl in zip(e, floor):
        assert got <= 1.5 * max(fl, 1e-3), (e, floor)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["A", "G", "T"])
def test_two_runs_are_bit_identical(case, dt):
    a, b = _hip(case, dt), _hip(case, dt)
    assert torch.equal(a[0], b[0]), "forward differs between two runs"
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "a gradient (both are gathers) differs between two runs"


# ---- through the C ABI, every written operand inside a guard band ---------------------------------------------------------
def _abi(case, dt, want=(True, True)):
    """(out, d input1, d input2) by ctypes; out and the gradients lie in NaN / sentinel guard bands, the workspace in a byte
    guard band, and the bands are checked.  A gradient that is not wanted is passed as NULL."""
    from vsrlab_amd import _lib
    lib = _lib.load_spatial_corr()
    shape, patch, stride, padding, dil = CC.CASES[case]
    p, s, pad, d = CC.pair(patch), CC.pair(stride), CC.pair(padding), CC.pair(dil)
    dev = _dev()
    a, b, cot = (t.to(dev).contiguous() for t in CC.case_inputs(case, torch.float32))
    desc = _lib.SpatialCorrDesc(*shape, *p, *s, *pad, *d, _lib.DT_BF16 if dt == "bf16" else _lib.DT_F32, 1.0)
    nbytes = int(lib.vsr_spatial_corr_workspace_bytes(desc))
    assert nbytes > 0
    ws_buf, ws = _guarded((nbytes,), torch.uint8, dev, 0x5a)
    out_buf, out = _guarded(tuple(cot.shape), torch.float32, dev, float("nan"))
    g1_buf, g1 = _guarded(shape, torch.float32, dev, SENTINEL)
    g2_buf, g2 = _guarded(shape, torch.float32, dev, SENTINEL)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.vsr_spatial_corr_fwd(desc, ptr(a), ptr(b), ptr(out), ptr(ws), nbytes, st) == 0
    assert lib.vsr_spatial_corr_bwd(desc, ptr(a), ptr(b), ptr(cot), ptr(g1) if want[0] else None, ptr(g2) if want[1] else None, ptr(ws),
                                    nbytes, st) == 0
    torch.cuda.synchronize()
    for name, buf, fill in (("out", out_buf, None), ("d input1", g1_buf, SENTINEL), ("d input2", g2_buf, SENTINEL), ("workspace", ws_buf, 0x5a)):
        for band in (buf[:GUARD], buf[-GUARD:]):
            assert bool(band.isnan().all() if fill is None else (band == fill).all()), f"{case} {dt}: the guard band of {name} was written"
    assert bool(torch.isfinite(out).all()), "an element of out was not written"
    return out, g1, g2


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CC.CASES))
def test_guard_bands_and_the_c_abi_equals_the_autograd_path(case, dt):
    out, g1, g2 = _abi(case, dt)
    ref = _hip(case, dt)
    assert torch.equal(out, ref[0]) and torch.equal(g1, ref[1]) and torch.equal(g2, ref[2])


@pytest.mark.parametrize("case", ["C", "T"])
def test_a_null_gradient_is_not_computed(case):
    full = _abi(case, "fp32")
    _, g1, g2 = _abi(case, "fp32", want=(True, False))
    assert torch.equal(g1, full[1]) and bool((g2 == SENTINEL).all()), "d input2 was written though NULL was passed"
    _, g1, g2 = _abi(case, "fp32", want=(False, True))
    assert torch.equal(g2, full[2]) and bool((g1 == SENTINEL).all()), "d input1 was written though NULL was passed"
    out, d1, d2 = _hip(case, "fp32", grad=(True, False))
    assert d2 is None and torch.equal(d1, full[1]) and torch.equal(out, full[0])
    out, d1, d2 = _hip(case, "fp32", grad=(False, True))
    assert d1 is None and torch.equal(d2, full[2])


def test_unsampled_and_cropped_positions_get_zero_gradient():
    """case G, stride (2, 1) and padding (2, 0): the padded rows 0, 2, 4, ... are sampled, i.e. the even rows of input1"""
    _, d1, _ = _hip("G", "fp32")
    assert float(d1[:, :, 1::2].abs().max()) == 0.0 and float(d1[:, :, 0::2].abs().min()) > 0.0


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_cost_volume(dt, oracle):
    from vsrlab_amd import functional as VF
    from vsrlab_amd.optical_flow.models.irr.pwc_modules import compute_cost_volume
    shape = CC.CASES[CC.COST_CASE][0]
    k = 2 * CC.COST_MAX_DISP + 1
    pd = {"max_disp": CC.COST_MAX_DISP, "ignored": "as in the reference"}
    got = _hip(CC.COST_CASE, dt, via=lambda a, b: compute_cost_volume(a, b, pd, compute_dtype=dt))
    assert tuple(got[0].shape) == (shape[0], k * k, shape[2], shape[3])
    same = _hip(CC.COST_CASE, dt, via=lambda a, b: VF.spatial_correlation(a, b, k, scale=1.0 / shape[1], compute_dtype=dt))
    assert torch.equal(got[0], same[0].reshape(got[0].shape)) and torch.equal(got[1], same[1]) and torch.equal(got[2], same[2])
    exact = CC.restate_cost_volume()
    e = _errors(got, exact)
    print(f"cost volume {dt}: out max-rel {e[0]:.3e}, d feat1 rel-L2 {e[1]:.3e}, d feat2 rel-L2 {e[2]:.3e}")
    if dt == "fp32":
        assert max(e) < 1e-3, e
    else:
        floor = _errors(CC.restate_cost_volume(store=bf16_store), exact)
        for g, fl in zip(e, floor):
            assert g <= 1.5 * max(fl, 1e-3), (e, floor)


@pytest.mark.parametrize("case", ["C", "G"])
def test_module_equals_function(case):
    from vsrlab_amd.core.modules.correlation import SpatialCorrelationSampler, iter_spatial_correlation_sample
    _, patch, stride, padding, dil = CC.CASES[case]
    m = SpatialCorrelationSampler(patch_size=patch, stride=stride, padding=padding, dilation_patch=dil)
    ref, mod = _hip(case, "fp32"), _hip(case, "fp32", via=m)
    fn = _hip(case, "fp32", via=lambda a, b: iter_spatial_correlation_sample(a, b, 1, patch, stride, padding, 1, dil))
    for got in (mod, fn):
        assert all(torch.equal(x, y) for x, y in zip(got, ref))


def test_channel_order_is_the_references():
    """only pixel (ty, tx) of input2 is non-zero: the output pixel (ty + 1, tx - 2) meets it at displacement (-1, +2), i.e.
    i = 4 - 1 = 3 (vertical, slow) and j = 4 + 2 = 6"""
    from vsrlab_amd import functional as VF
    h, w, ty, tx = 12, 40, 6, 33
    a = torch.ones(1, 3, h, w, device=_dev())
    b = torch.zeros(1, 3, h, w, device=_dev())
    b[:, :, ty, tx] = 1.0
    out = VF.spatial_correlation(a, b, 9)
    win = out[0, :, :, ty + 1, tx - 2]
    assert int(win.flatten().argmax()) == 3 * 9 + 6 and int((win != 0).sum()) == 1 and float(win.max()) == 3.0


def test_non_contiguous_inputs_dtype_and_double_backward():
    from vsrlab_amd import functional as VF
    _, patch, stride, padding, dil = CC.CASES["C"]
    a, b, cot = (t.to(_dev()) for t in CC.case_inputs("C", torch.float32))
    want = VF.spatial_correlation(a, b, patch, stride, padding, dil)
    nc = lambda t: t.transpose(2, 3).contiguous().transpose(2, 3)
    assert not nc(a).is_contiguous() and torch.equal(VF.spatial_correlation(nc(a), nc(b), patch, stride, padding, dil), want)
    out64 = VF.spatial_correlation(a.double().requires_grad_(True), b.double(), patch, stride, padding, dil)
    assert out64.dtype == torch.float64 and torch.equal(out64.detach().float(), want)
    a.requires_grad_(True)
    out = VF.spatial_correlation(a, b, patch, stride, padding, dil)
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad((out * cot).sum(), a, create_graph=True)
