"""GPU checks of the integer-tap warps (csrc/warp_taps.hip) behind ``flow_warp(..., 'nearest' / 'nearest4')``,
``functional.aligned_input`` and vsr/models/VRT/vrt.py, against the numpy oracle of tests/warp_taps_common.py (pinned to the
reference bit for bit by tests/test_warp_taps_host.py).  The op is a gather, so every forward comparison is ``torch.equal`` with no
tolerance and no exempt pixels; the backward is exact under integer cotangents and held to the fp32 summation bound under random
ones.  The cases and what each catches: ``warp_taps_common.CASES``."""
import ctypes

import pytest
import torch

import warp_taps_common as WT
from attention_common import GUARD, SENTINEL, _guarded

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
MODES = [(4, "nearest4"), (1, "nearest")]
CLIP_IDS = [WT.clip_name(*c) for c in WT.CLIP_CASES]


def _dev():
    return torch.device("cuda:0")


def _warp(x, flow_planar, mode, padding="zeros"):
    from vsrlab_amd.vsr.models.VRT.modules.spynet import flow_warp
    out = flow_warp(x, WT.to_channels_last(flow_planar), mode, padding)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def flows():
    """per (case, taps): the planar flow on the host, computed once and left unchanged"""
    return {(name, taps): WT.case_flow(name, taps) for name in WT.CASES for taps, _ in MODES}


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("taps,mode", MODES)
@pytest.mark.parametrize("name", list(WT.CASES))
def test_forward_equals_the_oracle_bit_for_bit(name, taps, mode, padding, dt, flows):
    x, flow = WT.case_x(name, dt), flows[name, taps]
    want = WT.warp(x, flow, taps, border=padding == "border")
    xd = x.to(_dev())
    keep = xd.clone()
    out = _warp(xd, flow.to(_dev()), mode, padding)
    assert out.shape == want.shape and out.dtype == dt and out.is_contiguous()
    assert torch.equal(xd, keep), "the input was modified"
    bad = int((out.cpu() != want).sum())
    print(f"{name} {mode} {padding} {dt}: {bad} of {want.numel()} values differ from the oracle")
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_non_finite_flows_give_zeros(dt):
    x = WT.case_x("odd", dt).to(_dev())
    for v in (float("nan"), float("inf"), float("-inf"), 3.4e38):
        flow = torch.full((2, 2, 5, 7), v)
        flow[:, 1] = 0.25                                             # one coordinate in frame, the other not
        for taps, mode in MODES:
            out = _warp(x, flow.to(_dev()), mode)
            assert not out.any() and torch.equal(out.cpu(), WT.warp(x.cpu(), flow, taps))


@pytest.mark.parametrize("taps,mode", MODES)
def test_input_forms_give_the_same_bits(taps, mode, flows):
    """the permuted, non-contiguous flow the reference passes and a frame x[:, i] of a clip against the contiguous forms; a bilinear
    call before and after: no state is shared"""
    from vsrlab_amd.vsr.models.VRT.modules.spynet import flow_warp
    dev = _dev()
    flow = flows["vec", taps].to(dev)
    clip = torch.stack([WT.case_x("vec"), WT.case_x("chan", shape=WT.CASES["vec"][0]), WT.case_x("odd", shape=WT.CASES["vec"][0])], 1).to(dev)
    x = clip[:, 1]
    assert not x.is_contiguous() and not WT.to_channels_last(flow).is_contiguous()
    bil = flow_warp(clip[:, 0].contiguous(), WT.to_channels_last(flow))
    want = WT.warp(x.cpu(), flow.cpu(), taps)
    a = flow_warp(x, WT.to_channels_last(flow), mode)                                   # slice of a clip, permuted flow
    b = flow_warp(x.contiguous(), WT.to_channels_last(flow).contiguous(), interp_mode=mode)
    c = flow_warp(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), WT.to_channels_last(flow), mode)   # channels-last x: copied
    d = flow_warp(x, WT.to_channels_last(flow.double()), mode)                          # the host side converts the flow to fp32
    torch.cuda.synchronize()
    for got in (a, b, c, d):
        assert torch.equal(got.cpu(), want)
    assert torch.equal(flow_warp(clip[:, 0].contiguous(), WT.to_channels_last(flow)), bil)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("clip", WT.CLIP_CASES, ids=CLIP_IDS)
def test_aligned_input_equals_the_oracle_and_the_per_pair_calls(clip, dt):
    from vsrlab_amd.vsr.models.VRT import vrt
    from vsrlab_amd.vsr.models.VRT.modules.spynet import flow_warp
    dev = _dev()
    x, fb, ff = WT.clip_inputs(*clip, dtype=dt)
    want = WT.aligned_input(x, fb, ff)
    xd, fbd, ffd = x.to(dev), fb.to(dev), ff.to(dev)
    keep = xd.clone()
    out = vrt.aligned_input(xd, fbd, ffd)
    assert out.dtype == dt and out.is_contiguous() and torch.equal(xd, keep)
    assert torch.equal(out.cpu(), want)
    xb, xf = vrt.get_aligned_image(xd, fbd, ffd)
    n = xd.size(1)
    # the reference's composition (vrt.py:211-228) from per-pair flow_warp calls
    rb = [torch.zeros_like(xd[:, -1]).repeat(1, 4, 1, 1)]
    for i in range(n - 1, 0, -1):
        rb.insert(0, flow_warp(xd[:, i], fbd[:, i - 1].permute(0, 2, 3, 1), 'nearest4'))
    rf = [torch.zeros_like(xd[:, 0]).repeat(1, 4, 1, 1)]
    for i in range(0, n - 1):
        rf.append(flow_warp(xd[:, i], ffd[:, i].permute(0, 2, 3, 1), 'nearest4'))
    rb, rf = torch.stack(rb, 1), torch.stack(rf, 1)
    assert torch.equal(xb, rb) and torch.equal(xf, rf)
    assert torch.equal(out, torch.cat([xd, rb, rf], 2))
    assert xb.untyped_storage().data_ptr() == xf.untyped_storage().data_ptr(), "the two halves are views of one result: nothing is copied"


def _round(t, dt):
    return t.to(dt) if dt == torch.bfloat16 else t.to(torch.float32)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("taps,mode", MODES)
@pytest.mark.parametrize("name", list(WT.CASES))
def test_backward_with_grid_cotangents_is_exact(name, taps, mode, padding, dt, flows):
    dev = _dev()
    flow = flows[name, taps]
    x = WT.case_x(name, dt).to(dev).requires_grad_(True)
    from vsrlab_amd.vsr.models.VRT.modules.spynet import flow_warp
    fl = WT.to_channels_last(flow.to(dev)).requires_grad_(True)                   # the leaf is the (N, H, W, 2) view itself
    out = flow_warp(x, fl, mode, padding)
    cot = WT.grid_cotangent(f"{name}:{mode}", out.shape)
    out.backward(cot.to(device=dev, dtype=dt))
    torch.cuda.synchronize()
    want = WT.warp_grad(cot, flow, taps, border=padding == "border")
    assert x.grad.dtype == dt and x.grad.shape == x.shape
    assert torch.equal(x.grad.cpu(), _round(want, dt)), "bf16: the oracle's value rounded once"
    assert fl.grad is not None and fl.grad.shape == fl.shape and not fl.grad.any(), "the flow gradient is a zeros tensor"


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("clip", WT.CLIP_CASES, ids=CLIP_IDS)
def test_clip_backward_with_grid_cotangents_is_exact(clip, dt):
    from vsrlab_amd.vsr.models.VRT import vrt
    dev = _dev()
    x, fb, ff = WT.clip_inputs(*clip, dtype=dt)
    xd = x.to(dev).requires_grad_(True)
    fbd, ffd = fb.to(dev).requires_grad_(True), ff.to(dev)
    out = vrt.aligned_input(xd, fbd, ffd)
    cot = WT.grid_cotangent(WT.clip_name(*clip), out.shape)
    out.backward(cot.to(device=dev, dtype=dt))
    torch.cuda.synchronize()
    want = WT.aligned_input_grad(cot, fb, ff)
    assert torch.equal(xd.grad.cpu(), _round(want, dt))
    assert fbd.grad is not None and not fbd.grad.any() and ffd.grad is None
    # through get_aligned_image's two views: the cotangent of the copy of x is then zero
    xd.grad = None
    xb, xf = vrt.get_aligned_image(xd, fbd, ffd)
    c = x.size(2)
    (xb * cot[:, :, c:5 * c].to(device=dev, dtype=dt)).sum().backward(retain_graph=True)
    (xf * cot[:, :, 5 * c:].to(device=dev, dtype=dt)).sum().backward()
    torch.cuda.synchronize()
    zeroed = cot.clone()
    zeroed[:, :, :c] = 0
    assert torch.equal(xd.grad.cpu(), _round(WT.aligned_input_grad(zeroed, fb, ff), dt))


def _check_bound(got, want, cnt, mag, what):
    """|got - want64| <= k 2^-23 S per source value: k contributions of magnitude sum S.  The fp32 recursive-summation bound
    (k - 1) u S with u = 2^-24, times 2 for the second-order terms and the rounding of the cotangent's own fp32 value: derived, not
    measured."""
    bound = cnt * 2.0 ** -23 * mag
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest |error| / bound = {ratio:.3f}, largest k = {int(cnt.max())}")
    assert (err <= bound).all()


@pytest.mark.parametrize("taps,mode", MODES)
@pytest.mark.parametrize("name", list(WT.CASES))
def test_backward_with_random_cotangents_is_within_the_summation_bound(name, taps, mode, flows):
    dev = _dev()
    flow = flows[name, taps]
    x = WT.case_x(name).to(dev).requires_grad_(True)
    out = _warp(x, flow.to(dev), mode)
    cot = WT.random_cotangent(f"{name}:{mode}", out.shape)
    out.backward(cot.to(dev))
    torch.cuda.synchronize()
    want, cnt, mag = WT.warp_grad(cot, flow, taps, stats=True)
    _check_bound(x.grad.cpu(), want, cnt, mag, f"{name} {mode}")


@pytest.mark.parametrize("clip", WT.CLIP_CASES, ids=CLIP_IDS)
def test_clip_backward_with_random_cotangents_is_within_the_summation_bound(clip):
    from vsrlab_amd.vsr.models.VRT import vrt
    dev = _dev()
    x, fb, ff = WT.clip_inputs(*clip)
    xd = x.to(dev).requires_grad_(True)
    out = vrt.aligned_input(xd, fb.to(dev), ff.to(dev))
    cot = WT.random_cotangent(WT.clip_name(*clip), out.shape)
    out.backward(cot.to(dev))
    torch.cuda.synchronize()
    want, cnt, mag = WT.aligned_input_grad(cot, fb, ff, stats=True)
    _check_bound(xd.grad.cpu(), want, cnt, mag, WT.clip_name(*clip))


def test_gradients_are_none_for_inputs_that_do_not_require_them():
    from vsrlab_amd import functional as VF
    dev = _dev()
    x, flow = WT.case_x("odd").to(dev), WT.to_channels_last(WT.case_flow("odd").to(dev))
    fl = flow.clone().requires_grad_(True)
    out = VF.flow_warp(x, fl, "nearest4")                             # only the flow requires grad
    assert out.requires_grad
    gf, = torch.autograd.grad(out.sum(), (fl,))
    assert gf.shape == fl.shape and not gf.any()
    xr = x.clone().requires_grad_(True)
    out = VF.flow_warp(xr, flow, "nearest4")
    out.sum().backward()
    assert xr.grad is not None and flow.grad is None
    assert not VF.flow_warp(x, flow, "nearest").requires_grad


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bands_intact(buf, what):
    for band in (buf[:GUARD], buf[-GUARD:]):
        assert bool((band == SENTINEL).all()), f"the guard band of {what} was written"


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["wide", "chan", "far", "vec"])
def test_guard_bands_of_the_pair_entries(name, dt, flows):
    """outputs, accumulator and gx lie in sentinel guard bands"""
    from vsrlab_amd import _lib
    lib = _lib.load_warp_taps()
    dev = _dev()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = _lib.DT_BF16 if dt == torch.bfloat16 else _lib.DT_F32
    n, c, h, w = WT.CASES[name][0]
    x = WT.case_x(name, dt)
    xd = x.to(dev)
    for taps, mode in MODES:
        flow = flows[name, taps]
        fd = flow.to(dev)
        desc = _lib.WarpTapsDesc(n, 1, c, h, w, taps, 0, code, 0)
        out_buf, out = _guarded((n, taps * c, h, w), dt, dev, SENTINEL)
        assert lib.vsr_warp_taps_fwd(desc, _ptr(xd), _ptr(fd), _ptr(out), st) == 0
        torch.cuda.synchronize()
        _bands_intact(out_buf, f"{name} {mode} out")
        assert torch.equal(out.cpu(), WT.warp(x, flow, taps))
        cot = WT.grid_cotangent(f"{name}:{mode}", out.shape)
        acc_buf, acc = _guarded((n, c, h, w), torch.float32, dev, SENTINEL)
        gx_buf, gx = (acc_buf, acc) if dt == torch.float32 else _guarded((n, c, h, w), dt, dev, SENTINEL)
        assert lib.vsr_warp_taps_bwd(desc, _ptr(cot.to(device=dev, dtype=dt)), _ptr(fd), _ptr(acc), _ptr(gx), st) == 0
        torch.cuda.synchronize()
        _bands_intact(acc_buf, f"{name} {mode} acc")
        _bands_intact(gx_buf, f"{name} {mode} gx")
        assert torch.equal(gx.cpu(), _round(WT.warp_grad(cot, flow, taps), dt))


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("clip", [(1, 2, (3, 6, 10)), (1, 2, (3, 9, 66)), (2, 2, (3, 4, 16))], ids=lambda c: WT.clip_name(*c))
def test_guard_bands_of_the_clip_entries(clip, dt):
    from vsrlab_amd import _lib
    lib = _lib.load_warp_taps()
    dev = _dev()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = _lib.DT_BF16 if dt == torch.bfloat16 else _lib.DT_F32
    b, d, (c, h, w) = clip
    x, fb, ff = WT.clip_inputs(*clip, dtype=dt)
    xd, fbd, ffd = x.to(dev), fb.to(dev), ff.to(dev)
    desc = _lib.WarpTapsDesc(b, d, c, h, w, 4, 0, code, 0)
    out_buf, out = _guarded((b, d, 9 * c, h, w), dt, dev, SENTINEL)
    assert lib.vsr_warp_taps_clip_fwd(desc, _ptr(xd), _ptr(fbd), _ptr(ffd), _ptr(out), st) == 0
    torch.cuda.synchronize()
    _bands_intact(out_buf, "the aligned input")
    assert torch.equal(out.cpu(), WT.aligned_input(x, fb, ff))
    cot = WT.grid_cotangent(WT.clip_name(*clip), out.shape)
    acc_buf, acc = _guarded((b, d, c, h, w), torch.float32, dev, SENTINEL)
    gx_buf, gx = (acc_buf, acc) if dt == torch.float32 else _guarded((b, d, c, h, w), dt, dev, SENTINEL)
    assert lib.vsr_warp_taps_clip_bwd(desc, _ptr(cot.to(device=dev, dtype=dt)), _ptr(fbd), _ptr(ffd), _ptr(acc), _ptr(gx), st) == 0
    torch.cuda.synchronize()
    _bands_intact(acc_buf, "the clip accumulator")
    _bands_intact(gx_buf, "the clip gx")
    assert torch.equal(gx.cpu(), _round(WT.aligned_input_grad(cot, fb, ff), dt))


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_repeats_are_bit_identical(dt, flows):
    from vsrlab_amd.vsr.models.VRT import vrt
    dev = _dev()
    flow = flows["vec", 4].to(dev)
    outs, grads = [], []
    for _ in range(2):
        x = WT.case_x("vec", dt).to(dev).requires_grad_(True)
        out = _warp(x, flow, "nearest4")
        out.backward(WT.grid_cotangent("repeat", out.shape).to(device=dev, dtype=dt))
        outs.append(out.detach())
        grads.append(x.grad)
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])
    xc, fb, ff = (t.to(dev) for t in WT.clip_inputs(2, 3, (3, 9, 66), dtype=dt))
    outs, grads = [], []
    for _ in range(2):
        leaf = xc.clone().requires_grad_(True)
        out = vrt.aligned_input(leaf, fb, ff)
        out.backward(WT.grid_cotangent("repeat-clip", out.shape).to(device=dev, dtype=dt))
        outs.append(out.detach())
        grads.append(leaf.grad)
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])


def test_nothing_is_saved_without_a_gradient_to_compute():
    """tensors packed for the backward: the flow(s) when x requires grad, nothing under no_grad or when only the flow does"""
    from vsrlab_amd import functional as VF
    dev = _dev()
    x, flow = WT.case_x("odd").to(dev), WT.to_channels_last(WT.case_flow("odd").to(dev))
    xc, fb, ff = (t.to(dev) for t in WT.clip_inputs(1, 2, (3, 6, 10)))
    packed = []

    def pack(t):
        packed.append(tuple(t.shape))
        return t

    def count(fn):
        packed.clear()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = fn()
        return len(packed), out

    with torch.no_grad():
        k, out = count(lambda: VF.flow_warp(x.clone().requires_grad_(True), flow, "nearest4"))
        assert k == 0 and not out.requires_grad and out.grad_fn is None
        k, out = count(lambda: VF.aligned_input(xc.clone().requires_grad_(True), fb, ff))
        assert k == 0 and not out.requires_grad
    assert count(lambda: VF.flow_warp(x, flow.clone().requires_grad_(True), "nearest4"))[0] == 0
    assert count(lambda: VF.flow_warp(x.clone().requires_grad_(True), flow, "nearest4"))[0] == 1
    assert count(lambda: VF.aligned_input(xc.clone().requires_grad_(True), fb, ff))[0] == 2


def test_get_flows_on_the_hip_spynet():
    """each returned level equals the direct SpyNet call viewed as (b, n - 1, 2, h / 2^i, w / 2^i), backward and forward in the frame
    order of vrt.py:199,204"""
    from vsrlab_amd.vsr.models.VRT import vrt
    from vsrlab_amd.vsr.models.VRT.modules.spynet import SpyNet
    dev = _dev()
    torch.manual_seed(0)
    net = SpyNet(pretrained=False, return_levels=[3, 4, 5]).to(dev).eval()
    b, n, c, h, w = 1, 3, 3, 64, 64
    x = torch.rand(b, n, c, h, w, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        fbs, ffs = vrt.get_flows(net, x)
        x1, x2 = x[:, :-1].reshape(-1, c, h, w), x[:, 1:].reshape(-1, c, h, w)
        db, df = net(x1, x2), net(x2, x1)
    assert len(fbs) == len(ffs) == 3
    for i in range(3):
        shape = (b, n - 1, 2, h >> i, w >> i)
        assert fbs[i].shape == shape and ffs[i].shape == shape
        assert torch.equal(fbs[i], db[i].view(shape)) and torch.equal(ffs[i], df[i].view(shape))
    assert not torch.equal(fbs[0], ffs[0])
    # and the front of VRT.forward end to end: the flows of level 0 feed the aligned input
    out = vrt.aligned_input(x, fbs[0], ffs[0])
    assert torch.equal(out.cpu(), WT.aligned_input(x.cpu(), fbs[0].cpu(), ffs[0].cpu()))


def test_a_cpu_tensor_is_refused():
    from vsrlab_amd import functional as VF
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.flow_warp(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 2), "nearest4")
