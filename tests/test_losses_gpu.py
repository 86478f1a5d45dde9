"""GPU tests of libvsrlab_losses.so and what stands on it: the fused L1 / RMSE pair reductions behind WL1Loss and rmse_loss, the
adjoint of the bilinear resize behind core.utils.resize, and LossPipeline on both.  Checkers: the fp64 restatement of
tests/losses_common.py (pinned to the reference's recorded results by tests/test_losses_host.py), torch's CPU F.interpolate under
autograd, and tests/golden/loss_pipeline.npz."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import losses_common as LC
from helpers import golden, rand, rel_err

pytestmark = pytest.mark.gpu

from oracle import basicvsr_oracle as O  # noqa: E402  (checker only)


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


# ---- the pair reductions ------------------------------------------------------------------------------------------------------
# The launch of csrc/pixel_losses.hip: at most vsr_pixel_loss_scratch_floats() = 1024 workgroups of 256 lanes, a lane moving 8
# elements per trip, so one sweep of the grid covers 1024 * 256 * 8 = 2,097,152 elements.  Two full sweeps make every lane take two
# trips; 3 * 256 * 8 more give the first three workgroups a third, and 5 more leave a tail that is no whole vector: 4,200,453.
BLOCK, VEC = 256, 8


def _two_trips():
    from vsrlab_amd import _lib
    sweep = _lib.load_losses().vsr_pixel_loss_scratch_floats() * BLOCK * VEC
    return 2 * sweep + 3 * BLOCK * VEC + 5


SHAPES = ["one", "seven", "ragged", "unaligned", "two_trips"]
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]
_cases = {}


def _case(name, xdt, ydt):
    """x, y on the GPU in their dtypes (y equal to x at every third element: ties), and the same rounded values in fp64 on the CPU.
    Built once per case and left unchanged."""
    key = (name, xdt, ydt)
    if key not in _cases:
        dev = _gpu()
        shape = {"one": (1,), "seven": (7,), "ragged": (1, 2, 3, 5, 7), "unaligned": (2, 3, 5, 7), "two_trips": (_two_trips(),)}[name]
        x, y = rand(711, *shape).to(xdt), rand(712, *shape).to(ydt)
        if x.numel() > 1:
            y.view(-1)[::3] = x.view(-1)[::3].to(ydt)             # exact in every pairing of DTYPES (a bf16 x in an fp32 y)
        xg, yg = x.to(dev), y.to(dev)
        if name == "unaligned":                                   # a contiguous view at a storage offset that is no multiple of 16 bytes
            x, y, xg, yg = x[0, 1:], y[0, 1:], xg[0, 1:], yg[0, 1:]
            assert xg.is_contiguous() and xg.data_ptr() % 16 != 0 and yg.data_ptr() % 16 != 0
        _cases[key] = (xg, yg, x.double(), y.double())
    return _cases[key]


def _ref(fn, x64, y64):
    x, y = x64.clone().requires_grad_(True), y64.clone().requires_grad_(True)
    v = fn(x, y)
    v.backward()
    return float(v.detach()), x.grad, y.grad


def _run(fn, xg, yg, wrt=(True, False)):
    x, y = xg.detach().requires_grad_(wrt[0]), yg.detach().requires_grad_(wrt[1])
    v = fn(x, y)
    v.backward()
    return v.detach(), x.grad, y.grad


@pytest.mark.parametrize("xdt,ydt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("name", SHAPES)
def test_l1_value_and_exact_gradient(name, xdt, ydt):
    from vsrlab_amd.core.losses import WL1Loss
    xg, yg, x64, y64 = _case(name, xdt, ydt)
    n = x64.numel()
    want, _, _ = _ref(LC.l1, x64, y64)
    v, gx, _ = _run(WL1Loss(), xg, yg)
    err = abs(float(v) - want) / want if want else abs(float(v))
    print(f"l1 {name} {xdt}/{ydt}: value rel err {err:.3e}")
    assert v.dtype == torch.float32 and err < 1e-5
    # exact by construction: sign(x - y) * fp32(1 / N), sign(0) = 0, rounded to x's dtype
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    want_g = (torch.sign(x64 - y64).float() * scale).to(xdt)
    assert gx.dtype == xdt and torch.equal(gx.cpu(), want_g)
    if n > 1:
        assert int((want_g == 0).sum()) >= n // 3                 # the ties are there
    # the second argument gets the exact negation; both at once are the same bits
    v2, gx2, gy2 = _run(WL1Loss(), xg, yg, wrt=(True, True))
    assert gy2.dtype == ydt and torch.equal(gy2, (-gx).to(ydt)) and torch.equal(gx2, gx) and torch.equal(v2, v)
    _, none, gy3 = _run(WL1Loss(), xg, yg, wrt=(False, True))
    assert none is None and torch.equal(gy3, gy2)
    with torch.no_grad():
        assert torch.equal(WL1Loss()(xg, yg), v)                  # value only (null gradient pointer): the same bits


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("n,aligned", [(n, True) for n in LC.ORDER_SIZES] + [(2051, False)], ids=lambda v: str(v))
def test_the_value_is_summed_in_the_stated_order(n, aligned, kind):
    """The contract of csrc/reduce.h, pinned: vsr_pixel_loss_fwd_bwd returns exactly the bits of LC.emulate_pair_loss_order -- the
    per-lane strided sums, the 64-lane shuffle tree, the PAIRWISE combiner, fp32(1 / n), the partials at stride 256 and the halving
    tree; the in-order combiner or a running sum over the partials give other bits (tests/test_losses_host.py).  Subtract, abs,
    multiply and add are all there is to these two values, so numpy fp32 reproduces them exactly.  `aligned=False`: views offset by
    one element, the scalar path.  Charbonnier (csrc/elementwise.hip) and the gradient norm (csrc/train_step.hip) take the same
    header functions but have a sqrtf in the value, whose device rounding numpy does not restate: they are covered by the identity of
    their instruction streams with the spelled-out form (profiles/reduce_header_isa.md) and by their own tests, not by an emulation."""
    from vsrlab_amd import _lib
    from vsrlab_amd.functional import _STORAGE_DT, _ptr, _stream
    dev = _gpu()
    lib = _lib.load_losses()
    x, y = LC.order_operands(n)
    want = torch.from_numpy(np.asarray(LC.emulate_pair_loss_order(x.numpy(), y.numpy(), kind, aligned=aligned)).reshape(()))
    if aligned:
        xg, yg = x.to(dev), y.to(dev)
    else:
        xg, yg = (torch.cat([t.new_zeros(1), t]).to(dev)[1:] for t in (x, y))
    assert xg.is_contiguous() and ((xg.data_ptr() | yg.data_ptr()) % 16 == 0) == aligned
    dx = torch.empty(n + 1, dtype=torch.float32, device=dev)[0 if aligned else 1:][:n]
    assert (dx.data_ptr() % 16 == 0) == aligned
    f32 = _STORAGE_DT[torch.float32]
    got = []
    for _ in range(2):
        loss = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        scratch = torch.full((lib.vsr_pixel_loss_scratch_floats(),), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(lib.vsr_pixel_loss_fwd_bwd({"l1": _lib.LOSS_L1, "mse": _lib.LOSS_MSE}[kind], _ptr(xg), f32, _ptr(yg), f32, _ptr(dx),
                                              _ptr(loss), _ptr(scratch), n, _stream()), "pixel_loss")
        got.append(loss.cpu())
    print(f"order {kind} n={n} aligned={aligned}: entry {float(got[0])!r} emulation {float(want)!r}")
    assert torch.equal(got[0].view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), got[0].view(torch.int32))


@pytest.mark.parametrize("xdt,ydt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("name", SHAPES)
def test_rmse_value_and_gradient(name, xdt, ydt):
    from vsrlab_amd.core.losses import rmse_loss
    xg, yg, x64, y64 = _case(name, xdt, ydt)
    want, want_gx, _ = _ref(LC.rmse, x64, y64)
    v, gx, _ = _run(rmse_loss, xg, yg)
    err = abs(float(v) - want) / want
    assert v.dtype == torch.float32 and gx.dtype == xdt
    if xdt == torch.float32:
        g_err = rel_err(gx, want_gx)
        print(f"rmse {name} {xdt}/{ydt}: value rel err {err:.3e}, gradient rel err {g_err:.3e}")
        assert g_err < 1e-5
    else:
        # within one bf16 step (2^-7 relative) of the fp64 gradient rounded to bf16
        rounded = want_gx.to(torch.bfloat16).double()
        diff = (gx.cpu().double() - rounded).abs()
        print(f"rmse {name} {xdt}/{ydt}: value rel err {err:.3e}, bf16 gradient elements that differ from the rounded fp64 one: "
              f"{float((diff > 0).double().mean()):.4f}, max difference {float((diff / rounded.abs().clamp_min(1e-30)).max()):.3e} relative")
        assert bool((diff <= 2.0 ** -7 * rounded.abs()).all())
    assert err < 1e-5
    v2, gx2, gy2 = _run(rmse_loss, xg, yg, wrt=(True, True))
    assert gy2.dtype == ydt and torch.equal(gy2, (-gx).to(ydt)) and torch.equal(gx2, gx) and torch.equal(v2, v)
    with torch.no_grad():
        assert torch.equal(rmse_loss(xg, yg), v)


def test_rmse_of_equal_operands_is_zero_with_a_nan_gradient():
    from vsrlab_amd.core.losses import rmse_loss
    xg = _case("ragged", torch.float32, torch.float32)[0]
    v, gx, _ = _run(rmse_loss, xg, xg.clone())
    assert float(v) == 0.0 and bool(torch.isnan(gx).all())


def test_no_double_backward():
    from vsrlab_amd.core.losses import WL1Loss, rmse_loss
    xg, yg, _, _ = _case("ragged", torch.float32, torch.float32)
    for fn in (WL1Loss(), rmse_loss):
        x = xg.detach().requires_grad_(True)
        with pytest.raises(RuntimeError, match="no double backward"):
            torch.autograd.grad(fn(x, yg), x, create_graph=True)


def test_single_losses_against_the_reference():
    """tests/golden/loss_pipeline.npz part 2: WL1Loss(2.0, reduction="sum") is twice the MEAN; rmse_loss; both gradients"""
    from vsrlab_amd.core.losses import WL1Loss, rmse_loss
    dev = _gpu()
    gold = golden("loss_pipeline")
    x, y = (t.to(dev) for t in LC.single_inputs())
    for tag, fn in (("wl1", WL1Loss(LC.SINGLE_L1_WEIGHT, reduction="sum")), ("rmse", rmse_loss)):
        v, gx, gy = _run(fn, x, y, wrt=(True, True))
        want = float(gold[f"{tag}__value"])
        print(f"{tag}: value rel err {abs(float(v) - want) / want:.3e}, d x {rel_err(gx, gold[f'{tag}__dx']):.3e}, d y {rel_err(gy, gold[f'{tag}__dy']):.3e}")
        assert abs(float(v) - want) < 1e-5 * want
        assert rel_err(gx, gold[f"{tag}__dx"]) < 1e-5 and rel_err(gy, gold[f"{tag}__dy"]) < 1e-5


# ---- the adjoint of the resize ------------------------------------------------------------------------------------------------
SIZES = [((64, 96), (16, 24)), ((37, 53), (9, 13)), ((20, 28), (40, 56)), ((9, 13), (37, 53)), ((8, 8), (8, 8)), ((1, 5), (3, 2)),
         ((6, 1), (1, 4))]


@pytest.mark.parametrize("src,dst", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_adjoint(src, dst):
    dev = _gpu()
    from vsrlab_amd.core.utils import resize
    x = rand(721, 2, 3, *src)
    d = rand(722, 2, 3, *dst, lo=0.5, hi=1.5)                     # positive: a zero of the gradient is a pixel that nothing samples
    xc = x.clone().requires_grad_(True)
    F.interpolate(xc.reshape(-1, 1, *src), size=dst, mode="bilinear", align_corners=False).reshape(2, 3, *dst).backward(d)
    xg = x.to(dev).requires_grad_(True)
    out = resize(xg, dst)
    out.backward(d.to(dev))
    g = xg.grad
    err = rel_err(g, xc.grad)
    # <R x, d> = <x, R^T d> on the two HIP kernels, the sums in fp64 on the host
    lhs = float((out.detach().cpu().double() * d.double()).sum())
    rhs = float((x.double() * g.cpu().double()).sum())
    bound = 1e-5 * float((out.detach().cpu().double().abs() * d.double().abs()).sum())
    print(f"resize adjoint {src} -> {dst}: rel err {err:.3e}, |<Rx,d> - <x,R^T d>| {abs(lhs - rhs):.3e} (bound {bound:.3e})")
    assert g.shape == x.shape and g.dtype == torch.float32 and err < 1e-5
    assert abs(lhs - rhs) <= bound
    xg2 = x.to(dev).requires_grad_(True)
    resize(xg2, dst).backward(d.to(dev))
    assert torch.equal(xg2.grad, g)
    if src[0] >= 2 * dst[0] and src[1] >= 2 * dst[1]:             # down-scaling without antialiasing: pixels that no output samples
        unsampled = xc.grad == 0
        assert int(unsampled.sum()) > 0 and bool((g.cpu()[unsampled] == 0).all()) and bool((g.cpu()[~unsampled] > 0).all())


def test_resize_is_differentiable_and_keeps_the_input_dtype():
    dev = _gpu()
    from vsrlab_amd.core.utils import resize
    x = rand(723, 1, 2, 3, 9, 13).to(dev)
    with torch.no_grad():
        plain = resize(x, (5, 7))
    xr = x.clone().requires_grad_(True)
    out = resize(xr, (5, 7))                                      # raised NotImplementedError before
    assert out.requires_grad and torch.equal(out.detach(), plain) and not resize(x, (5, 7)).requires_grad
    xb = x.to(torch.bfloat16).requires_grad_(True)
    ob = resize(xb, (5, 7))
    ob.sum().backward()
    out.sum().backward()
    assert ob.dtype == torch.float32 and xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, xr.grad.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="no double backward"):
        xr2 = x.clone().requires_grad_(True)
        torch.autograd.grad(resize(xr2, (5, 7)).sum(), xr2, create_graph=True)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------
class Rmse(nn.Module):
    def forward(self, x, y):
        from vsrlab_amd.core.losses import rmse_loss
        return rmse_loss(x, y)


def _pipeline():
    from vsrlab_amd.core.losses import CharbonnierLoss, LossPipeline, WL1Loss
    return LossPipeline({"rmse": Rmse(), "l1": WL1Loss(LC.L1_WEIGHT), "charb": CharbonnierLoss(LC.CHARB_EPS)}, LC.PIPELINE,
                        prefix=LC.PREFIX, postfix=LC.POSTFIX)


def _evaluate(pipe):
    dev = _gpu()
    sr, hr, lq = (t.to(dev) for t in LC.pipeline_inputs())
    sr.requires_grad_(True), lq.requires_grad_(True)
    out = pipe({"sr": sr, "hr": hr, "lq": lq})
    total = [k for k in out if k.endswith("loss" + (pipe.postfix or ""))]
    assert len(total) == 1
    out[total[0]].backward()
    return {k: v.detach() for k, v in out.items() if k not in ("sr", "hr", "lq")}, sr.grad, lq.grad


def test_pipeline_against_the_reference():
    """the recorded pipeline (tests/golden/loss_pipeline.npz part 1) in fp32: this package's CharbonnierLoss (the kernel of
    libvsrlab_hip.so), WL1Loss and rmse_loss (libvsrlab_losses.so) and both directions of the resize in ONE autograd graph; the
    reference's pipeline has no OpticalFlowConsistency term either"""
    gold = golden("loss_pipeline")
    vals, dsr, dlq = _evaluate(_pipeline())
    assert sorted(vals) == sorted(LC.OUTPUT_KEYS)
    for k in LC.OUTPUT_KEYS:
        want = float(gold["pipe__" + k.replace("/", "|")])
        print(f"pipeline {k}: {float(vals[k]):.7f}, rel err {abs(float(vals[k]) - want) / want:.3e}")
        assert abs(float(vals[k]) - want) < 1e-5 * want
    print(f"pipeline d sr rel err {rel_err(dsr, gold['pipe__dsr']):.3e}, d lq rel err {rel_err(dlq, gold['pipe__dlq']):.3e}")
    assert rel_err(dsr, gold["pipe__dsr"]) < 1e-5 and rel_err(dlq, gold["pipe__dlq"]) < 1e-5


def test_a_cloned_pipeline_gives_the_same_numbers_under_its_names():
    pipe = _pipeline()
    vals, dsr, dlq = _evaluate(pipe)
    twin = pipe.clone(prefix="val/")
    tvals, tdsr, tdlq = _evaluate(twin)
    assert sorted(tvals) == sorted("val/" + k[len(LC.PREFIX):] for k in vals)
    assert all(torch.equal(tvals["val/" + k[len(LC.PREFIX):]], v) for k, v in vals.items())
    assert torch.equal(tdsr, dsr) and torch.equal(tdlq, dlq)


def test_compute_loss_is_unchanged():
    """the first block of tests/test_training_glue.py::test_compute_loss_two_terms_value_and_gradients with that test's checker and
    tolerances, and the bits of its resized target with and without the autograd path"""
    dev = _gpu()
    from vsrlab_amd.core.losses import CharbonnierLoss
    from vsrlab_amd.core.utils import compute_loss, resize
    sr = rand(1, 1, 2, 3, 64, 96).requires_grad_(True)
    hr = rand(2, 1, 2, 3, 64, 96)
    lq = rand(3, 1, 2, 3, 16, 24).requires_grad_(True)
    want = O.charbonnier(sr, hr) + O.charbonnier(lq, LC.interp(hr, (16, 24)))
    want.backward()
    sr_d = sr.detach().to(dev).requires_grad_(True)
    lq_d = lq.detach().to(dev).requires_grad_(True)
    got = compute_loss(CharbonnierLoss(), sr_d, hr.to(dev), lq_d)
    got.backward()
    assert abs(float(got.detach()) - float(want.detach())) < 1e-5 * float(want.detach())
    assert rel_err(sr_d.grad.cpu(), sr.grad) < 1e-5 and rel_err(lq_d.grad.cpu(), lq.grad) < 1e-5
    again = compute_loss(CharbonnierLoss(), sr_d.detach().requires_grad_(True), hr.to(dev), lq_d.detach().requires_grad_(True))
    assert torch.equal(again.detach(), got.detach())
    with torch.no_grad():
        tgt = resize(hr.to(dev), (16, 24))
    assert torch.equal(resize(hr.to(dev).requires_grad_(True), (16, 24)).detach(), tgt)
