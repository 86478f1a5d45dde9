"""GPU tests of the HIP VGG19 perceptual loss (csrc/perceptual_engine.hip) against the reference's fp64 golden
(tests/golden/perceptual_loss.npz), an fp64 pure-torch restatement (tests/perceptual_common.py) and, in bf16, the restatement
that rounds to bf16 where the build stores (noise-floor criterion of test_hip_parity.py: error <= 1.5 x that oracle's).

d sr goes through sign(f_k(sr) - f_k(hr)), which flips wherever |d| is below the fp32 error of the features.  In the golden case
tap '25' (2 x 512 x 5 x 9 values) has such a near-tie: image 1, channel 222, pixel (3, 0), f(sr) = 0.7545706 and f(hr) = 0.7545714,
|d| = 8e-7, i.e. 1e-6 of the value, within the accumulated fp32 rounding of twelve convolutions; every other element of the tap
cotangent matches fp64.  That one element moves d sr by 2 * scale * J^T e = 1.8e-3 rel-L2 (one element of a 46,080-value tap:
~2 / sqrt(numel) of the tap's share); the loss and the terms are unaffected (~1e-7).  The d sr bound at fp32 is therefore 1e-2."""
DSR_FP32 = 1e-2
import pytest
import torch

from helpers import golden, rand, rel_err, rel_l2
from perceptual_common import keyed_vgg_state_dict, param_list, perceptual_terms

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _params(dev):
    return [p.to(dev) for p in param_list(keyed_vgg_state_dict())]


def _run(sr, hr, params, dtype, weight=1.0, **kw):
    from vsrlab_amd import functional as VF
    x = sr.detach().clone().requires_grad_(True)
    loss, terms = VF.perceptual_loss(x, hr, params, weight, compute_dtype=dtype, return_terms=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), terms, x.grad


def _oracle(sr, hr, weight=1.0, store=None):
    x = sr.detach().double().cpu().requires_grad_(True)
    sd = keyed_vgg_state_dict(dtype=torch.float64)
    if store is not None:
        sd = {k: store(v) for k, v in sd.items()}
        x_in = store(x)
    else:
        x_in = x
    terms = perceptual_terms(x_in, store(hr.double().cpu()) if store else hr.double().cpu(), param_list(sd), weight, store)
    terms.sum().backward()
    return terms.sum().detach(), terms.detach(), x.grad


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def test_fp32_matches_the_reference_golden():
    dev = _gpu()
    z = golden("perceptual_loss")
    shape = tuple(int(s) for s in z["shape"])
    sr, hr = rand(int(z["seed_sr"]), *shape).to(dev), rand(int(z["seed_hr"]), *shape).to(dev)
    loss, terms, dsr = _run(sr, hr, _params(dev), "fp32")
    e = (rel_err(loss, z["loss"]), rel_err(terms, z["terms"]), rel_l2(dsr, z["dsr"]))
    print("fp32 vs golden: loss %.2e terms %.2e dsr %.2e" % e)
    assert e[0] <= 1e-3 and e[1] <= 1e-3 and e[2] <= DSR_FP32, e
    assert dsr.shape == sr.shape


def test_fp32_matches_the_fp64_restatement_at_a_second_shape():
    dev = _gpu()
    sr, hr = rand(81, 2, 3, 3, 48, 80).to(dev), rand(82, 2, 3, 3, 48, 80).to(dev)
    loss, terms, dsr = _run(sr, hr, _params(dev), "fp32", weight=1e-2)
    l64, t64, g64 = _oracle(sr, hr, 1e-2)
    e = (rel_err(loss, l64), rel_err(terms, t64), rel_l2(dsr, g64))
    print("fp32 vs fp64 restatement: loss %.2e terms %.2e dsr %.2e" % e)
    assert e[0] <= 1e-3 and e[1] <= 1e-3 and e[2] <= DSR_FP32, e


def test_bf16_meets_the_noise_floor():
    dev = _gpu()
    z = golden("perceptual_loss")
    shape = tuple(int(s) for s in z["shape"])
    sr, hr = rand(int(z["seed_sr"]), *shape).to(dev), rand(int(z["seed_hr"]), *shape).to(dev)
    loss, terms, dsr = _run(sr, hr, _params(dev), "bf16")
    le, te, ge = _oracle(sr, hr, store=_bf16)
    ref_l, ref_t, ref_g = torch.as_tensor(z["loss"]), torch.as_tensor(z["terms"]), torch.as_tensor(z["dsr"])
    ours = (rel_err(loss, ref_l), rel_err(terms, ref_t), rel_l2(dsr, ref_g))
    emu = (rel_err(le, ref_l), rel_err(te, ref_t), rel_l2(ge, ref_g))
    print("bf16: ours loss %.2e terms %.2e dsr %.2e | bf16-storage oracle %.2e %.2e %.2e" % (ours + emu))
    floors = (1e-3, 1e-3, 1e-2)
    for o, m, f in zip(ours, emu, floors):
        assert o <= 1.5 * max(m, f), (ours, emu)


def test_deterministic_across_calls_and_chunk_sizes():
    from vsrlab_amd import functional as VF
    dev = _gpu()
    params = _params(dev)
    sr, hr = rand(91, 2, 3, 3, 40, 72).to(dev), rand(92, 2, 3, 3, 40, 72).to(dev)
    for dtype in ("fp32", "bf16"):
        dt = VF.resolve_dtype(dtype)
        one = VF.perceptual_workspace_bytes(1, 40, 72, dt)
        per = VF.perceptual_workspace_bytes(2, 40, 72, dt) - one
        runs = [_run(sr, hr, params, dtype)]
        runs.append(_run(sr, hr, params, dtype))
        for chunk in (1, 2, 6):
            assert VF.perceptual_chunk(6, 40, 72, dt, True, one + (chunk - 1) * per) == chunk
            runs.append(_run(sr, hr, params, dtype, max_workspace_bytes=one + (chunk - 1) * per))
        for loss, terms, dsr in runs[1:]:
            assert torch.equal(loss, runs[0][0]) and torch.equal(terms, runs[0][1]) and torch.equal(dsr, runs[0][2]), dtype


def test_backward_scales_and_no_grad_forward_gives_the_same_bits():
    from vsrlab_amd import functional as VF
    dev = _gpu()
    params = _params(dev)
    sr, hr = rand(93, 1, 2, 3, 40, 72).to(dev), rand(94, 1, 2, 3, 40, 72).to(dev)
    loss, _, g1 = _run(sr, hr, params, "fp32")
    x = sr.clone().requires_grad_(True)
    (3 * VF.perceptual_loss(x, hr, params, compute_dtype="fp32")).backward()
    assert torch.equal(x.grad, 3 * g1)
    with torch.no_grad():
        l2 = VF.perceptual_loss(sr, hr, params, compute_dtype="fp32")
    assert torch.equal(l2, loss)
    # no second backward, no double backward
    x = sr.clone().requires_grad_(True)
    lx = VF.perceptual_loss(x, hr, params, compute_dtype="fp32")
    lx.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        lx.backward()
    x = sr.clone().requires_grad_(True)
    lx = VF.perceptual_loss(x, hr, params, compute_dtype="fp32")
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(lx, x, create_graph=True)


def test_generator_step_with_perceptual_loss():
    """generator_step (train_gan.py) with the reference's gan.yaml perceptual term: the term equals a standalone call (under
    the same autocast, hence bf16), and the generator's gradients differ from a dummy_loss run."""
    from vsrlab_amd.core.losses import AdversarialLoss, CharbonnierLoss, PerceptualLoss
    from vsrlab_amd.train_gan import dummy_loss, generator_step
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.unet_discriminator import UNetDiscriminator
    from vsrlab_amd.vsr.models.RealBasicVSR.realbasicvsr import RealBasicVSR
    dev = _gpu()
    torch.manual_seed(0)
    g = RealBasicVSR(2, mid_channels=64, upscale=4, res_blocks=2, pretrained_flow=False, train_flow=False).to(dev)
    d = UNetDiscriminator(3, 64).to(dev).train()
    perc = PerceptualLoss(1e-2, vgg_weights=keyed_vgg_state_dict()).to(dev)
    lr, hr = rand(95, 1, 2, 3, 16, 24).to(dev), rand(96, 1, 2, 3, 64, 96).to(dev)
    adv, crit = AdversarialLoss(), CharbonnierLoss()
    grads = []
    for ploss in (perc, dummy_loss):
        g.zero_grad()
        sr, loss, perceptual_g, _ = generator_step(g, d, crit, ploss, adv, lr, hr)
        loss.backward()
        grads.append(torch.cat([p.grad.flatten() for p in g.parameters() if p.grad is not None]))
        if ploss is perc:
            with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
                alone = perc(sr.detach(), hr)
            assert torch.equal(perceptual_g.detach(), alone) and float(perceptual_g) > 0
    assert grads[0].shape == grads[1].shape and not torch.equal(grads[0], grads[1])
    assert bool(torch.isfinite(grads[0]).all())


def test_bf16_full_size_frame():
    """One bf16 call at 2160x3840 x 2 frames: finite, within 1e-2 of stock PyTorch fp32 on the same GPU, and the peak allocation
    stays within the workspace budget plus d sr."""
    from vsrlab_amd import functional as VF
    import gc
    dev = _gpu()
    gc.collect()
    torch.cuda.empty_cache()
    params = _params(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    sr = torch.rand(1, 2, 3, 2160, 3840, device=dev, generator=g)
    hr = torch.rand(1, 2, 3, 2160, 3840, device=dev, generator=g)
    budget = 12 << 30
    x = sr.clone().requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = VF.perceptual_loss(x, hr, params, compute_dtype="bf16", max_workspace_bytes=budget)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())
    dsr_bytes = sr.numel() * 4
    assert peak <= budget + dsr_bytes, (peak, budget, dsr_bytes)
    del x
    with torch.no_grad():
        ref = sum(float(t) for t in perceptual_terms(sr.reshape(-1, 3, 2160, 3840), hr.reshape(-1, 3, 2160, 3840), params))
    print(f"2160x3840 x2 bf16: loss {float(loss):.6f}, stock fp32 {ref:.6f}, peak {peak / 2**30:.2f} GiB")
    assert abs(float(loss) - ref) <= 1e-2 * abs(ref)
