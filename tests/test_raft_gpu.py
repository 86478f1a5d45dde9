"""GPU checks of the fused correlation lookup (csrc/raft_corr.hip), of RAFT-small and of OpticalFlowConsistency on top of it,
against the fp64 restatements of tests/raft_common.py (pinned to the reference by tests/test_raft_host.py)."""
import os

import numpy as np
import pytest
import torch

import raft_common as RC
from helpers import GOLDEN, bf16_store, rel_err, rel_l2, sub_stride

pytestmark = pytest.mark.gpu

CASES = {"17x23-L4": (2, 17, 23, 4), "17x23-L2": (2, 17, 23, 2), "16x16-L4": (1, 16, 16, 4), "16x16-L2": (1, 16, 16, 2)}


def _dev():
    return torch.device("cuda:0")


def _inputs(case, dtype=torch.float64):
    n, h, w, L = CASES[case]
    f1, f2, coords, cot = RC.lookup_inputs(n, h, w, dtype=dtype)
    return f1, f2, coords, cot[:, :L * RC.TAPS].contiguous(), L


def _restate(case, store=None, dtype=torch.float64):
    f1, f2, coords, cot, L = _inputs(case, dtype)
    f1.requires_grad_(True), f2.requires_grad_(True)
    out = RC.corr_lookup_ref(coords, f1, f2, L, store=store)
    (out * cot).sum().backward()
    return out.detach(), f1.grad, f2.grad


@pytest.fixture(scope="module")
def oracle():
    """per case: the fp64 restatement and its bf16-storage twin (out, d fmap1, d fmap2), computed once"""
    return {case: (_restate(case), _restate(case, store=bf16_store)) for case in CASES}


def _hip(case, compute_dtype, one_shot=False, grad=True):
    from vsrlab_amd import functional as VF
    f1, f2, coords, cot, L = (t.to(_dev()) if torch.is_tensor(t) else t for t in _inputs(case, torch.float32))
    if not grad:
        with torch.no_grad():
            return VF.raft_corr_lookup(VF.raft_corr_pyramid(f1, f2, L, compute_dtype), coords), None, None
    f1.requires_grad_(True), f2.requires_grad_(True)
    if one_shot:
        out = VF.raft_correlation(coords, f1, f2, num_levels=L, radius=3, compute_dtype=compute_dtype)
    else:
        out = VF.raft_corr_lookup(VF.raft_corr_pyramid(f1, f2, L, compute_dtype), coords)
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), f1.grad, f2.grad


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_lookup_against_the_fp64_restatement(case, oracle):
    (o, d1, d2), _ = oracle[case]
    out, g1, g2 = _hip(case, "fp32")
    e = rel_err(out, o), rel_l2(g1, d1), rel_l2(g2, d2)
    print(f"{case} fp32: out max-rel {e[0]:.3e}, d fmap1 rel-L2 {e[1]:.3e}, d fmap2 rel-L2 {e[2]:.3e}")
    assert max(e) < 1e-3, e


@pytest.mark.parametrize("case", list(CASES))
def test_bf16_lookup_is_at_the_noise_floor_of_bf16_storage(case, oracle):
    (o, d1, d2), (oe, d1e, d2e) = oracle[case]
    out, g1, g2 = _hip(case, "bf16")
    e = rel_err(out, o), rel_l2(g1, d1), rel_l2(g2, d2)
    floor = rel_err(oe, o), rel_l2(d1e, d1), rel_l2(d2e, d2)
    print(f"{case} bf16: out max-rel {e[0]:.3e} (restatement {floor[0]:.3e}), d fmap1 rel-L2 {e[1]:.3e} ({floor[1]:.3e}), "
          f"d fmap2 rel-L2 {e[2]:.3e} ({floor[2]:.3e})")
    for got, fl in zip(e, floor):
        assert got <= 1.5 * max(fl, 1e-3), (e, floor)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_one_shot_equals_pyramid_plus_lookup_bit_for_bit(dt):
    a, b = _hip("17x23-L4", dt), _hip("17x23-L4", dt, one_shot=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert rel_l2(a[2], b[2]) < 1e-6


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_repeatability_and_no_grad(dt):
    a, b = _hip("17x23-L4", dt), _hip("17x23-L4", dt)
    assert torch.equal(a[0], b[0]), "forward differs between two runs"
    assert torch.equal(a[1], b[1]), "d fmap1 (a gather) differs between two runs"
    e = rel_l2(a[2], b[2])
    print(f"d fmap2 (fp32 atomic adds) between two runs: rel-L2 {e:.3e}")
    assert e < 1e-6
    assert torch.equal(_hip("17x23-L4", dt, grad=False)[0], a[0]), "no_grad changes the forward's bits"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_far_and_outside_windows_are_exactly_zero(dt):
    n, h, w, L = CASES["17x23-L4"]
    out = _hip("17x23-L4", dt, grad=False)[0]
    assert bool(torch.isfinite(out).all())
    for (y, x) in RC.far_points(h, w):
        assert float(out[:, :, y, x].abs().max()) == 0.0
    top, bottom = RC.outside_rows(h)
    assert float(out[:, :RC.TAPS, top].abs().max()) == 0.0 and float(out[:, :RC.TAPS, bottom].abs().max()) == 0.0
    assert float(out[:, :RC.TAPS, 5].abs().max()) > 0.0


def test_channel_order_is_the_references():
    """only target pixel (tx, ty) of fmap2 is non-zero; a query centred at (tx - 2, ty + 1) meets it at window offset
    (+2, -1) in (x, y): i = 5 (x, slow), j = 2 (y, fast), channel 5 * 7 + 2 of level 0"""
    from vsrlab_amd import functional as VF
    h, w, tx, ty = 16, 20, 9, 6
    f1 = torch.ones(1, 128, h, w, device=_dev())
    f2 = torch.zeros(1, 128, h, w, device=_dev())
    f2[:, :, ty, tx] = 1.0
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords = torch.stack([xs, ys])[None].to(_dev())
    out = VF.raft_correlation(coords, f1, f2, num_levels=1)
    win = out[0, :, ty + 1, tx - 2]
    assert int(win.argmax()) == 5 * 7 + 2 and int((win != 0).sum()) == 1
    assert abs(float(win.max()) - 128 / float(np.sqrt(np.float32(128)))) < 1e-4
    assert int(out[0, :, ty - 2, tx + 1].argmax()) == 2 * 7 + 5


def test_peak_memory_has_no_room_for_a_volume():
    """(1, 128, 135, 240): the packed maps + the output (25 MB) + 64 MiB of allocator slack; the volume alone is 4.2 GB"""
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    n, h, w = 1, 135, 240
    g = torch.Generator(device=_dev()).manual_seed(3)
    f1 = torch.randn(n, 128, h, w, device=_dev(), generator=g).requires_grad_(True)
    f2 = torch.randn(n, 128, h, w, device=_dev(), generator=g).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords = torch.stack([xs, ys])[None].to(_dev()) + 1.25
    packed = VF.raft_corr_workspace_bytes(f1.shape, 4, 3, _lib.DT_F32)
    out_bytes = n * 4 * RC.TAPS * h * w * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pyr = VF.raft_corr_pyramid(f1, f2, 4, "fp32")
    out = VF.raft_corr_lookup(pyr, coords)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak / 2**20:.1f} MiB: packed maps {packed / 2**20:.1f} MiB, output {out_bytes / 2**20:.1f} MiB")
    assert pyr.packed_bytes == packed and out.shape == (n, 196, h, w)
    assert peak <= packed + out_bytes + (64 << 20)
    assert (h * w) ** 2 * 4 > 4.1e9


# ---- RAFT-small and the loss ---------------------------------------------------------------------------------------------------
def _golden_sub(z, tag, key, value):
    v = value.detach().double().cpu()
    return rel_err(v.flatten()[::sub_stride(v.numel())], torch.from_numpy(z[f"{tag}__sub__{key}"]))


@pytest.fixture(scope="module")
def raft_oracle():
    """golden (b) and (c) through the restatement: fp64 (checked against the stored golden), fp32 and fp32 + bf16 storage"""
    z = np.load(os.path.join(GOLDEN, "raft.npz"), allow_pickle=False)
    schema = RC.load_schema()

    def model(dtype, store):
        sd = RC.raft_state_dict(schema, dtype)
        ref, supp, cot = RC.raft_inputs(dtype)
        ref.requires_grad_(True), supp.requires_grad_(True)
        up = RC.raft_small_ref(sd, ref, supp, store=store)
        (up * cot).mean().backward()
        return up.detach(), ref.grad, supp.grad

    def loss(dtype, store):
        sd = RC.raft_state_dict(schema, dtype)
        sr, hr = RC.loss_inputs(dtype)
        sr.requires_grad_(True)
        v = RC.flow_consistency_ref(sd, sr, hr, store=store)
        v.backward()
        return v.detach(), sr.grad

    b64, c64 = model(torch.float64, None), loss(torch.float64, None)
    assert _golden_sub(z, "b", "flow_up", b64[0]) < 1e-6 and _golden_sub(z, "b", "dref", b64[1]) < 1e-6
    assert abs(float(c64[0]) / float(z["c__loss"]) - 1) < 1e-6 and _golden_sub(z, "c", "dsr", c64[1]) < 1e-6
    return {"b": {None: b64, "fp32": model(torch.float32, None), "bf16": model(torch.float32, bf16_store)},
            "c": {None: c64, "fp32": loss(torch.float32, None), "bf16": loss(torch.float32, bf16_store)}}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_raft_small_end_to_end_against_the_golden(dt, raft_oracle):
    from vsrlab_amd.optical_flow.models.raft.raft import RAFT
    m = RAFT(small=True, scale_factor=8, weights=RC.raft_state_dict(RC.load_schema(), torch.float32), compute_dtype=dt).to(_dev())
    ref, supp, cot = (t.to(_dev()) for t in RC.raft_inputs(torch.float32))
    ref.requires_grad_(True), supp.requires_grad_(True)
    up = m(ref, supp)
    (up * cot).mean().backward()
    torch.cuda.synchronize()
    o, cpu = raft_oracle["b"][None], raft_oracle["b"][dt]
    e = rel_err(up, o[0]), rel_l2(ref.grad, o[1]), rel_l2(supp.grad, o[2])
    c = rel_err(cpu[0], o[0]), rel_l2(cpu[1], o[1]), rel_l2(cpu[2], o[2])
    print(f"RAFT-small {dt}: flow_up max-rel {e[0]:.3e} (CPU {c[0]:.3e}), d ref rel-L2 {e[1]:.3e} ({c[1]:.3e}), d supp rel-L2 {e[2]:.3e} ({c[2]:.3e})")
    assert e[0] <= 1.5 * max(c[0], 1e-3), (e, c)
    assert e[1] <= 1.5 * max(c[1], 2e-4) and e[2] <= 1.5 * max(c[2], 2e-4), (e, c)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_flow_consistency_loss_against_the_golden(dt, raft_oracle):
    from vsrlab_amd.core.losses import OpticalFlowConsistency
    loss = OpticalFlowConsistency(weight=1.0, weights=RC.raft_state_dict(RC.load_schema(), torch.float32), compute_dtype=dt).to(_dev())
    sr, hr = (t.to(_dev()) for t in RC.loss_inputs(torch.float32))
    sr.requires_grad_(True)
    v = loss(sr, hr)
    v.backward()
    torch.cuda.synchronize()
    o, cpu = raft_oracle["c"][None], raft_oracle["c"][dt]
    e = abs(float(v) / float(o[0]) - 1), rel_l2(sr.grad, o[1])
    c = abs(float(cpu[0]) / float(o[0]) - 1), rel_l2(cpu[1], o[1])
    print(f"OpticalFlowConsistency {dt}: value rel {e[0]:.3e} (CPU {c[0]:.3e}), d sr rel-L2 {e[1]:.3e} ({c[1]:.3e})")
    assert e[0] <= 1.5 * max(c[0], 1e-3) and e[1] <= 1.5 * max(c[1], 2e-4), (e, c)
    assert all(p.grad is None for p in loss.parameters())


def test_autograd_contract():
    from vsrlab_amd import functional as VF
    f1, f2, coords, cot, L = (t.to(_dev()) if torch.is_tensor(t) else t for t in _inputs("16x16-L2", torch.float32))
    f1.requires_grad_(True), f2.requires_grad_(True)
    out = VF.raft_correlation(coords, f1, f2, num_levels=L)
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad((out * cot).sum(), f1, create_graph=True)
    out = VF.raft_correlation(coords, f1, f2, num_levels=L)
    (out * cot).sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a second time"):
        (out * cot).sum().backward()
    for shape, kw in (((1, 128, 15, 16), dict(num_levels=4)), ((1, 64, 16, 16), dict(num_levels=4)), ((1, 128, 16, 16), dict(num_levels=4, radius=4))):
        z = torch.zeros(shape, device=_dev())
        with pytest.raises(RuntimeError, match="unsupported shape"):
            VF.raft_correlation(torch.zeros(shape[0], 2, shape[2], shape[3], device=_dev()), z, z, **kw)


def test_one_lookup_at_the_benchmark_size_in_bf16():
    """(1, 128, 270, 480): 1/8 of 2160 x 3840, where the all-pairs volume would be 67 GB"""
    from vsrlab_amd import functional as VF
    h, w = 270, 480
    g = torch.Generator(device=_dev()).manual_seed(7)
    f1 = torch.randn(1, 128, h, w, device=_dev(), generator=g).requires_grad_(True)
    f2 = torch.randn(1, 128, h, w, device=_dev(), generator=g).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords = torch.stack([xs, ys])[None].to(_dev()) + (torch.rand(1, 2, h, w, device=_dev(), generator=g) * 8 - 4)
    out = VF.raft_correlation(coords, f1, f2, compute_dtype="bf16")
    out.square().mean().backward()
    torch.cuda.synchronize()
    for t in (out, f1.grad, f2.grad):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
