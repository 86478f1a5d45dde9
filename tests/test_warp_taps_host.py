"""CPU checks of the integer-tap warps (functional.flow_warp 'nearest' / 'nearest4', functional.aligned_input,
vsr/models/VRT/vrt.py): the numpy oracle of tests/warp_taps_common.py against the reference's recorded results, bit for bit; the
library's exports and its argument checks (every entry refuses bad arguments before it touches the GPU); the Python surface's
call forms and refusals; get_flows against a stub flow network.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import warp_taps_common as WT
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(4, "nearest4"), (1, "nearest")]


@pytest.fixture(scope="module")
def gold():
    return golden("warp_taps")


def test_the_golden_covers_the_case_table(gold):
    want = set()
    for name in WT.CASES:
        for _, mode in MODES:
            want |= {f"{name}__{mode}", f"{name}__{mode}_gx", f"{name}__{mode}_gflow_absmax"}
            if name in WT.BORDER_GOLDEN:
                want.add(f"{name}__{mode}_border")
    for clip in WT.CLIP_GOLDEN:
        want |= {WT.clip_name(*clip) + "__backward", WT.clip_name(*clip) + "__forward"}
    assert set(gold) == want
    assert set(WT.CLIP_GOLDEN) <= set(WT.CLIP_CASES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "warp_taps.npz")) < 512 * 1024


@pytest.mark.parametrize("taps,mode", MODES)
@pytest.mark.parametrize("name", list(WT.CASES))
def test_oracle_equals_the_reference_exactly(name, taps, mode, gold):
    x, flow = WT.case_x(name), WT.case_flow(name, taps)
    out = WT.warp(x, flow, taps)
    assert out.shape == (x.shape[0], taps * x.shape[1]) + tuple(x.shape[2:])
    assert np.array_equal(out.numpy(), gold[f"{name}__{mode}"].numpy())
    if name in WT.BORDER_GOLDEN:
        assert np.array_equal(WT.warp(x, flow, taps, border=True).numpy(), gold[f"{name}__{mode}_border"].numpy())
    gx = WT.warp_grad(WT.grid_cotangent(f"{name}:{mode}", out.shape), flow, taps)
    assert gx.dtype == torch.float64 and np.array_equal(gx.numpy(), gold[f"{name}__{mode}_gx"].numpy().astype(np.float64))
    assert float(gold[f"{name}__{mode}_gflow_absmax"]) == 0.0, "the reference's flow gradient is a zeros tensor"


def test_the_cases_catch_what_they_are_for():
    inframe = lambda name, taps: float(np.mean([v.mean() for v, _, _ in WT.tap_indices(WT.case_flow(name, taps), taps)]))
    assert inframe("odd", 4) < 0.45 and inframe("wide", 4) > 0.6
    for name in ("integer", "edge", "far"):
        assert 0.2 < inframe(name, 4) < 0.8
    taps = WT.tap_indices(WT.case_flow("integer", 4), 4)
    assert all(np.array_equal(taps[0][j], taps[k][j]) for k in range(1, 4) for j in range(3)), "floor == ceil: four equal taps"
    _, cnt, _ = WT.warp_grad(torch.ones(1, 12, 6, 10), WT.case_flow("integer", 4), 4, stats=True)
    assert cnt.max() >= 8 and (cnt % 4 == 0).all()
    far = WT.case_flow("far", 4)
    assert far.abs().max() > 2 ** 31 and any(v.any() for v, _, _ in WT.tap_indices(far, 4))
    for name in WT.CASES:                                                           # 'nearest': no position near a tie
        flow = WT.case_flow(name, 1)
        frac = (flow - torch.floor(flow))[flow.abs() < 100]
        assert ((frac - 0.5).abs() > 0.04).all()
    nan = torch.full((1, 2, 3, 4), float("nan"))
    inf = torch.full((1, 2, 3, 4), float("inf"))
    for bad in (nan, inf, -inf):
        assert not any(v.any() for v, _, _ in WT.tap_indices(bad, 4)) and not WT.warp(torch.ones(1, 1, 3, 4), bad, 1).any()


@pytest.mark.parametrize("clip", WT.CLIP_GOLDEN, ids=lambda c: WT.clip_name(*c))
def test_aligned_input_oracle_equals_the_reference(clip, gold):
    x, fb, ff = WT.clip_inputs(*clip)
    name = WT.clip_name(*clip)
    want = torch.cat([x, gold[name + "__backward"], gold[name + "__forward"]], 2)
    assert np.array_equal(WT.aligned_input(x, fb, ff).numpy(), want.numpy())


def test_aligned_input_gradient_is_the_identity_plus_both_scatters():
    """the clip oracle's gradient against torch autograd through the pair oracle's own gather indices (fp64, exact cotangents)"""
    b, d, f = 2, 3, (3, 6, 10)
    x, fb, ff = WT.clip_inputs(b, d, f)
    cot = WT.grid_cotangent("clip-host", (b, d, 27, 6, 10))
    leaf = x.double().requires_grad_(True)
    parts = [leaf]
    for flows, src, shift in ((fb, range(1, d), -1), (ff, range(0, d - 1), 1)):
        frames = [torch.zeros(b, 12, 6, 10, dtype=torch.float64)] * d
        for i in src:
            fl = flows[:, i - 1] if shift < 0 else flows[:, i]
            taps = []
            for valid, iy, ix in WT.tap_indices(fl, 4):
                got = leaf[:, i][torch.arange(b)[:, None, None], :, torch.from_numpy(iy), torch.from_numpy(ix)]
                taps.append((got * torch.from_numpy(valid)[..., None]).permute(0, 3, 1, 2))
            frames[i + shift] = torch.cat(taps, 1)
        parts.append(torch.stack(frames, 1))
    out = torch.cat(parts, 2)
    assert torch.equal(out.detach().float(), WT.aligned_input(x, fb, ff))
    out.backward(cot.double())
    gx, cnt, mag = WT.aligned_input_grad(cot, fb, ff, stats=True)
    assert torch.equal(gx, leaf.grad) and cnt.min() >= 1 and (mag >= gx.abs()).all()


def test_library_exports():
    """the entry points live in a library of their own, which exports what its header declares and nothing else"""
    from vsrlab_amd import _lib
    lib = _lib.load_warp_taps()
    names = {"vsr_warp_taps_fwd", "vsr_warp_taps_bwd", "vsr_warp_taps_clip_fwd", "vsr_warp_taps_clip_bwd"}
    assert set(_lib.WARP_TAPS_EXPORTS) == names and not names & set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "vsrlab_warp_taps.h")).read()
    assert set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header)) == names
    from test_hr_tail_host import _exported_vsr_symbols          # the dynamic symbol table, read from the ELF file
    assert _exported_vsr_symbols(_lib.WARP_TAPS_LIB_PATH) == names
    assert not any(hasattr(_lib.load(), n) for n in names)
    assert all(hasattr(lib, n) for n in names)


def test_every_entry_rejects_bad_arguments_before_touching_the_gpu():
    from vsrlab_amd import _lib
    lib = _lib.load_warp_taps()
    BADARG, UNSUPPORTED = -1, -2
    mk = lambda N=1, D=3, C=3, H=8, W=8, taps=4, border=0, dtype=0, xs=0: _lib.WarpTapsDesc(N, D, C, H, W, taps, border, dtype, xs)
    one = ctypes.c_void_p(256)                                    # a non-null pointer that is never dereferenced: every call below is refused
    entries = {
        "fwd": lambda d, p=one: lib.vsr_warp_taps_fwd(d, p, p, p, None),
        "bwd": lambda d, p=one: lib.vsr_warp_taps_bwd(d, p, p, p, ctypes.c_void_p(512), None),
        "clip_fwd": lambda d, p=one: lib.vsr_warp_taps_clip_fwd(d, p, p, p, p, None),
        "clip_bwd": lambda d, p=one: lib.vsr_warp_taps_clip_bwd(d, p, p, p, p, ctypes.c_void_p(512), None),
    }
    for name, call in entries.items():
        assert call(None) == BADARG, name                                            # no descriptor
        assert call(mk(), None) == BADARG, name                                      # null pointers
        for bad in (mk(H=1), mk(W=1), mk(H=1, W=1)):
            assert call(bad) == UNSUPPORTED, name                                    # extent 1: the reference reads index 0 for every tap
        for bad in (mk(H=0), mk(W=-3), mk(N=0), mk(C=0)):
            assert call(bad) == BADARG, name
        for taps in (0, 2, 3, 5, -1):
            assert call(mk(taps=taps)) == BADARG, (name, taps)
        for dtype in (2, -1, 7):
            assert call(mk(dtype=dtype)) == UNSUPPORTED, (name, dtype)
        assert call(mk(xs=-1)) == BADARG, name
        assert call(mk(H=(1 << 24) + 1)) == UNSUPPORTED and call(mk(H=1 << 16, W=1 << 16)) == UNSUPPORTED, name
    for name in ("clip_fwd", "clip_bwd"):
        for d in (1, 0, -2):
            assert entries[name](mk(D=d)) == BADARG, (name, d)                       # a clip has at least one pair
        assert entries[name](mk(taps=1)) == BADARG and entries[name](mk(xs=640)) == BADARG
    # each null pointer on its own
    d = mk()
    assert lib.vsr_warp_taps_fwd(d, None, one, one, None) == lib.vsr_warp_taps_fwd(d, one, None, one, None) == BADARG
    assert lib.vsr_warp_taps_fwd(d, one, one, None, None) == BADARG
    assert lib.vsr_warp_taps_bwd(d, one, one, None, one, None) == lib.vsr_warp_taps_bwd(d, one, one, one, None, None) == BADARG
    assert lib.vsr_warp_taps_clip_fwd(d, one, one, None, one, None) == lib.vsr_warp_taps_clip_bwd(d, one, one, None, one, one, None) == BADARG
    # a bf16 gradient is rounded from the fp32 accumulator: the two cannot be one buffer
    assert lib.vsr_warp_taps_bwd(mk(dtype=1), one, one, one, one, None) == BADARG
    assert lib.vsr_warp_taps_clip_bwd(mk(dtype=1), one, one, one, one, one, None) == BADARG


def test_flow_warp_call_forms_and_refusals():
    """the reference's positional and keyword forms reach the HIP path (which refuses a CPU tensor: there is no fallback), and what is
    not provided raises NotImplementedError before anything else"""
    from vsrlab_amd import functional as VF
    from vsrlab_amd.vsr.models.VRT.modules.spynet import flow_warp
    x, flow = torch.rand(1, 3, 4, 6), torch.zeros(1, 4, 6, 2)
    for call in (lambda: flow_warp(x, flow, "nearest4"), lambda: flow_warp(x, flow, interp_mode="nearest4"),
                 lambda: flow_warp(x, flow, "nearest", "border", True), lambda: flow_warp(x, flow, interp_mode="nearest", padding_mode="zeros"),
                 lambda: flow_warp(x, flow.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), "nearest4"),
                 lambda: VF.flow_warp(x, flow, "nearest4"), lambda: VF.flow_warp(x, flow, interpolation="nearest", align_corners=True),
                 lambda: flow_warp(x, flow), lambda: flow_warp(x, flow, "bilinear", "border")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for mode in ("nearest", "nearest4", "bilinear"):
        with pytest.raises(NotImplementedError):
            flow_warp(x, flow, mode, "reflection")
        with pytest.raises(NotImplementedError):
            flow_warp(x, flow, mode, "zeros", False)
        with pytest.raises(NotImplementedError):
            VF.flow_warp(x, flow, interpolation=mode, align_corners=False)
    with pytest.raises(NotImplementedError):
        flow_warp(x, flow, "bicubic")
    for shape in ((1, 3, 1, 6), (1, 3, 4, 1), (1, 3, 1, 1)):
        with pytest.raises(NotImplementedError, match="at least 2"):
            flow_warp(torch.rand(shape), torch.zeros(shape[0], shape[2], shape[3], 2), "nearest4")
    with pytest.raises(ValueError):
        flow_warp(x, torch.zeros(1, 2, 4, 6), "nearest4")                            # a planar flow is not the reference's form
    with pytest.raises(ValueError):
        flow_warp(x.half(), flow, "nearest")


def test_aligned_input_validation():
    from vsrlab_amd.vsr.models.VRT import vrt
    x, f = torch.rand(1, 3, 3, 4, 6), torch.zeros(1, 2, 2, 4, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vrt.aligned_input(x, f, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vrt.get_aligned_image(x, f, f)
    with pytest.raises(ValueError):
        vrt.aligned_input(x[:, :1], f[:, :0], f[:, :0])                              # D < 2
    with pytest.raises(ValueError):
        vrt.aligned_input(x, f, f[:, :1])
    with pytest.raises(ValueError):
        vrt.aligned_input(x[0], f[0], f[0])
    with pytest.raises(NotImplementedError, match="at least 2"):
        vrt.aligned_input(torch.rand(1, 2, 3, 1, 6), torch.zeros(1, 1, 2, 1, 6), torch.zeros(1, 1, 2, 1, 6))


class _StubFlow:
    """a flow network's interface: ``return_levels`` and a call on two (B (D - 1), C, H, W) batches that returns one
    (B (D - 1), 2, H / 2^i, W / 2^i) tensor per level, here a function of the frames that tells the two apart"""

    def __init__(self, levels):
        self.return_levels = levels
        self.calls = []

    def __call__(self, ref, supp):
        self.calls.append((ref.clone(), supp.clone()))
        base = torch.stack([ref.mean(1), supp.mean(1) * 2], 1)
        flows = [torch.nn.functional.avg_pool2d(base, 2 ** i) for i in range(len(self.return_levels))]
        return flows if len(flows) > 1 else flows[0]


@pytest.mark.parametrize("levels", [[3, 4, 5], [5]])
def test_get_flows_views_and_frame_order(levels):
    from vsrlab_amd.vsr.models.VRT import vrt
    b, n, c, h, w = 2, 4, 3, 8, 16
    x = torch.rand(b, n, c, h, w, generator=torch.Generator().manual_seed(5))
    net = _StubFlow(levels)
    fbs, ffs = vrt.get_flows(net, x)
    x1, x2 = x[:, :-1].reshape(-1, c, h, w), x[:, 1:].reshape(-1, c, h, w)
    assert len(net.calls) == 2
    assert torch.equal(net.calls[0][0], x1) and torch.equal(net.calls[0][1], x2), "backward: optical_flow(x_1, x_2) (vrt.py:199)"
    assert torch.equal(net.calls[1][0], x2) and torch.equal(net.calls[1][1], x1), "forward: optical_flow(x_2, x_1) (vrt.py:204)"
    assert len(fbs) == len(ffs) == len(levels)
    for i, (fb, ff) in enumerate(zip(fbs, ffs)):
        assert fb.shape == ff.shape == (b, n - 1, 2, h >> i, w >> i)
        pool = lambda a, s: torch.nn.functional.avg_pool2d(torch.stack([a.mean(1), s.mean(1) * 2], 1), 2 ** i).view(b, n - 1, 2, h >> i, w >> i)
        assert torch.equal(fb, pool(x1, x2)) and torch.equal(ff, pool(x2, x1))
    # level 0, clip 1, pair 2: the backward flow's reference frame is frame 2 and its support frame 3; the forward flow's the reverse
    assert torch.equal(fbs[0][1, 2, 0], x[1, 2].mean(0)) and torch.equal(fbs[0][1, 2, 1], x[1, 3].mean(0) * 2)
    assert torch.equal(ffs[0][1, 2, 0], x[1, 3].mean(0)) and torch.equal(ffs[0][1, 2, 1], x[1, 2].mean(0) * 2)


def test_documents_say_what_is_provided():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "nearest4" in readme and "aligned_input" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "11h" in design and "warp_taps" in design
    assert "nearest4" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
