"""CPU-side checks of the RAFT surface: the fp64 restatements (tests/raft_common.py) against the goldens recorded from the
reference (tests/golden/raft.npz), which guards the fixture and the helpers against each other; the state_dict schema; dotted
paths; exported symbols; constructor, size and weight-file validation."""
import importlib
import os

import numpy as np
import pytest
import torch

import raft_common as RC
from helpers import GOLDEN, proj_vector, rel_err


def _z():
    return np.load(os.path.join(GOLDEN, "raft.npz"), allow_pickle=False)


def _check(z, tag, key, value, tol=1e-6):
    """``value`` against what tests/golden/make_golden_raft.py stored: whole, or every stride-th element, plus its statistics"""
    v = value.detach().double()
    if f"{tag}__{key}" in z.files:
        assert rel_err(v, torch.from_numpy(z[f"{tag}__{key}"])) < tol
    else:
        assert rel_err(v.flatten()[::RC.sub_stride(v.numel())], torch.from_numpy(z[f"{tag}__sub__{key}"])) < tol
    s, n, p = (float(t) for t in z[f"{tag}__stats__{key}"])
    assert abs(float(v.norm()) / n - 1) < tol
    assert abs(float((v * proj_vector(f"raft.{tag}.{key}", tuple(v.shape))).sum()) - p) < tol * n * np.sqrt(v.numel())


def test_lookup_restatement_reproduces_the_reference_correlation():
    z = _z()
    f1, f2, coords, cot = RC.lookup_inputs(1, 17, 23)
    f1.requires_grad_(True), f2.requires_grad_(True)
    out = RC.corr_lookup_ref(coords, f1, f2)
    (out * cot).sum().backward()
    assert float(z["a__out_absmax"]) > 1.0
    _check(z, "a", "out", out)
    _check(z, "a", "dfmap1", f1.grad)
    _check(z, "a", "dfmap2", f2.grad)
    # the far points and the rows pushed outside are exact zeros
    for (y, x) in RC.far_points(17, 23):
        assert float(out[:, :, y, x].abs().max()) == 0.0
    assert float(out[:, :49, 1].abs().max()) == 0.0 and float(out[:, :49, 15].abs().max()) == 0.0


def test_on_demand_form_equals_the_all_pairs_form():
    """the identity the kernel rests on: level l of the volume = dot products with fmap2 pooled l times (fp64, to rounding)"""
    f1, f2, _, _ = RC.lookup_inputs(2, 17, 23, seed=5)
    vols = RC.corr_volumes(f1, f2, 4)
    lev = f2
    for l in range(4):
        if l:
            lev = torch.nn.functional.avg_pool2d(lev, 2, stride=2)
        direct = torch.einsum("ndp,ndq->npq", f1.reshape(2, 128, -1), lev.reshape(2, 128, -1)) / float(np.float32(np.sqrt(np.float32(128))))
        assert tuple(vols[l].shape[-2:]) == RC.level_sizes(17, 23, 4)[l]
        assert float((direct - vols[l].reshape(direct.shape)).abs().max()) < 1e-12


def test_raft_small_restatement_reproduces_the_reference_model():
    z = _z()
    sd = RC.raft_state_dict(RC.load_schema())
    ref, supp, cot = RC.raft_inputs()
    ref.requires_grad_(True), supp.requires_grad_(True)
    flow_up, low = RC.raft_small_ref(sd, ref, supp, return_low=True)
    (flow_up * cot).mean().backward()
    # the golden moves its windows: more than 4 px of flow at 1/8 resolution
    assert float(z["b__max_low_flow"]) > 4.0
    assert abs(float(low.abs().max()) - float(z["b__max_low_flow"])) < 1e-6
    _check(z, "b", "flow_up", flow_up)
    _check(z, "b", "dref", ref.grad)
    _check(z, "b", "dsupp", supp.grad)


def test_flow_consistency_restatement_reproduces_the_reference_loss():
    z = _z()
    sd = RC.raft_state_dict(RC.load_schema())
    sr, hr = RC.loss_inputs()
    sr.requires_grad_(True)
    loss = RC.flow_consistency_ref(sd, sr, hr)
    loss.backward()
    assert abs(float(loss) / float(z["c__loss"]) - 1) < 1e-6
    _check(z, "c", "dsr", sr.grad)


def test_state_dict_schema_equals_the_reference():
    from vsrlab_amd.optical_flow.models.raft.raft import RAFT
    m = RAFT(small=True, scale_factor=8, pretrained=False)
    schema = RC.load_schema()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == schema
    assert len(schema) == 106 and sum(int(np.prod(s)) for _, s in schema) == 990162
    from vsrlab_amd.optical_flow.models.raft.raft import load_raft_state_dict
    sd = load_raft_state_dict({"module." + k: v for k, v in RC.raft_state_dict(schema, torch.float32).items()})
    m.load_state_dict(sd, strict=True)
    m2 = RAFT(weights={"module." + k: v for k, v in sd.items()})
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_reference_dotted_paths_resolve():
    from vsrlab_amd.compat import install_as_vsrlab
    install_as_vsrlab(force=True)
    for mod, names in (("raft", ("RAFT",)), ("corr", ("correlation",)), ("extractor", ("SmallEncoder", "BottleneckBlock")),
                       ("update", ("SmallUpdateBlock", "ConvGRU", "SmallMotionEncoder", "FlowHead")),
                       ("utils", ("coords_grid", "upflow", "bilinear_sampler"))):
        m = importlib.import_module("vsrlab.optical_flow.models.raft." + mod)
        for name in names:
            assert hasattr(m, name), (mod, name)
    assert hasattr(importlib.import_module("vsrlab.core.losses"), "OpticalFlowConsistency")


def test_library_exports_and_workspace():
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    for name in ("vsr_raft_corr_workspace_bytes", "vsr_raft_corr_pyramid_fwd", "vsr_raft_corr_pyramid_bwd", "vsr_raft_corr_lookup_fwd",
                 "vsr_raft_corr_lookup_bwd"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.vsr_abi_version() == 4
    pix = 17 * 23 * 2 + 8 * 11 + 4 * 5 + 2 * 2                      # fmap1 + the four levels
    b32 = VF.raft_corr_workspace_bytes((1, 128, 17, 23), 4, 3, _lib.DT_F32)
    b16 = VF.raft_corr_workspace_bytes((1, 128, 17, 23), 4, 3, _lib.DT_BF16)
    assert pix * 128 * 4 <= b32 <= pix * 128 * 4 + 5 * 256 and pix * 128 * 2 <= b16 <= pix * 128 * 2 + 5 * 256
    assert VF.raft_corr_workspace_bytes((1, 128, 17, 23), 4, 3, _lib.DT_BF16, gradients=True) == b32
    assert VF.raft_corr_workspace_bytes((1, 128, 16, 16), 4) > 0          # level 3 is 2 x 2
    assert VF.raft_corr_workspace_bytes((1, 128, 15, 16), 4) == 0         # level 3 would be 1 high
    assert VF.raft_corr_workspace_bytes((1, 128, 15, 16), 3) > 0
    assert VF.raft_corr_workspace_bytes((1, 256, 17, 23), 4) == 0         # D
    assert VF.raft_corr_workspace_bytes((1, 128, 17, 23), 4, 4) == 0      # radius
    assert VF.raft_corr_workspace_bytes((1, 128, 17, 23), 5) == 0         # levels


def test_validation():
    from vsrlab_amd import functional as VF
    from vsrlab_amd.optical_flow.models.raft.raft import RAFT
    with pytest.raises(NotImplementedError):
        RAFT(small=False, pretrained=False)
    m = RAFT(pretrained=False)
    for h, w in ((130, 136), (128, 132), (120, 136), (128, 120)):       # not a multiple of 8; below 128
        with pytest.raises(ValueError, match="multiples of 8 and at least 128"):
            m(torch.zeros(1, 3, h, w), torch.zeros(1, 3, h, w))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError):
        VF.raft_corr_pyramid(torch.zeros(1, 128, 16, 16), torch.zeros(1, 128, 16, 17))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.raft_correlation(torch.zeros(1, 2, 16, 16), torch.zeros(1, 128, 16, 16), torch.zeros(1, 128, 16, 16))


def test_missing_weight_file_is_file_not_found(tmp_path, monkeypatch):
    from vsrlab_amd.core.losses import OpticalFlowConsistency
    from vsrlab_amd.optical_flow.models.raft.raft import RAFT
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    expected = os.path.join(str(tmp_path), "src", "optical_flow", "weights", "raft-small.pth")
    with pytest.raises(FileNotFoundError) as e:
        RAFT()
    assert expected in str(e.value)
    with pytest.raises(FileNotFoundError):
        OpticalFlowConsistency()
    with pytest.raises(FileNotFoundError):
        RAFT(weights=str(tmp_path / "nope.pth"))
    # ... and a file at the expected place loads, frozen inside the loss
    os.makedirs(os.path.dirname(expected))
    torch.save({"module." + k: v for k, v in RC.raft_state_dict(RC.load_schema(), torch.float32).items()}, expected)
    loss = OpticalFlowConsistency(weight=0.5)
    assert loss.weight == 0.5 and loss.of.scale_factor == 8 and not any(p.requires_grad for p in loss.parameters())
