"""Host-side tests of the VGG19 perceptual loss (core/losses.py:8,29-64): module tree, weight loading without downloads, Hydra
alias, argument checks and the workspace plan.  No GPU needed."""
import os

import pytest
import torch

from helpers import golden, rand, rel_err
from perceptual_common import CONVS, LAYER_WEIGHTS, keyed_vgg_state_dict, param_list, perceptual_terms


def _torchvision_style(sd):
    return {k.replace("vgg.vgg_layers.", "features."): v for k, v in sd.items()}


def test_module_tree_keys_and_frozen_parameters():
    from vsrlab_amd.core import losses as L
    sd = keyed_vgg_state_dict()
    m = L.PerceptualLoss(1e-2, vgg_weights=sd)
    got = m.state_dict()
    assert list(got) == [f"vgg.vgg_layers.{i}.{n}" for i, _, _ in CONVS for n in ("weight", "bias")]
    assert len(got) == 32
    for k, v in sd.items():
        assert got[k].shape == v.shape and torch.equal(got[k], v), k
    assert all(not p.requires_grad for p in m.parameters())
    assert m.layer_weights == LAYER_WEIGHTS == L.LAYER_WEIGHTS and m.weight == 1e-2
    layers = m.vgg.vgg_layers
    assert len(layers) == 35 and isinstance(layers[34], torch.nn.Conv2d)
    assert all(layers[i].inplace for i in range(35) if isinstance(layers[i], torch.nn.ReLU))
    assert [i for i in range(35) if isinstance(layers[i], torch.nn.MaxPool2d)] == [4, 9, 18, 27]


def test_weights_load_torchvision_and_reference_style(tmp_path, monkeypatch):
    from vsrlab_amd.core import losses as L
    sd = keyed_vgg_state_dict()
    tv = _torchvision_style(sd)
    tv["features.36.foo"] = torch.zeros(1)                 # keys outside features[:35] (classifier, last pool) are ignored
    tv["classifier.0.weight"] = torch.zeros(2, 2)
    ref_path = tmp_path / "ref.pth"
    torch.save(sd, ref_path)
    a = L.PerceptualLoss(vgg_weights=str(ref_path))
    b = L.PerceptualLoss(vgg_weights=tv)
    # torchvision's cache file under a temporary TORCH_HOME
    home = tmp_path / "torch_home"
    os.makedirs(home / "hub" / "checkpoints")
    torch.save(_torchvision_style(sd), home / "hub" / "checkpoints" / L.VGG19_CHECKPOINT)
    monkeypatch.setenv("TORCH_HOME", str(home))
    monkeypatch.setattr(torch.hub, "_hub_dir", None, raising=False)
    assert torch.hub.get_dir() == str(home / "hub")
    c = L.PerceptualLoss()
    for m in (a, b, c):
        for k, v in sd.items():
            assert torch.equal(m.state_dict()[k], v), k


def test_missing_weights_raise_and_never_download(tmp_path, monkeypatch):
    from vsrlab_amd.core import losses as L
    calls = []
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", lambda *a, **k: calls.append(a))
    monkeypatch.setattr(torch.hub, "download_url_to_file", lambda *a, **k: calls.append(a))
    import urllib.request
    monkeypatch.setattr(urllib.request, "urlopen", lambda *a, **k: calls.append(a))
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "empty"))
    monkeypatch.setattr(torch.hub, "_hub_dir", None, raising=False)
    with pytest.raises(FileNotFoundError, match="vgg19-dcbb9e9d.pth"):
        L.PerceptualLoss(weight=1e-2)
    assert calls == []


def test_hydra_alias_instantiates_with_the_cached_checkpoint(tmp_path, monkeypatch):
    from vsrlab_amd import compat
    from vsrlab_amd.core import losses as L
    home = tmp_path / "torch_home"
    os.makedirs(home / "hub" / "checkpoints")
    torch.save(_torchvision_style(keyed_vgg_state_dict()), home / "hub" / "checkpoints" / L.VGG19_CHECKPOINT)
    monkeypatch.setenv("TORCH_HOME", str(home))
    monkeypatch.setattr(torch.hub, "_hub_dir", None, raising=False)
    compat.install_as_vsrlab()
    m = compat.instantiate({"_target_": "vsrlab.core.losses.PerceptualLoss", "weight": 1e-2})
    assert isinstance(m, L.PerceptualLoss) and m.weight == 1e-2 and len(m.state_dict()) == 32


def test_cpu_tensors_and_bad_shapes_raise_before_any_gpu_call(monkeypatch):
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core import losses as L

    def boom():
        raise AssertionError("the HIP library was reached")
    monkeypatch.setattr(_lib, "load", boom)
    m = L.PerceptualLoss(vgg_weights=keyed_vgg_state_dict())
    x = torch.rand(1, 2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        m(x, x.clone())
    for a, b in ((torch.rand(1, 3, 15, 32), torch.rand(1, 3, 15, 32)),      # too small for four pools
                 (torch.rand(1, 4, 32, 32), torch.rand(1, 4, 32, 32)),      # not RGB
                 (torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 48))):     # shapes differ
        with pytest.raises(ValueError):
            m(a, b)
    with pytest.raises(ValueError):
        VF.perceptual_loss(x, x, m.vgg.params()[:30])


def test_workspace_scales_with_the_chunk_size():
    from vsrlab_amd import functional as VF
    for dt in (VF.DT_F32, VF.DT_BF16):
        ws = [VF.perceptual_workspace_bytes(n, 40, 72, dt) for n in (1, 2, 3, 6)]
        per = ws[1] - ws[0]
        assert per > 0 and ws[0] > per
        assert abs((ws[3] - ws[0]) - 5 * per) <= 5 * 4096          # linear in n (256-byte rounding of each buffer)
        assert VF.perceptual_workspace_bytes(2, 40, 72, dt, need_grad=False) < ws[1]
    assert VF.perceptual_workspace_bytes(1, 15, 72) == 0 and VF.perceptual_workspace_bytes(1, 16, 16) > 0
    big = VF.perceptual_workspace_bytes(1, 2160, 3840, VF.DT_BF16)
    assert VF.perceptual_chunk(7, 2160, 3840, VF.DT_BF16, True, 2 * big) == 2
    assert VF.perceptual_chunk(7, 2160, 3840, VF.DT_BF16, True, big // 2) == 1
    assert VF.perceptual_chunk(7, 2160, 3840, VF.DT_BF16, True, 100 * big) == 7


def test_restatement_matches_the_reference_golden():
    """The fp64 restatement the GPU tests check against reproduces the reference's own numbers (tap quirk included)."""
    z = golden("perceptual_loss")
    shape = tuple(int(s) for s in z["shape"])
    sr = rand(int(z["seed_sr"]), *shape).double().requires_grad_(True)
    hr = rand(int(z["seed_hr"]), *shape).double()
    terms = perceptual_terms(sr, hr, param_list(keyed_vgg_state_dict(dtype=torch.float64)))
    terms.sum().backward()
    assert rel_err(terms, z["terms"]) < 1e-12 and rel_err(terms.sum(), z["loss"]) < 1e-12
    assert rel_err(sr.grad, z["dsr"]) < 1e-10
