"""Generate tests/golden/perceptual_loss.npz from the REAL reference PerceptualLoss (core/losses.py:8,29-64).

Needs a checkout of the reference (santurini/vsrlab); pass its ``src`` directory, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_perceptual.py PATH/TO/vsrlab/src

core/losses.py imports torchvision.models (vgg19), kornia and RAFT at module level; they are replaced by in-memory stubs:
``vgg19`` returns the standard configuration-'E' ``features`` (Conv2d 3x3 / ReLU(inplace=True) / MaxPool2d(2, 2)), so the
reference's own PerceptualVGG slices, freezes and runs it, tap quirk included.  Weights are NOT stored: both sides regenerate
them with tests/perceptual_common.keyed_vgg_state_dict.  Everything runs in fp64.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

SHAPE = (1, 2, 3, 40, 72)          # deep levels odd: 5 x 9 at the fourth pool input, 2 x 4 at conv5
SEED_SR, SEED_HR = 71, 72


def _vgg19_stub(pretrained=False):
    cfg = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    m = nn.Module()
    m.features = nn.Sequential(*layers)
    return m


def import_reference_losses(ref_src):
    if not os.path.isfile(os.path.join(ref_src, "core", "losses.py")):
        raise SystemExit(f"{ref_src}: not the reference's src directory (core/losses.py missing)")
    pkg = types.ModuleType("vsrlab")
    pkg.__path__ = [ref_src]
    sys.modules["vsrlab"] = pkg
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.vgg19 = _vgg19_stub
    ops = types.ModuleType("torchvision.ops")

    class DeformConv2d(nn.Module):
        pass

    ops.DeformConv2d = DeformConv2d
    ops.deform_conv2d = None
    tv.models, tv.ops = models, ops
    kornia = types.ModuleType("kornia")
    kg = types.ModuleType("kornia.geometry")
    kgt = types.ModuleType("kornia.geometry.transform")
    kgt.resize = None
    kornia.geometry, kg.transform = kg, kgt
    raft = types.ModuleType("vsrlab.optical_flow.models.raft.raft")

    class RAFT(nn.Module):
        pass

    raft.RAFT = RAFT
    for name, mod in (("torchvision", tv), ("torchvision.models", models), ("torchvision.ops", ops), ("kornia", kornia),
                      ("kornia.geometry", kg), ("kornia.geometry.transform", kgt), ("vsrlab.optical_flow.models.raft.raft", raft)):
        sys.modules[name] = mod
    from vsrlab.core import losses
    return losses


def main(ref_src):
    from helpers import rand
    from perceptual_common import LAYER_WEIGHTS, keyed_vgg_state_dict
    losses = import_reference_losses(ref_src)
    assert losses.LAYER_WEIGHTS == LAYER_WEIGHTS
    torch.set_num_threads(8)
    m = losses.PerceptualLoss(weight=1).double()
    sd = keyed_vgg_state_dict(dtype=torch.float64)
    assert set(m.state_dict()) == set(sd) and len(sd) == 32
    m.load_state_dict(sd, strict=True)
    sr = rand(SEED_SR, *SHAPE).double().requires_grad_(True)
    hr = rand(SEED_HR, *SHAPE).double()
    loss = m(sr, hr)
    loss.backward()
    h, w = SHAPE[-2:]
    with torch.no_grad():
        fs = m.vgg(sr.reshape(-1, 3, h, w))
        fh = m.vgg(hr.reshape(-1, 3, h, w))
        terms = torch.stack([torch.nn.functional.l1_loss(fs[k], fh[k]) * LAYER_WEIGHTS[k] for k in LAYER_WEIGHTS])
        # the pre-ReLU tap 34, recomputed (the stored dict entry is the module output itself)
        x = sr.reshape(-1, 3, h, w)
        for j, mod in enumerate(m.vgg.vgg_layers):
            x = mod(x.clone())
            if j == 34:
                conv54 = x
    share = terms / loss.detach()
    assert torch.allclose(terms.sum(), loss.detach(), rtol=1e-12), (terms.sum(), loss)
    assert float(share.min()) >= 0.01, share           # every tap pins the result
    neg = float((conv54 < 0).double().mean())
    assert neg > 0.05, neg                              # tap 34 is pre-ReLU: negative outputs present
    print("tap shares", [f"{float(s):.3f}" for s in share], f"conv5_4 negative fraction {neg:.3f}")
    out = {"seed_sr": np.int64(SEED_SR), "seed_hr": np.int64(SEED_HR), "shape": np.asarray(SHAPE, np.int64),
           "loss": loss.detach().numpy(), "terms": terms.numpy(), "dsr": sr.grad.numpy()}
    np.savez_compressed(os.path.join(HERE, "perceptual_loss.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
