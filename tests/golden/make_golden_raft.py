"""Generate tests/golden/raft.npz and tests/golden/raft_schema.json from the REAL reference (its ``correlation``, ``RAFT`` and
``OpticalFlowConsistency``).  Needs a checkout of the reference (santurini/vsrlab); pass its ``src`` directory, from the
repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raft.py PATH/TO/vsrlab/src

The reference is imported under its ``vsrlab`` alias; torchvision and kornia, which core/losses.py imports and RAFT does not use,
are in-memory stubs.  Everything runs in fp64 with keyed weights (tests/raft_common.raft_state_dict): only the key / shape list
and the reference's OUTPUTS are stored.  Large tensors are stored as every stride-th element plus (sum, norm, projection), the
scheme of deform_conv.npz.

(a) ``correlation()`` on (1, 128, 17, 23): output, d fmap1, d fmap2 for a keyed cotangent.
(b) ``RAFT(small=True, scale_factor=8, pretrained=False)`` on (2, 3, 128, 136): flow_up, d ref, d supp.
(c) ``OpticalFlowConsistency`` on (1, 3, 3, 128, 136): value and d sr; ``torch.load`` is patched to return the keyed weights (with
    the ``module.`` prefix the constructor strips), so the reference class's own constructor runs."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import raft_common as RC  # noqa: E402
from helpers import BIG, grad_stats, sub_stride  # noqa: E402


def import_reference(ref_src):
    if not os.path.isfile(os.path.join(ref_src, "optical_flow", "models", "raft", "raft.py")):
        raise SystemExit(f"{ref_src}: not the reference's src directory (optical_flow/models/raft/raft.py missing)")
    pkg = types.ModuleType("vsrlab")
    pkg.__path__ = [ref_src]
    sys.modules["vsrlab"] = pkg
    tv, models, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.ops")
    models.vgg19 = None

    class DeformConv2d(nn.Module):
        pass

    ops.DeformConv2d, ops.deform_conv2d = DeformConv2d, None
    tv.models, tv.ops = models, ops
    kornia, kg, kgt = types.ModuleType("kornia"), types.ModuleType("kornia.geometry"), types.ModuleType("kornia.geometry.transform")
    kgt.resize = None
    kornia.geometry, kg.transform = kg, kgt
    for name, mod in (("torchvision", tv), ("torchvision.models", models), ("torchvision.ops", ops), ("kornia", kornia),
                      ("kornia.geometry", kg), ("kornia.geometry.transform", kgt)):
        sys.modules[name] = mod
    from vsrlab.core import losses
    from vsrlab.optical_flow.models.raft import corr, raft
    return corr, raft, losses


def put(store, tag, key, g):
    g = g.detach()
    if g.numel() <= BIG:
        store[f"{tag}__{key}"] = g.numpy().astype(np.float64)
    else:
        store[f"{tag}__sub__{key}"] = g.flatten()[::sub_stride(g.numel())].numpy().astype(np.float64)
    store[f"{tag}__stats__{key}"] = grad_stats(f"raft.{tag}.{key}", g).numpy()


def main(ref_src):
    torch.set_num_threads(8)
    corr, raft, losses = import_reference(ref_src)
    store = {}

    # (a) the lookup
    f1, f2, coords, cot = RC.lookup_inputs(1, 17, 23)
    f1.requires_grad_(True), f2.requires_grad_(True)
    out = corr.correlation(coords, f1, f2, num_levels=4, radius=3)
    (out * cot).sum().backward()
    put(store, "a", "out", out)
    put(store, "a", "dfmap1", f1.grad)
    put(store, "a", "dfmap2", f2.grad)
    store["a__out_absmax"] = np.float64(out.detach().abs().max())

    # (b) RAFT-small
    m = raft.RAFT(small=True, scale_factor=8, pretrained=False)
    schema = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "raft_schema.json"), "w") as f:
        json.dump(schema, f)
    sd = RC.raft_state_dict(schema)
    m = m.double()
    m.load_state_dict(sd, strict=True)
    ref, supp, cot = RC.raft_inputs()
    ref.requires_grad_(True), supp.requires_grad_(True)
    flow_up = m(ref, supp)
    (flow_up * cot).mean().backward()
    with torch.no_grad():
        _, low = RC.raft_small_ref(sd, ref.detach(), supp.detach(), return_low=True)
    h, w = low.shape[-2:]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    cx, cy = xs + low[:, 0], ys + low[:, 1]
    leaving = float(((cx - 3 < 0) | (cx + 3 > w - 1) | (cy - 3 < 0) | (cy + 3 > h - 1)).double().mean())
    max_low = float(low.abs().max())
    print(f"(b) max |flow| at 1/8 resolution {max_low:.2f} px, windows leaving the map {leaving:.3f}, flow_up absmax {float(flow_up.detach().abs().max()):.2f}")
    assert max_low > 4.0 and leaving > 0.2, (max_low, leaving)
    store["b__max_low_flow"] = np.float64(max_low)
    put(store, "b", "flow_up", flow_up)
    put(store, "b", "dref", ref.grad)
    put(store, "b", "dsupp", supp.grad)

    # (c) the loss: the reference class's own constructor, fed the keyed weights through torch.load
    real_load = torch.load
    torch.load = lambda *a, **k: {"module." + key: v.float() for key, v in sd.items()}
    try:
        loss_mod = losses.OpticalFlowConsistency(weight=1.0)
    finally:
        torch.load = real_load
    loss_mod = loss_mod.double()
    loss_mod.of.load_state_dict(sd, strict=True)          # the constructor loaded the fp32 roundings: restore the fp64 values
    assert not any(p.requires_grad for p in loss_mod.parameters())
    sr, hr = RC.loss_inputs()
    sr.requires_grad_(True)
    loss = loss_mod(sr, hr)
    loss.backward()
    print(f"(c) loss {float(loss):.6f}, |d sr| max {float(sr.grad.abs().max()):.3e}")
    assert float(loss) > 1e-3
    store["c__loss"] = np.float64(loss.detach())
    put(store, "c", "dsr", sr.grad)

    path = os.path.join(HERE, "raft.npz")
    np.savez_compressed(path, **store)
    print("raft.npz", len(store), "arrays,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
