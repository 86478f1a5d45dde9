"""Generate tests/golden/conv3d.npz from the REAL reference (its ``ConvST`` / ``ConvSTBlock``, ``PixelShufflePack3D`` and VRT's
``Upsample``).  Needs a checkout of the reference (santurini/vsrlab) and ``einops``, which its modules import; pass its ``src``
directory, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conv3d.py PATH/TO/vsrlab/src

The reference is imported under its ``vsrlab`` alias with the in-memory stubs of make_golden_raft.py.  Everything runs in fp64 on
the CPU on the inputs of tests/conv3d_common.py; only the reference's OUTPUTS are stored (tensors above mixer_common.FULL elements as
a sub-sample plus three statistics), under 128 KiB:

(1) per op case ``op{i}``: output, d input, d weight and d bias of the layer as the reference composes it -- ``nn.Conv3d`` between its
    ``rearrange`` / ``transpose`` hops, ``nn.PixelShuffle`` on the (b,t,c,h,w) order, ``nn.LeakyReLU`` -- under a seeded cotangent.
(2) per module case: output, d input and every parameter gradient with the seeded weights; the ``state_dict`` keys and shapes."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import conv3d_common as CC  # noqa: E402
from make_golden_mixer import key_record  # noqa: E402
from make_golden_raft import import_reference  # noqa: E402


def main(ref_src):
    import_reference(ref_src)
    conv = importlib.import_module("vsrlab.core.modules.conv")
    ups = importlib.import_module("vsrlab.core.modules.upsampling")
    vrt = importlib.import_module("vsrlab.vsr.models.VRT.vrt")
    classes = {"ConvST": conv.ConvST, "ConvSTBlock": conv.ConvSTBlock, "PixelShufflePack3D": ups.PixelShufflePack3D, "Upsample": vrt.Upsample}
    store = {}

    # (1) the layer, as the reference composes it
    for i, case in enumerate(CC.OP_CASES):
        x, w, b, cot = (None if v is None else v.double() for v in CC.op_inputs(i))
        k = CC.TAPS[case["taps"]]
        layer = nn.Conv3d(case["Cin"], case["Cout"], k, padding=tuple(s // 2 for s in k), bias=b is not None).double()
        layer.load_state_dict({"weight": w} if b is None else {"weight": w, "bias": b})
        x.requires_grad_(True)
        y = layer(x.transpose(1, 2) if case["order"] == "t" else x)                    # (b,c,t,h,w), the 'rearrange'
        if case.get("shuffle"):
            y = nn.PixelShuffle(case["shuffle"])(y.transpose(1, 2)).transpose(1, 2)    # Upsample's Transpose_Dim12 hops
        if case.get("slope") is not None:
            y = nn.LeakyReLU(case["slope"])(y)
        if case["order"] == "t":
            y = y.transpose(1, 2)
        (y * cot).sum().backward()
        CC.put(store, f"op{i}__out", y)
        CC.put(store, f"op{i}__dx", x.grad)
        CC.put(store, f"op{i}__dw", layer.weight.grad)
        if b is not None:
            CC.put(store, f"op{i}__db", layer.bias.grad)
        print(f"(1) op{i} {case['name']}: out {tuple(y.shape)}")

    # (2) the modules
    for name, (cls, args, _) in CC.MODULE_CASES.items():
        model = classes[cls](*args)
        key_record(store, "module_" + name, model)
        model.load_state_dict(CC.module_params(name), strict=True)
        model = model.double()
        x, cot = (v.double() for v in CC.module_inputs(name))
        x.requires_grad_(True)
        out = model(x)
        (out * cot).sum().backward()
        CC.put(store, f"{name}__out", out)
        CC.put(store, f"{name}__dx", x.grad)
        for k, p in model.named_parameters():
            CC.put(store, f"{name}__grad__{k}", p.grad)
        print(f"(2) {name}: out {tuple(out.shape)}, {len(list(model.parameters()))} parameter gradients")

    path = os.path.join(HERE, "conv3d.npz")
    np.savez_compressed(path, **store)
    print("conv3d.npz", len(store), "arrays,", os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 128 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
