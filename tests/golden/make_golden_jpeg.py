"""Generate tests/golden/jpeg.npz from the REAL reference: ``RandomJPEGCompression`` of core/augmentations.py.  Needs a checkout
of the reference (santurini/vsrlab) and Pillow with JPEG support; pass the reference's ``src`` directory, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jpeg.py PATH/TO/vsrlab/src

core/augmentations.py is loaded by path.  It imports ``av`` (used only by its video classes) and
``torchvision.transforms.functional`` (of which the JPEG class uses ``to_pil_image`` and ``to_tensor``); neither is a dependency
here, so both names are shimmed before the import: ``av`` by an empty module, the two torchvision functions by their restatements in
tests/jpeg_common.py.  The class, its constructor, its forward and the PIL round trip are the reference's own.

Stored, for every case of ``jpeg_common.CASES`` at its qualities: the fp32 input ``<case>__x`` (the keyed input of
``jpeg_common.case_input``, stored so that the file stands alone) and the reference's output as bytes ``<case>__q<quality>``
(every output value is k / 255; k is stored)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_common as J  # noqa: E402


def load_reference(ref_src):
    path = os.path.join(ref_src, "core", "augmentations.py")
    if not os.path.isfile(path):
        raise SystemExit(f"{path}: not found (pass the reference's src directory)")
    if "av" not in sys.modules:
        sys.modules["av"] = types.ModuleType("av")
    if "torchvision" not in sys.modules:
        tv, tr, fn = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))
        fn.to_pil_image, fn.to_tensor = J.to_pil_image, J.to_tensor
        tv.transforms, tr.functional = tr, fn
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    spec = importlib.util.spec_from_file_location("reference_augmentations", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_src):
    if not J.pil_has_jpeg():
        raise SystemExit("Pillow without JPEG support: the reference cannot run")
    aug = load_reference(ref_src)
    store = {}
    for name in J.CASES:
        x = J.case_input(name)
        store[f"{name}__x"] = x.numpy()
        for q in J.CASES[name][1]:
            m = aug.RandomJPEGCompression([q, q])            # the reference's constructor: randint(q, q)
            assert m.q == q
            out = m(x)
            assert out.dtype == torch.float32 and out.shape == x.shape
            k = (out * 255).round()
            assert torch.equal(k / 255, out), "an output of the reference is not k / 255"
            store[f"{name}__q{q}"] = k.to(torch.uint8).numpy()
            assert torch.equal(m(x[0]), out[0]), "the reference's 3-D path differs from its batched path"
    out = os.path.join(HERE, "jpeg.npz")
    np.savez_compressed(out, **store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out) / 1024:.0f} KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
