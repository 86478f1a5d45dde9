"""Generate tests/golden/loss_pipeline.npz from the REAL reference (its ``LossPipeline``, ``WL1Loss``, ``rmse_loss`` and
``CharbonnierLoss``).  Needs a checkout of the reference (santurini/vsrlab); pass its ``src`` directory, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py PATH/TO/vsrlab/src

The reference is imported under its ``vsrlab`` alias with the in-memory stubs of make_golden_raft.py; ``kornia``'s ``resize``, which
``LossPipeline.match_shapes`` calls, is bilinear ``F.interpolate(align_corners=False)`` over the flattened leading dimensions
(tests/losses_common.interp: the identity tests/test_training_glue.py::test_resize_matches_interpolate rests on).  Everything runs in
fp64 on the inputs of tests/losses_common.py; only the reference's OUTPUTS are stored, a few KiB.

(1) ``LossPipeline`` with losses charb / l1 (``WL1Loss(0.5)``) / rmse (``rmse_loss`` in a two-line module), prefix ``train/``, postfix
    ``_g`` and the four terms of losses_common.PIPELINE: every output key, d sr, d lq, and the key lists.
(2) ``WL1Loss(2.0, reduction="sum")`` and ``rmse_loss`` on a ragged (1, 2, 3, 5, 7) pair: value, d x, d y."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import losses_common as LC  # noqa: E402
from make_golden_raft import import_reference  # noqa: E402


def main(ref_src):
    _, _, losses = import_reference(ref_src)
    losses.resize = LC.interp
    store = {}

    class Rmse(nn.Module):
        def forward(self, x, y):
            return losses.rmse_loss(x, y)

    # (1) the pipeline
    pipe = losses.LossPipeline({"rmse": Rmse(), "l1": losses.WL1Loss(LC.L1_WEIGHT), "charb": losses.CharbonnierLoss()}, LC.PIPELINE,
                               prefix=LC.PREFIX, postfix=LC.POSTFIX)
    assert list(pipe.keys()) == ["charb", "l1", "rmse"]
    sr, hr, lq = (t.double() for t in LC.pipeline_inputs())
    sr.requires_grad_(True), lq.requires_grad_(True)
    out = pipe({"sr": sr, "hr": hr, "lq": lq})
    keys = [k for k in out if k not in ("sr", "hr", "lq")]
    assert sorted(keys) == sorted(LC.OUTPUT_KEYS), keys
    out[LC.PREFIX + "loss" + LC.POSTFIX].backward()
    for k in keys:
        store["pipe__" + k.replace("/", "|")] = np.float64(out[k].detach())
        print(f"(1) {k} = {float(out[k].detach()):.6f}")
    store["pipe__dsr"] = sr.grad.numpy().astype(np.float64)
    store["pipe__dlq"] = lq.grad.numpy().astype(np.float64)
    store["pipe__output_keys"] = np.array(keys)
    store["pipe__order"] = np.array([name for cfg in pipe.pipeline for name in cfg])

    # (2) the single losses
    for tag, fn in (("wl1", losses.WL1Loss(LC.SINGLE_L1_WEIGHT, reduction="sum")), ("rmse", losses.rmse_loss)):
        x, y = (t.double().requires_grad_(True) for t in LC.single_inputs())
        v = fn(x, y)
        v.backward()
        print(f"(2) {tag} = {float(v):.6f}")
        store[f"{tag}__value"] = np.float64(v.detach())
        store[f"{tag}__dx"] = x.grad.numpy().astype(np.float64)
        store[f"{tag}__dy"] = y.grad.numpy().astype(np.float64)

    path = os.path.join(HERE, "loss_pipeline.npz")
    np.savez_compressed(path, **store)
    print("loss_pipeline.npz", len(store), "arrays,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
