"""Generate tests/golden/warp_taps.npz from the REAL reference (through ``make_golden.import_reference()``): ``flow_warp`` of
vsr/models/VRT/modules/spynet.py in its 'nearest4' and 'nearest' modes and the static ``VRT.get_aligned_image`` of
vsr/models/VRT/vrt.py, on the seeded inputs of tests/warp_taps_common.py.  From the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_warp_taps.py

Stored per case of ``warp_taps_common.CASES`` and mode m in (nearest4, nearest): ``<case>__<m>`` the fp32 output with padding 'zeros',
``<case>__<m>_border`` with padding 'border' (cases of ``BORDER_GOLDEN``), ``<case>__<m>_gx`` the reference's autograd gradient
w.r.t. x under the integer cotangent ``grid_cotangent`` (small integers: every partial sum is exact in fp32, so the fp32 reference
IS the exact gradient and an fp64 oracle must equal it) and ``<case>__<m>_gflow_absmax``, the largest magnitude of its flow gradient
(a zeros tensor, not None).  Per clip of ``CLIP_GOLDEN``: ``<clip>__backward`` and ``<clip>__forward``, the two tensors of
``get_aligned_image``.  Inputs are not stored: they are regenerated from their keys."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import warp_taps_common as WT  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    from vsrlab.vsr.models.VRT.modules.spynet import flow_warp
    from vsrlab.vsr.models.VRT.vrt import VRT
    store = {}
    for name in WT.CASES:
        for taps, mode in ((4, "nearest4"), (1, "nearest")):
            x = WT.case_x(name).requires_grad_(True)
            flow = WT.to_channels_last(WT.case_flow(name, taps)).requires_grad_(True)      # the non-contiguous view the reference passes
            out = flow_warp(x, flow, mode)
            store[f"{name}__{mode}"] = out.detach().numpy()
            out.backward(WT.grid_cotangent(f"{name}:{mode}", out.shape))
            store[f"{name}__{mode}_gx"] = x.grad.numpy()
            assert flow.grad is not None and flow.grad.shape == flow.shape
            store[f"{name}__{mode}_gflow_absmax"] = np.float32(flow.grad.abs().max())
            if name in WT.BORDER_GOLDEN:
                store[f"{name}__{mode}_border"] = flow_warp(x.detach(), flow.detach(), mode, "border").numpy()
    for b, d, f in WT.CLIP_GOLDEN:
        x, fb, ff = WT.clip_inputs(b, d, f)
        xb, xf = VRT.get_aligned_image(x, fb, ff)
        store[WT.clip_name(b, d, f) + "__backward"] = xb.numpy()
        store[WT.clip_name(b, d, f) + "__forward"] = xf.numpy()
    out = os.path.join(HERE, "warp_taps.npz")
    np.savez_compressed(out, **store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
