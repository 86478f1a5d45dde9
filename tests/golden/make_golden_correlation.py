"""Generate tests/golden/correlation.npz from the REAL reference: ``iter_spatial_correlation_sample`` of
core/modules/correlation.py and ``compute_cost_volume`` of optical_flow/models/irr/pwc_modules.py.  Needs a checkout of the
reference (santurini/vsrlab); pass its ``src`` directory, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_correlation.py PATH/TO/vsrlab/src

The two files are loaded by path (both import torch only).  Everything runs in fp64 on the keyed inputs of
tests/correlation_common.py: only the reference's OUTPUTS are stored -- per case of ``CASES`` the sampler's output and both
gradients for the keyed cotangent, and the cost volume (max_disp 4) at case A the same way.  Tensors above ``BIG`` elements are
stored as every stride-th element plus (sum, norm, projection), the scheme of deform_conv.npz."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import correlation_common as CC  # noqa: E402
from helpers import BIG, grad_stats, sub_stride  # noqa: E402


def load_by_path(name, path):
    if not os.path.isfile(path):
        raise SystemExit(f"{path}: not found (pass the reference's src directory)")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def put(store, tag, key, g):
    g = g.detach()
    if g.numel() <= BIG:
        store[f"{tag}__{key}"] = g.numpy().astype(np.float64)
    else:
        store[f"{tag}__sub__{key}"] = g.flatten()[::sub_stride(g.numel())].numpy().astype(np.float64)
    store[f"{tag}__stats__{key}"] = grad_stats(f"correlation.{tag}.{key}", g).numpy()


def main(ref_src):
    torch.set_num_threads(8)
    corr = load_by_path("reference_correlation", os.path.join(ref_src, "core", "modules", "correlation.py"))
    pwc = load_by_path("reference_pwc_modules", os.path.join(ref_src, "optical_flow", "models", "irr", "pwc_modules.py"))
    store = {}
    for case in CC.CASES:
        for key, v in zip(("out", "d_input1", "d_input2"), CC.restate(case, fn=corr.iter_spatial_correlation_sample)):
            put(store, case, key, v)
        # the module form gives the same numbers
        _, patch, stride, padding, dil = CC.CASES[case]
        a, b, _ = CC.case_inputs(case)
        m = corr.SpatialCorrelationSampler(patch_size=patch, stride=stride, padding=padding, dilation_patch=dil)
        assert torch.equal(m(a, b), corr.iter_spatial_correlation_sample(a, b, patch_size=patch, stride=stride, padding=padding,
                                                                         dilation_patch=dil))
    for key, v in zip(("out", "d_input1", "d_input2"), CC.restate_cost_volume(fn=pwc.compute_cost_volume)):
        put(store, "cost", key, v)
    out = os.path.join(HERE, "correlation.npz")
    np.savez_compressed(out, **store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out) / 1024:.0f} KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
