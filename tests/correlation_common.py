"""Pure-torch restatements for the local-correlation tests (core/modules/correlation.py, irr/pwc_modules.py
compute_cost_volume), in whatever dtype their inputs have (fp64 for the oracles).

Not the reference's loop over displacements: the padded ``input2`` is turned into a view of all its windows by two ``unfold``
calls, strided by ``stride`` and ``dilation_patch``, and the whole result is one ``einsum``.  It shares nothing with the
kernel's formulation (tiles, bounds tests, per-chunk accumulation) either.  Pinned to the reference by
tests/test_correlation_host.py through tests/golden/correlation.npz.

``store``: where the bf16 build rounds -- both maps as they are re-laid -- the restatement rounds too (``bf16_store``;
straight-through for the gradient, as the kernel's sums and both gradients stay fp32); None = exact."""
import zlib

import torch
import torch.nn.functional as F

from helpers import BIG, _st, bf16_store, grad_stats, sub_stride  # noqa: F401  (the host tests read them here)

# name: (N, C, H, W), patch, stride, padding, dilation_patch -- the cases of the golden and of the GPU tests
CASES = {
    "A": ((2, 20, 11, 13), 9, 1, 0, 1),                     # C not a multiple of 8, ragged edges, batch stride
    "B": ((1, 196, 7, 16), 9, 1, 0, 1),                     # IRR's widest level; map shorter than the patch
    "C": ((2, 5, 9, 10), (3, 5), 2, (1, 2), 1),             # padding crop, stride, odd sizes, non-square patch
    "D": ((1, 33, 12, 17), 5, (1, 2), 0, 2),                # dilated patch, mixed stride, C = 32 + 1
    "E": ((1, 8, 3, 4), 9, 1, 0, 1),                        # map smaller than the displacement
    "F": ((1, 1, 6, 7), 1, 1, 0, 1),                        # a single tap and channel
    "G": ((1, 7, 10, 9), (7, 3), (2, 1), (2, 0), (2, 1)),   # everything per-axis at once
    "T": ((1, 16, 37, 70), 9, 1, 0, 1),                     # 5 x 3 workgroup tiles of 8 x 32
    # A grid below the 256 compute units is multiplied by groups of patch rows (forward) or of channel chunks (backward); A .. T
    # all run one row / one chunk per group.  U: 175 tiles, no split at all.  V: 96 tiles, two uneven groups of 5 + 4 rows.
    "U": ((5, 3, 40, 224), 9, 1, 0, 1),
    "V": ((1, 2, 64, 384), 9, 1, 0, 1),
}
COST_CASE, COST_MAX_DISP = "A", 4


def pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def out_shape(shape, patch, stride, padding):
    """(N, P_h, P_w, ceil(H' / s_h), ceil(W' / s_w))"""
    (n, _, h, w), p, s, pad = shape, pair(patch), pair(stride), pair(padding)
    return (n, p[0], p[1], -(-(h + 2 * pad[0]) // s[0]), -(-(w + 2 * pad[1]) // s[1]))


def spatial_correlation_ref(input1, input2, patch_size=1, stride=1, padding=0, dilation_patch=1, store=None):
    p, s, pad, d = pair(patch_size), pair(stride), pair(padding), pair(dilation_patch)
    m = (d[0] * (p[0] - 1) // 2, d[1] * (p[1] - 1) // 2)
    a = F.pad(_st(input1, store), (pad[1], pad[1], pad[0], pad[0]))
    b = F.pad(_st(input2, store), (pad[1] + m[1], pad[1] + m[1], pad[0] + m[0], pad[0] + m[0]))
    win = b.unfold(2, 2 * m[0] + 1, 1).unfold(3, 2 * m[1] + 1, 1)               # (N, C, H', W', 2 m_h + 1, 2 m_w + 1)
    win = win[:, :, ::s[0], ::s[1], ::d[0], ::d[1]]
    return torch.einsum("nchw,nchwij->nijhw", a[:, :, ::s[0], ::s[1]], win)


def compute_cost_volume_ref(feat1, feat2, param_dict, store=None):
    k = 2 * param_dict["max_disp"] + 1
    n, c, h, w = feat1.shape
    return (spatial_correlation_ref(feat1, feat2, k, store=store) / c).reshape(n, k * k, h, w)


def keyed(key, shape, dtype=torch.float64):
    """standard normal, a function of the key and the shape alone"""
    g = torch.Generator().manual_seed(zlib.crc32(("correlation." + key).encode()) & 0x7fffffff)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).to(dtype)


def case_inputs(case, dtype=torch.float64):
    """input1, input2, cotangent of the sampler's output"""
    shape, patch, stride, padding, _ = CASES[case]
    return (keyed(case + ".input1", shape, dtype), keyed(case + ".input2", shape, dtype),
            keyed(case + ".cot", out_shape(shape, patch, stride, padding), dtype))


def restate(case, store=None, dtype=torch.float64, fn=None):
    """(out, d input1, d input2) of the sampler at a case, for its keyed cotangent; ``fn``: evaluate something else with the
    restatement's signature (the golden generator passes the reference's function)."""
    _, patch, stride, padding, dil = CASES[case]
    a, b, cot = case_inputs(case, dtype)
    a.requires_grad_(True), b.requires_grad_(True)
    if fn is None:
        out = spatial_correlation_ref(a, b, patch, stride, padding, dil, store=store)
    else:
        out = fn(a, b, patch_size=patch, stride=stride, padding=padding, dilation_patch=dil)
    (out * cot).sum().backward()
    return out.detach(), a.grad, b.grad


def restate_cost_volume(store=None, dtype=torch.float64, fn=None):
    a, b, cot = case_inputs(COST_CASE, dtype)
    a.requires_grad_(True), b.requires_grad_(True)
    args = (a, b, {"max_disp": COST_MAX_DISP, "unused": None})
    out = compute_cost_volume_ref(*args, store=store) if fn is None else fn(*args)
    (out * cot.reshape(out.shape)).sum().backward()
    return out.detach(), a.grad, b.grad
