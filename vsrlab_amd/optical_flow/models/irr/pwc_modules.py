"""``compute_cost_volume`` of the reference's ``irr/pwc_modules.py`` on one HIP launch: the (2 max_disp + 1)^2 displacements
share a single read of both feature maps."""
from .... import functional as VF


def compute_cost_volume(feat1, feat2, param_dict, compute_dtype=None):
    """(N, (2 max_disp + 1)^2, H, W): channel ``i * (2 max_disp + 1) + j`` is the mean over channels of ``feat1`` times ``feat2``
    displaced by ``(i - max_disp, j - max_disp)`` (vertical, horizontal), zeros outside.  Only ``param_dict["max_disp"]`` is
    read, as in the reference."""
    num_shifts = 2 * int(param_dict["max_disp"]) + 1
    n, c, h, w = feat1.shape
    cost = VF.spatial_correlation(feat1, feat2, patch_size=num_shifts, scale=1.0 / c, compute_dtype=compute_dtype)
    return cost.reshape(n, num_shifts * num_shifts, h, w)
