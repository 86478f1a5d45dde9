"""``correlation`` of the reference's ``raft/corr.py`` on the fused HIP lookup: no all-pairs volume is formed."""
from .... import functional as VF


def correlation(coords, fmap1, fmap2, num_levels=4, radius=4, compute_dtype=None):
    """(N, num_levels * (2 radius + 1)^2, H, W).  The signature (and the default radius 4) is the reference's; the HIP kernel
    serves RAFT-small's radius 3 and raises ``RuntimeError('... unsupported shape ...')`` for anything else."""
    return VF.raft_correlation(coords, fmap1, fmap2, num_levels=num_levels, radius=radius, compute_dtype=compute_dtype)
