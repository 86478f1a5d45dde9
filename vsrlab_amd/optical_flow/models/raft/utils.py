"""``coords_grid`` / ``upflow`` / ``bilinear_sampler`` of the reference's ``raft/utils.py``."""
import torch
import torch.nn.functional as F


def bilinear_sampler(img, coords, mask=False):
    """``grid_sample`` in pixel coordinates (``align_corners=True``, zeros outside); ``coords[..., 0]`` is x.  Kept for the
    dotted path: the HIP lookup does its own sampling."""
    h, w = img.shape[-2:]
    x, y = coords[..., 0:1], coords[..., 1:2]
    grid = torch.cat([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], dim=-1).type_as(img)
    out = F.grid_sample(img, grid, align_corners=True)
    if mask:
        inside = (grid[..., 0:1] > -1) & (grid[..., 1:2] > -1) & (grid[..., 0:1] < 1) & (grid[..., 1:2] < 1)
        return out, inside.float()
    return out


def coords_grid(batch, ht, wd):
    """(batch, 2, ht, wd) integer pixel coordinates, channel 0 = x."""
    ys, xs = torch.meshgrid(torch.arange(ht), torch.arange(wd), indexing="ij")
    return torch.stack([xs, ys], dim=0)[None].repeat(batch, 1, 1, 1)


def upflow(flow, scale_factor=2, mode='bilinear'):
    return scale_factor * F.interpolate(flow, scale_factor=scale_factor, mode=mode, align_corners=True)
