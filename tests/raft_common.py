"""Pure-torch restatements for the RAFT tests, in whatever dtype their inputs have (fp64 for the oracles):

* ``corr_lookup_ref``: the correlation lookup in the all-pairs form -- the (H W) x (H W) volume, pooled over its second pixel
  index, sampled with an explicit floor / four-corner gather (no grid_sample, so no coordinate normalisation rounding).  It
  shares nothing with the kernel's formulation (pooled feature maps, dot products on demand).
* ``raft_small_ref``: RAFT-small as a function of a state dict, and ``flow_consistency_ref``, the loss on top of it.

``store``: where the bf16 build rounds -- the packed fmap1 and every stored level of the fmap2 pyramid -- the restatement rounds
too (``bf16_store``; straight-through for the gradient, as the kernel's fp32 accumulators are); None = exact.  The levels are a
property of fmap2 alone, so with ``store`` they are formed by pooling the rounded map, level by level, and the volume of each
level is still all pairs."""
import math

import torch
import torch.nn.functional as F

from helpers import BIG, _st, bf16_store, grad_stats, sub_stride  # noqa: F401  (the host tests read them here)

RADIUS = 3
TAPS = (2 * RADIUS + 1) ** 2


def level_sizes(H, W, num_levels):
    return [(H >> l, W >> l) for l in range(num_levels)]


def corr_volumes(fmap1, fmap2, num_levels=4, store=None):
    """[(N, H*W, H_l, W_l)]: level l of <fmap1[p], fmap2[q]> / float32(sqrt(D))."""
    N, D, H, W = fmap1.shape
    scale = torch.sqrt(torch.tensor(D).float()).to(fmap1.dtype)         # the reference divides by a float32 square root
    f1 = _st(fmap1, store).reshape(N, D, H * W)
    if store is None:
        vol = torch.matmul(f1.transpose(1, 2), fmap2.reshape(N, D, H * W)).reshape(N * H * W, 1, H, W) / scale
        vols = [vol]
        for _ in range(num_levels - 1):
            vol = F.avg_pool2d(vol, 2, stride=2)
            vols.append(vol)
        return [v.reshape(N, H * W, v.shape[-2], v.shape[-1]) for v in vols]
    lev, vols = _st(fmap2, store), []
    for l in range(num_levels):
        if l:
            lev = _st(F.avg_pool2d(lev, 2, stride=2), store)
        vols.append(torch.matmul(f1.transpose(1, 2), lev.reshape(N, D, -1)).reshape(N, H * W, lev.shape[-2], lev.shape[-1]) / scale)
    return vols


def corr_lookup_ref(coords, fmap1, fmap2, num_levels=4, radius=RADIUS, store=None):
    """(N, num_levels * 49, H, W); channel l * 49 + i * 7 + j samples level l at (x, y) = coords / 2^l + (i - 3, j - 3)."""
    N, D, H, W = fmap1.shape
    cx, cy = coords[:, 0].reshape(N, H * W, 1), coords[:, 1].reshape(N, H * W, 1)
    d = torch.arange(-radius, radius + 1, dtype=coords.dtype, device=coords.device)
    di, dj = [t.reshape(1, 1, -1) for t in torch.meshgrid(d, d, indexing="ij")]       # i slow (x), j fast (y)
    outs = []
    for l, vol in enumerate(corr_volumes(fmap1, fmap2, num_levels, store)):
        Hl, Wl = vol.shape[-2:]
        x, y = cx / 2 ** l + di, cy / 2 ** l + dj                                      # (N, HW, 49)
        x0, y0 = torch.floor(x), torch.floor(y)
        ax, ay = x - x0, y - y0
        flat = vol.reshape(N, H * W, Hl * Wl)

        def corner(xx, yy, wgt):
            valid = (xx >= 0) & (xx <= Wl - 1) & (yy >= 0) & (yy <= Hl - 1)
            idx = (yy.clamp(0, Hl - 1) * Wl + xx.clamp(0, Wl - 1)).long()
            return flat.gather(2, idx) * torch.where(valid, wgt, torch.zeros_like(wgt))

        outs.append(corner(x0, y0, (1 - ax) * (1 - ay)) + corner(x0 + 1, y0, ax * (1 - ay)) +
                    corner(x0, y0 + 1, (1 - ax) * ay) + corner(x0 + 1, y0 + 1, ax * ay))
    return torch.cat(outs, dim=2).reshape(N, H, W, -1).permute(0, 3, 1, 2)


# ---- inputs of the lookup tests and of golden (a) ----------------------------------------------------------------------------
FAR = (1e4, 3e9)


def lookup_inputs(N, H, W, seed=11, dtype=torch.float64):
    """fmap1, fmap2 (N, 128, H, W), coords (N, 2, H, W), cotangent (N, 196, H, W).  coords: the pixel grid + U(-6, 6); rows 1
    and H - 2 pushed 40 px outside (left / below); a handful of exact-integer and exact-half positions; two far points
    (+-1e4 and +-3e9 px), whose windows are exactly 0."""
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(N, 128, H, W, generator=g, dtype=torch.float64)
    f2 = torch.randn(N, 128, H, W, generator=g, dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    coords = torch.stack([xs, ys])[None].repeat(N, 1, 1, 1) + (torch.rand(N, 2, H, W, generator=g, dtype=torch.float64) * 12 - 6)
    coords[:, 0, 1] -= 40.0
    coords[:, 1, H - 2] += 40.0
    for k, (y, x) in enumerate(special_points(H, W)):
        if k < 4:
            coords[:, :, y, x] = torch.tensor([float((x + 2) % W), float((y + 1) % H)], dtype=torch.float64).view(1, 2)       # integers
        elif k < 8:
            coords[:, :, y, x] = torch.tensor([x + 0.5, y - 1.5], dtype=torch.float64).view(1, 2)                           # halves
    (ya, xa), (yb, xb) = far_points(H, W)
    coords[:, 0, ya, xa], coords[:, 1, ya, xa] = FAR[0], -FAR[0]
    coords[:, 0, yb, xb], coords[:, 1, yb, xb] = -FAR[1], FAR[1]
    cot = torch.randn(N, 4 * TAPS, H, W, generator=g, dtype=torch.float64)
    return [t.to(dtype) for t in (f1, f2, coords, cot)]


def special_points(H, W):
    return [(3 + k, (5 * k + 2) % W) for k in range(8)]


def far_points(H, W):
    return (H // 2, W // 2), (H - 1, W - 1)


def outside_rows(H):
    return (1, H - 2)


# ---- RAFT-small as a function of its state dict -----------------------------------------------------------------------------
def _conv(sd, key, x, stride=1, padding=0):
    return F.conv2d(x, sd[key + ".weight"], sd[key + ".bias"], stride=stride, padding=padding)


def _bottleneck(sd, pre, x, norm, stride):
    y = F.relu(norm(_conv(sd, pre + ".conv1", x)))
    y = F.relu(norm(_conv(sd, pre + ".conv2", y, stride=stride, padding=1)))
    y = F.relu(norm(_conv(sd, pre + ".conv3", y)))
    if stride != 1:
        x = norm(_conv(sd, pre + ".downsample.0", x, stride=stride))
    return F.relu(x + y)


def small_encoder_ref(sd, pre, x, instance_norm):
    norm = (lambda t: F.instance_norm(t, eps=1e-5)) if instance_norm else (lambda t: t)
    x = F.relu(norm(_conv(sd, pre + ".conv1", x, stride=2, padding=3)))
    for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
        x = _bottleneck(sd, f"{pre}.{layer}.0", x, norm, stride)
        x = _bottleneck(sd, f"{pre}.{layer}.1", x, norm, 1)
    return _conv(sd, pre + ".conv2", x)


def update_ref(sd, net, inp, corr, flow):
    p = "update_block."
    cor = F.relu(_conv(sd, p + "encoder.convc1", corr))
    flo = F.relu(_conv(sd, p + "encoder.convf2", F.relu(_conv(sd, p + "encoder.convf1", flow, padding=3)), padding=1))
    motion = torch.cat([F.relu(_conv(sd, p + "encoder.conv", torch.cat([cor, flo], 1), padding=1)), flow], 1)
    x = torch.cat([inp, motion], 1)
    hx = torch.cat([net, x], 1)
    z = torch.sigmoid(_conv(sd, p + "gru.convz", hx, padding=1))
    r = torch.sigmoid(_conv(sd, p + "gru.convr", hx, padding=1))
    q = torch.tanh(_conv(sd, p + "gru.convq", torch.cat([r * net, x], 1), padding=1))
    net = (1 - z) * net + z * q
    return net, _conv(sd, p + "flow_head.conv2", F.relu(_conv(sd, p + "flow_head.conv1", net, padding=1)), padding=1)


def raft_small_ref(sd, ref, supp, iters=12, scale_factor=8, store=None, return_low=False):
    """flow_up (N, 2, H, W); fnet on [supp, ref] (instance norm), cnet(supp) split 96 (tanh) / 64 (relu), ``iters`` updates with
    the coordinates detached before every lookup, bilinear align_corners=True upsampling times ``scale_factor``."""
    n = supp.shape[0]
    fmaps = small_encoder_ref(sd, "fnet", torch.cat([supp, ref], 0), True)
    fmap1, fmap2 = fmaps[:n], fmaps[n:]
    cnet = small_encoder_ref(sd, "cnet", supp, False)
    net, inp = torch.tanh(cnet[:, :96]), torch.relu(cnet[:, 96:])
    H, W = supp.shape[-2] // 8, supp.shape[-1] // 8
    ys, xs = torch.meshgrid(torch.arange(H, dtype=supp.dtype), torch.arange(W, dtype=supp.dtype), indexing="ij")
    coords0 = torch.stack([xs, ys])[None].repeat(n, 1, 1, 1)
    coords1 = coords0.clone()
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = corr_lookup_ref(coords1, fmap1, fmap2, 4, RADIUS, store=store)
        net, delta = update_ref(sd, net, inp, corr, coords1 - coords0)
        coords1 = coords1 + delta
    low = coords1 - coords0
    up = scale_factor * F.interpolate(low, scale_factor=scale_factor, mode="bilinear", align_corners=True)
    return (up, low) if return_low else up


def flow_consistency_ref(sd, sr, hr, weight=1.0, store=None):
    b, t, c, h, w = sr.shape
    pair = lambda v: (v[:, 1:].reshape(-1, c, h, w), v[:, :-1].reshape(-1, c, h, w))
    flow_sr = raft_small_ref(sd, *pair(sr), store=store)
    with torch.no_grad():
        flow_hr = raft_small_ref(sd, *pair(hr), store=store)
    return F.l1_loss(flow_sr, flow_hr) * weight


# ---- keyed weights and inputs of goldens (b) and (c) ------------------------------------------------------------------------
# Gains over oracle.basicvsr_oracle.keyed_tensor's 0.7 / sqrt(fan_in), chosen so that the 1/8-resolution flow of golden (b)
# exceeds 4 px somewhere and some windows leave the map (stored in the golden as b__max_low_flow and asserted by the host test):
# with smaller weights the twelve updates never move a window.
WSCALE = 1.0
FLOW_HEAD_SCALE = 3.0
RAFT_SHAPE = (2, 3, 128, 136)
LOSS_SHAPE = (1, 3, 3, 128, 136)


def raft_state_dict(schema, dtype=torch.float64):
    """``schema``: [(key, shape)] of RAFT-small's state dict -> keyed weights, a function of the key alone."""
    from oracle.basicvsr_oracle import keyed_tensor
    out = {}
    for k, shape in schema:
        v = keyed_tensor("raft." + k, tuple(shape)).double()
        if not k.endswith("bias"):
            v = v * (FLOW_HEAD_SCALE if k.startswith("update_block.flow_head.conv2") else WSCALE)
        out[k] = v.to(dtype)
    return out


def load_schema():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_schema.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def raft_inputs(dtype=torch.float64):
    """ref, supp, cotangent of flow_up for golden (b): smooth images (a few low-frequency waves + noise), supp a shifted ref"""
    g = torch.Generator().manual_seed(31)
    n, c, h, w = RAFT_SHAPE
    base = _smooth_images(n, c, h + 16, w + 16, g)
    ref, supp = base[..., 8:8 + h, 8:8 + w], base[..., 5:5 + h, 12:12 + w]
    cot = torch.randn(n, 2, h, w, generator=g, dtype=torch.float64)
    return ref.contiguous().to(dtype), supp.contiguous().to(dtype), cot.to(dtype)


def loss_inputs(dtype=torch.float64):
    g = torch.Generator().manual_seed(37)
    b, t, c, h, w = LOSS_SHAPE
    base = _smooth_images(b, c, h + 16, w + 16, g)                      # one scene, each frame a shifted crop of it
    hr = torch.stack([base[:, :, 8 + 2 * k:8 + 2 * k + h, 11 - 3 * k:11 - 3 * k + w] for k in range(t)], 1)
    sr = hr + 0.05 * torch.randn(hr.shape, generator=g, dtype=torch.float64)
    return sr.contiguous().to(dtype), hr.contiguous().to(dtype)


def _smooth_images(n, c, h, w, g):
    ys = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    img = torch.zeros(n, c, h, w, dtype=torch.float64)
    for _ in range(6):
        fy, fx, ph = (torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64) for _ in range(3))
        img = img + torch.sin(2 * math.pi * (fy * ys / 24 + fx * xs / 24 + ph))
    return 0.5 + img / 8 + 0.05 * torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
