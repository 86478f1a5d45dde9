"""VRT's aligned input at size: the fused clip call (csrc/warp_taps.hip: one launch forward; init + scatter (+ round for bf16)
backward) and, in the same run, the same computation as the reference composes it from torch ops on the GPU -- per frame pair four
``grid_sample(mode='nearest')`` calls on four normalised grids and a ``cat``, then two ``stack``s and the ``cat`` of vrt.py:150 --
written out below.
    python tools/bench_warp_taps.py [--shapes 8x6x3x64x64,1x16x3x184x320] [--warmup 5] [--iters 20] [--calls 20] [--out profiles/warp_taps_bench.json]
Default shapes: B=8 of 6 x 3 x 64 x 64 (the configs' img_size) and B=1 of 16 x 3 x 184 x 320 (BASELINE config 5 padded to whole
windows).  fp32 and bf16.  A timed window is ``--calls`` calls back to back between two hipEvents (one fused call is tens of
microseconds: a window of one would measure the enqueue); per-call time = window / calls; the fused call and the composition
alternate window by window and the median of the windows after warm-up is reported with min and max.  "fwd" is the forward under
no_grad, "fwd_bwd" a forward with autograd and a backward from a fixed cotangent, "entry_fwd" the forward through the C entry into a
preallocated output (no allocation, no autograd).  ``--fused-only`` leaves the composition out (for a run under a profiler).
Algorithmic bytes of the forward per pixel and frame: x read once (C values), four flow values (16 bytes), 9 C values written;
gb_per_s is that count over the time and hbm_fraction the same over 8 TB/s.  Nothing here is a gate: the file is where the numbers go."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
DEFAULT_SHAPES = "8x6x3x64x64,1x16x3x184x320"


def tree_hash():
    try:
        with open(os.path.join(ROOT, "vsrlab_amd", "lib", "BUILD_INFO.json")) as f:
            info = json.load(f)
        return info["git_head"] + ("+dirty" if info.get("git_dirty_csrc") else "")
    except Exception:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
        return out or "unknown"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


# ---- the composition: what the reference runs, from torch ops --------------------------------------------------------------
def composed_nearest4(x, flow):
    """x (N, C, H, W), flow (N, H, W, 2): four nearest grid_samples on the floor / ceil grids, concatenated"""
    _, _, h, w = x.shape
    ys, xs = torch.meshgrid(torch.arange(0, h), torch.arange(0, w), indexing="ij")
    pos = torch.stack((xs, ys), 2).to(device=x.device, dtype=flow.dtype) + flow        # fp32 positions also under bf16 frames
    sx, sy = max(w - 1, 1), max(h - 1, 1)
    x0 = 2.0 * torch.floor(pos[..., 0]) / sx - 1.0
    x1 = 2.0 * torch.ceil(pos[..., 0]) / sx - 1.0
    y0 = 2.0 * torch.floor(pos[..., 1]) / sy - 1.0
    y1 = 2.0 * torch.ceil(pos[..., 1]) / sy - 1.0
    taps = [F.grid_sample(x, torch.stack(g, 3).to(x.dtype), mode="nearest", padding_mode="zeros", align_corners=True)
            for g in ((x0, y0), (x0, y1), (x1, y0), (x1, y1))]
    return torch.cat(taps, 1)


def composed_aligned_input(x, fb, ff):
    d = x.size(1)
    back = [torch.zeros_like(x[:, -1]).repeat(1, 4, 1, 1)]
    for i in range(d - 1, 0, -1):
        back.insert(0, composed_nearest4(x[:, i], fb[:, i - 1].permute(0, 2, 3, 1)))
    fwd = [torch.zeros_like(x[:, 0]).repeat(1, 4, 1, 1)]
    for i in range(0, d - 1):
        fwd.append(composed_nearest4(x[:, i], ff[:, i].permute(0, 2, 3, 1)))
    return torch.cat([x, torch.stack(back, 1), torch.stack(fwd, 1)], 2)


def smooth_flow(g, n, h, w, amp=4.0):
    """a flow as a flow network gives it: smooth, a few pixels, sub-pixel everywhere"""
    low = (torch.rand(n, 2, -(-h // 8) + 1, -(-w // 8) + 1, generator=g) * 2 - 1) * amp
    return F.interpolate(low, size=(h, w), mode="bilinear", align_corners=True).contiguous()


def alternate(legs, warmup, iters):
    """legs: name -> callable window; returns name -> per-window times after warm-up, the legs taking turns"""
    ts = {k: [] for k in legs}
    for _ in range(warmup + iters):
        for k, fn in legs.items():
            ts[k].append(timed(fn))
    return {k: v[warmup:] for k, v in ts.items()}


def stats(ts, calls):
    ts = [t / calls for t in ts]
    return statistics.median(ts), [round(min(ts), 4), round(max(ts), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated BxDxCxHxW")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_taps.py measures on an MI355X; no GPU found")
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load_warp_taps()
    dev = torch.device("cuda:0")
    result = {"what": "tools/bench_warp_taps.py: VRT's aligned input, cat([x, x_backward, x_forward], 2); the fused HIP clip call against the "
                      "reference's composition from torch ops (4 grid_sample + cat per pair, 2 stack, cat) on the same MI355X in the same run; "
                      "hipEvent windows of %d calls, the legs alternating, median per call; gb_per_s = algorithmic forward bytes / time" % args.calls,
              "tree": tree_hash(), "warmup": args.warmup, "iters": args.iters, "calls_per_window": args.calls, "shapes": {}}
    for shape in args.shapes.split(","):
        B, D, C, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        clip = torch.rand(B, D, C, H, W, generator=g)
        fb = smooth_flow(g, B * (D - 1), H, W).view(B, D - 1, 2, H, W).to(dev)
        ff = smooth_flow(g, B * (D - 1), H, W).view(B, D - 1, 2, H, W).to(dev)
        entry = {"B": B, "D": D, "C": C, "H": H, "W": W, "composition_launches_about": (D - 1) * 2 * 26 + 8, "legs": {}}
        for dt, tdt, code in (("fp32", torch.float32, _lib.DT_F32), ("bf16", torch.bfloat16, _lib.DT_BF16)):
            x = clip.to(tdt).to(dev)
            e = x.element_size()
            fwd_bytes = B * D * H * W * (C * e + 16 + 9 * C * e)
            cot = torch.randn(B, D, 9 * C, H, W, generator=g).to(tdt).to(dev)
            same = None
            if dt == "fp32" and not args.fused_only:   # bf16: grid_sample wants the grid in the frames' dtype, which moves taps
                with torch.no_grad():
                    same = bool(torch.equal(VF.aligned_input(x, fb, ff), composed_aligned_input(x, fb, ff)))

            def fused_fwd():
                with torch.no_grad():
                    for _ in range(args.calls):
                        VF.aligned_input(x, fb, ff)

            def comp_fwd():
                with torch.no_grad():
                    for _ in range(args.calls):
                        composed_aligned_input(x, fb, ff)

            def both(fn):
                def window():
                    for _ in range(args.calls):
                        leaf = x.detach().requires_grad_(True)
                        fn(leaf, fb, ff).backward(cot)
                return window

            out = torch.empty(B, D, 9 * C, H, W, dtype=tdt, device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            p = lambda t: ctypes.c_void_p(t.data_ptr())

            desc = _lib.WarpTapsDesc(B, D, C, H, W, 4, 0, code, 0)

            def entry_fwd():
                for _ in range(args.calls):
                    lib.vsr_warp_taps_clip_fwd(ctypes.byref(desc), p(x), p(fb), p(ff), p(out), st)

            legs = {"fused_fwd": fused_fwd, "fused_fwd_bwd": both(VF.aligned_input), "entry_fwd": entry_fwd}
            if not args.fused_only:
                legs.update({"composed_fwd": comp_fwd, "composed_fwd_bwd": both(composed_aligned_input)})
            ts = alternate(legs, args.warmup, args.iters)
            rec = {"equals_composition_bit_for_bit": same, "forward_bytes_mb": round(fwd_bytes / 1e6, 3)}
            for k, v in ts.items():
                m, mm = stats(v, args.calls)
                rec[k + "_ms"] = round(m, 4)
                rec[k + "_ms_min_max"] = mm
            for k in ("fused_fwd", "entry_fwd"):
                rec[k + "_gb_per_s"] = round(fwd_bytes / (rec[k + "_ms"] * 1e-3) / 1e9, 1)
                rec[k + "_hbm_fraction"] = round(fwd_bytes / (rec[k + "_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
            if not args.fused_only:
                rec["composed_over_fused_fwd"] = round(rec["composed_fwd_ms"] / rec["fused_fwd_ms"], 1)
                rec["composed_over_fused_fwd_bwd"] = round(rec["composed_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 1)
            entry["legs"][dt] = rec
            print(shape, dt, rec, flush=True)
        result["shapes"][shape] = entry
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
