"""The local correlation / PWC cost volume at size: the fused HIP kernel (csrc/spatial_corr.hip) against a torch evaluation of
the displacement loop (one pass over both maps per displacement, as the reference evaluates it) on the same GPU.
    python tools/bench_spatial_corr.py [--shapes 196x7x16,...] [--patch 9] [--batch 1] [--warmup 5] [--iters 20] [--out profiles/spatial_corr_bench.json]
Default shapes: the five IRR-PWC levels of a 448 x 1024 frame and two super-resolution-sized maps.  Forward and forward +
backward (both gradients), fp32 and bf16 storage; hipEvent timing, median after warm-up, the two paths interleaved in one
process.  Per leg: the speed-up and the fraction of 8 TB/s reached on the algorithmic bytes -- forward: both maps read once and
the output written once; forward + backward: that, plus both maps and the cotangent read and both gradients written once more.
Nothing here is a gate: the file is where the numbers go."""
import argparse
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
DEFAULT_SHAPES = "196x7x16,128x14x32,96x28x64,64x56x128,32x112x256,64x135x240,32x270x480"


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


def torch_loop(f1, f2, patch, store=None):
    """stride 1, no padding, dilation_patch 1: plane (i, j) = sum_c f1 * (f2 shifted by (i - m, j - m)), one pass per plane"""
    if store is not None:
        f1, f2 = store(f1), store(f2)
    m = (patch - 1) // 2
    h, w = f1.shape[-2:]
    wide = F.pad(f2, (m, m, m, m))
    planes = [(f1 * wide[:, :, i:i + h, j:j + w]).sum(dim=1) for i in range(patch) for j in range(patch)]
    return torch.stack(planes, dim=1).reshape(f1.shape[0], patch, patch, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated CxHxW")
    ap.add_argument("--patch", type=int, default=9)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spatial_corr.py measures on an MI355X; no GPU found")
    from vsrlab_amd import functional as VF
    dev = torch.device("cuda:0")
    P, N = args.patch, args.batch
    result = {"what": "tools/bench_spatial_corr.py: local correlation, patch %d, stride 1, batch %d; fused HIP kernel vs the torch displacement "
                      "loop on the same MI355X, interleaved, hipEvent median; hbm_fraction = algorithmic bytes / time / 8 TB/s" % (P, N),
              "tree": tree_hash(), "warmup": args.warmup, "iters": args.iters, "shapes": {}}
    for shape in args.shapes.split(","):
        C, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        f1 = torch.randn(N, C, H, W, device=dev, generator=g)
        f2 = torch.randn(N, C, H, W, device=dev, generator=g)
        cot = torch.randn(N, P, P, H, W, device=dev, generator=g)
        maps, vol = 2 * f1.numel() * 4, cot.numel() * 4
        bytes_of = {"fwd": maps + vol, "fwd_bwd": (maps + vol) + (maps + vol + maps)}
        entry = {"N": N, "C": C, "H": H, "W": W, "algorithmic_mb": {k: round(v / 1e6, 2) for k, v in bytes_of.items()}, "legs": {}}
        for dt in ("fp32", "bf16"):
            store = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if dt == "bf16" else None

            def hip_fwd():
                with torch.no_grad():
                    VF.spatial_correlation(f1, f2, P, compute_dtype=dt)

            def hip_fb():
                a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
                VF.spatial_correlation(a, b, P, compute_dtype=dt).backward(cot)

            def ref_fwd():
                with torch.no_grad():
                    torch_loop(f1, f2, P, store)

            def ref_fb():
                a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
                torch_loop(a, b, P, store).backward(cot)

            for leg, hip, ref in (("fwd", hip_fwd, ref_fwd), ("fwd_bwd", hip_fb, ref_fb)):
                th, tr = [], []
                for i in range(args.warmup + args.iters):
                    x, y = timed(hip), timed(ref)
                    if i >= args.warmup:
                        th.append(x)
                        tr.append(y)
                mh, mr = statistics.median(th), statistics.median(tr)
                rec = {"hip_ms": round(mh, 4), "hip_ms_min_max": [round(min(th), 4), round(max(th), 4)], "torch_loop_ms": round(mr, 3),
                       "speedup": round(mr / mh, 1), "hbm_fraction": round(bytes_of[leg] / (mh * 1e-3) / HBM_BYTES_PER_S, 4)}
                entry["legs"][f"{dt}_{leg}"] = rec
                print(shape, dt, leg, rec, flush=True)
        result["shapes"][shape] = entry
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
