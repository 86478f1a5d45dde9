"""RAFT's correlation lookup at size: the fused HIP lookup (pyramid built once, outside the timed region, as RAFT's twelve
iterations use it) against a torch all-pairs evaluation of the same lookup (tests/raft_common.corr_lookup_ref: the volume, its
pooled copies, a four-corner gather; rebuilt in every call, as the reference does) on the same GPU, wherever the volume fits.
    python tools/bench_raft_corr.py [--sizes 6x68x120,1x270x480] [--warmup 3] [--iters 10] [--max-volume-gb 8] [--out profiles/raft_corr_bench.json]
Lookup forward and forward + backward (the backward leg includes the pyramid's own backward: un-pool and unpack), fp32 and
bf16; hipEvent timing, median after warm-up; peak device memory above the inputs for both paths.  The two paths run interleaved
in one process.  Nothing here is a gate: the file is where the numbers go."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6x68x120,1x270x480")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-volume-gb", type=float, default=8.0, help="run the all-pairs path only where its level-0 volume is below this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raft_corr.py measures on an MI355X; no GPU found")
    import raft_common as RC
    from vsrlab_amd import functional as VF
    dev = torch.device("cuda:0")
    result = {"what": "tools/bench_raft_corr.py: RAFT correlation lookup (4 levels, radius 3, D = 128), fused HIP lookup vs a torch "
                      "all-pairs evaluation on the same MI355X, interleaved, hipEvent median; HIP pyramid build outside the timed lookup",
              "tree": tree_hash(), "warmup": args.warmup, "iters": args.iters, "sizes": {}}
    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        f1 = torch.randn(N, 128, H, W, device=dev, generator=g)
        f2 = torch.randn(N, 128, H, W, device=dev, generator=g)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        coords = torch.stack([xs, ys])[None].to(dev) + (torch.rand(N, 2, H, W, device=dev, generator=g) * 8 - 4)
        cot = torch.randn(N, 196, H, W, device=dev, generator=g)
        volume_gb = N * (H * W) ** 2 * 4 / 1e9
        allpairs = volume_gb <= args.max_volume_gb
        entry = {"queries": N * H * W, "allpairs_volume_gb": round(volume_gb, 2), "legs": {}}
        if not allpairs:
            entry["allpairs"] = f"not run: the level-0 volume alone is {volume_gb:.1f} GB (--max-volume-gb {args.max_volume_gb})"
        for dt in ("fp32", "bf16"):
            store = RC.bf16_store if dt == "bf16" else None
            with torch.no_grad():
                pyr = VF.raft_corr_pyramid(f1, f2, 4, dt)

            def hip_fwd():
                with torch.no_grad():
                    VF.raft_corr_lookup(pyr, coords)

            def hip_build():
                with torch.no_grad():
                    VF.raft_corr_pyramid(f1, f2, 4, dt)

            def hip_fb():
                a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
                (VF.raft_corr_lookup(VF.raft_corr_pyramid(a, b, 4, dt), coords) * cot).sum().backward()

            def ref_fwd():
                with torch.no_grad():
                    RC.corr_lookup_ref(coords, f1, f2, 4, store=store)

            def ref_fb():
                a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
                (RC.corr_lookup_ref(coords, a, b, 4, store=store) * cot).sum().backward()

            for leg, hip, ref in (("pyramid_build", hip_build, None), ("lookup_fwd", hip_fwd, ref_fwd), ("pyramid_lookup_fwd_bwd", hip_fb, ref_fb)):
                ref = ref if allpairs else None
                th, tr = [], []
                for i in range(args.warmup + args.iters):
                    a = timed(hip)
                    c = timed(ref) if ref else None
                    if i >= args.warmup:
                        th.append(a)
                        if ref:
                            tr.append(c)
                rec = {"hip_ms": round(statistics.median(th), 4), "hip_ms_min_max": [round(min(th), 4), round(max(th), 4)],
                       "hip_peak_mb": round(peak_of(hip) / 1e6, 1)}
                if ref:
                    rec.update(allpairs_ms=round(statistics.median(tr), 3), allpairs_peak_mb=round(peak_of(ref) / 1e6, 1),
                               speedup=round(statistics.median(tr) / statistics.median(th), 1))
                entry["legs"][f"{dt}_{leg}"] = rec
                print(size, dt, leg, rec, flush=True)
            del pyr
        result["sizes"][size] = entry
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
