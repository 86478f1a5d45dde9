"""The JPEG round trip at size: the fused HIP kernels (csrc/jpeg_degrade.hip) on the GPU, and beside them the reference's way -- a
PIL save / load per frame -- on this host's cores, measured in the same run.
    python tools/bench_jpeg.py [--shapes 14x540x960,14x135x240] [--quality 75] [--warmup 5] [--iters 20] [--calls 50] [--pil-iters 3] [--out profiles/jpeg_bench.json]
Default shapes: a 14-frame clip at 540 x 960 and at 135 x 240.  fp32 and bf16; a timed window is ``--calls`` calls back to back
between two hipEvents (one call is tens of microseconds: a window of one would measure the enqueue), per-call time = window /
calls, median of the windows after warm-up.  ``--pil-iters 0`` leaves the PIL loop out (for a run under a profiler).  The
kernel's own byte count per call: the input read once, the byte planes of the workspace (1.5 bytes per padded pixel) written once
and read once, the output written once; hbm_fraction is that count / time / 8 TB/s.  The PIL loop runs the frames of a CPU clip
over a pool of as many threads as this process may use (16 at most; PIL releases the interpreter lock while it encodes and
decodes), wall-clock median.  Nothing here is a gate: the file is where the numbers go."""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
DEFAULT_SHAPES = "14x540x960,14x135x240"


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


def pil_frame(frame, q):
    """one frame the reference's way: to_pil_image -> JPEG at quality q -> to_tensor"""
    from PIL import Image
    img = Image.fromarray(np.ascontiguousarray(frame.mul(255).byte().permute(1, 2, 0).numpy()), mode="RGB")
    with io.BytesIO() as buf:
        img.save(buf, format="JPEG", quality=q)
        buf.seek(0)
        with Image.open(buf) as im:
            im.load()
            a = np.asarray(im, dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated NxHxW")
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--pil-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py measures on an MI355X; no GPU found")
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    import ctypes
    dev = torch.device("cuda:0")
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    threads = max(1, min(cores, 16))
    try:
        from PIL import features
        have_pil = bool(features.check("jpg"))
    except Exception:
        have_pil = False
    q = args.quality
    result = {"what": "tools/bench_jpeg.py: JPEG round trip at quality %d; fused HIP kernels on an MI355X (hipEvent windows of %d calls, median per call) and the reference's "
                      "PIL loop on %d host threads (wall median); hbm_fraction = the kernel's own bytes / time / 8 TB/s" % (q, args.calls, threads),
              "tree": tree_hash(), "warmup": args.warmup, "iters": args.iters, "calls_per_window": args.calls, "pil_iters": args.pil_iters, "pil_threads": threads, "shapes": {}}
    for shape in args.shapes.split(","):
        N, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        clip = (0.5 + 0.35 * torch.sin(yy * 0.05 + xx * 0.03 + torch.rand(N, 3, 1, 1, generator=g) * 6.28)
                + 0.2 * (torch.rand(N, 3, H, W, generator=g) - 0.5)).clamp(0, 1)
        padded = N * (-(-H // 16) * 16) * (-(-W // 16) * 16)
        entry = {"N": N, "H": H, "W": W, "legs": {}}
        for dt, tdt, code in (("fp32", torch.float32, _lib.DT_F32), ("bf16", torch.bfloat16, _lib.DT_BF16)):
            x = clip.to(tdt).to(dev)
            L4 = ctypes.c_longlong * 4
            desc = _lib.JpegDesc(N, H, W, q, code, code, L4(*x.stride()), L4(*x.stride()))
            ws = int(_lib.load_jpeg().vsr_jpeg_workspace_bytes(ctypes.byref(desc)))
            planes = padded * 3 // 2
            moved = 2 * x.numel() * x.element_size() + 2 * planes
            def window():
                for _ in range(args.calls):
                    VF.jpeg_compress(x, q)

            ts = [timed(window) / args.calls for _ in range(args.warmup + args.iters)][args.warmup:]
            m = statistics.median(ts)
            rec = {"hip_ms": round(m, 4), "hip_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "workspace_bytes": ws,
                   "u8_plane_bytes": planes, "u8_bytes_per_padded_pixel": planes / padded, "bytes_moved_mb": round(moved / 1e6, 2),
                   "gb_per_s": round(moved / (m * 1e-3) / 1e9, 1), "hbm_fraction": round(moved / (m * 1e-3) / HBM_BYTES_PER_S, 4),
                   "frames_per_s": round(N / (m * 1e-3), 0)}
            entry["legs"][dt] = rec
            print(shape, dt, rec, flush=True)
        if have_pil and args.pil_iters > 0:
            with ThreadPoolExecutor(threads) as pool:
                tp = []
                for _ in range(1 + args.pil_iters):
                    t0 = time.perf_counter()
                    out = torch.stack(list(pool.map(lambda f: pil_frame(f, q), clip)))
                    tp.append((time.perf_counter() - t0) * 1e3)
            mp = statistics.median(tp[1:])
            same = float((out == VF.jpeg_compress(clip.to(dev), q).cpu()).float().mean())
            entry["pil_loop"] = {"ms": round(mp, 2), "frames_per_s": round(N / (mp * 1e-3), 0),
                                 "speedup_fp32": round(mp / entry["legs"]["fp32"]["hip_ms"], 1), "share_of_values_equal_to_hip": same}
        else:
            entry["pil_loop"] = None
        print(shape, "pil", entry["pil_loop"], flush=True)
        result["shapes"][shape] = entry
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
