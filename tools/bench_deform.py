"""Flow-guided deformable convolution at size (VRT config 5, first stage: 15 frame pairs, 120 channels, 184 x 320, 8 groups):
forward and forward + backward, fp32 and bf16, on the HIP path against the pure-torch restatement of tests/deform_common.py on
the same GPU -- the only other way to compute the operator where torchvision is absent.  The two paths run interleaved in one
process; hipEvent timing, median.
    python tools/bench_deform.py [--shape 15,120,184,320] [--groups 8] [--warmup 3] [--iters 10] [--out profiles/deform_conv_bench.json]
The rate is over the algorithmic bytes: x + raw conv_offset output + flow + y (forward), plus dy, d x, d out, d flow (backward)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="15,120,184,320")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import deform_common as DC
    from vsrlab_amd import functional as VF
    N, C, H, W = (int(v) for v in args.shape.split(","))
    dg = args.groups
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, C, H, W, generator=g).to(dev)
    raw = (torch.randn(N, 27 * dg, H, W, generator=g) * 0.6).to(dev)
    flow = ((torch.rand(N, 2, H, W, generator=g) * 2 - 1) * 6).to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5).to(dev)
    b = (torch.randn(C, generator=g) * 0.1).to(dev)
    cot = torch.randn(N, C, H, W, generator=g).to(dev)
    pix = N * H * W
    bytes_fwd = pix * 4 * (C + 27 * dg + 2 + C)
    bytes_bwd = bytes_fwd + pix * 4 * (C + C + 27 * dg + 2)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (x, raw, flow, w, b)]

    def hip_fwd(dt):
        with torch.no_grad():
            VF.flow_guided_deform_conv(x, raw, flow, w, b, 10.0, compute_dtype=dt)

    def hip_fb(dt):
        xl, rl, fl, wl, bl = leaves()
        (VF.flow_guided_deform_conv(xl, rl, fl, wl, bl, 10.0, compute_dtype=dt) * cot).sum().backward()

    def ref_fwd(dt):                                  # one image at a time: the columns of 15 images are 3.8 GB
        store = DC.bf16_store if dt == "bf16" else None
        with torch.no_grad():
            for n in range(N):
                DC.flow_guided_deform_conv_ref(x[n:n + 1], raw[n:n + 1], flow[n:n + 1], w, b, 10.0, store=store)

    def ref_fb(dt):
        store = DC.bf16_store if dt == "bf16" else None
        xl, rl, fl, wl, bl = leaves()
        for n in range(N):
            y = DC.flow_guided_deform_conv_ref(xl[n:n + 1], rl[n:n + 1], fl[n:n + 1], wl, bl, 10.0, store=store)
            (y * cot[n:n + 1]).sum().backward()

    result = {"what": "tools/bench_deform.py: flow-guided deformable 3x3 convolution, HIP path vs the pure-torch restatement on the same "
                      "MI355X, interleaved, hipEvent median", "shape": [N, C, H, W], "deform_groups": dg, "tree": tree_hash(),
              "warmup": args.warmup, "iters": args.iters, "algorithmic_gb": {"fwd": bytes_fwd / 1e9, "fwd_bwd": bytes_bwd / 1e9}, "legs": {}}
    for dt in ("fp32", "bf16"):
        for leg, hip, ref, nbytes in (("fwd", hip_fwd, ref_fwd, bytes_fwd), ("fwd_bwd", hip_fb, ref_fb, bytes_bwd)):
            th, tr = [], []
            for i in range(args.warmup + args.iters):
                a, c = timed(lambda: hip(dt)), timed(lambda: ref(dt))
                if i >= args.warmup:
                    th.append(a)
                    tr.append(c)
            mh, mr = statistics.median(th), statistics.median(tr)
            result["legs"][f"{dt}_{leg}"] = {"hip_ms": round(mh, 3), "restatement_ms": round(mr, 3), "speedup": round(mr / mh, 2),
                                             "hip_gb_per_s": round(nbytes / mh / 1e6, 1), "hip_ms_min_max": [round(min(th), 3), round(max(th), 3)]}
            print(dt, leg, result["legs"][f"{dt}_{leg}"], flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
