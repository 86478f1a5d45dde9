"""PSNR + SSIM of a batch at size: the fused HIP call (vsrlab_amd.functional.psnr_ssim: one pass, clamp inside) against the stock
PyTorch route the reference takes -- clamp, contiguous, then SSIM as depthwise Gaussian convolutions plus elementwise passes and
PSNR as its own pass (tests/metrics_common.py, fp32, same GPU), each metric ending in its own .item().
    python tools/bench_metrics.py [--shapes 14,3,2160,3840 32,3,1920,2560] [--repeats 10] [--warmup 3] [--out profiles/metrics_bench.json]
Times are medians of HIP-event intervals.  Prints the JSON and writes it to --out."""
import argparse
import glob
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BYTES_PER_S = 8e12


def bench_step_ms():
    """ms_per_step of the newest committed BENCH_r*.json (bench.py's own result line) and that file's name."""
    files = sorted(glob.glob(os.path.join(ROOT, "BENCH_r*.json")), key=lambda p: int(re.search(r"_r(\d+)", p).group(1)))
    if not files:
        return None, None
    with open(files[-1]) as f:
        tail = json.load(f)["run"]["stdout_tail"]
    return float(json.loads(tail.splitlines()[0])["ms_per_step"]), os.path.basename(files[-1])


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["14,3,2160,3840", "32,3,1920,2560"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--no-stock", action="store_true", help="time the fused call alone (for a profiler run)")
    a = ap.parse_args()
    if a.repeats < 10 or a.warmup < 3:
        ap.error("at least 10 repeats after 3 warm-ups")
    import metrics_common as MC
    from vsrlab_amd import functional as VF
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs an MI355X")
    dev = torch.device("cuda:0")
    step_ms, step_file = bench_step_ms()
    res = {"what": "PSNR + SSIM (piqa defaults) of clamp(sr, 0, 1) against hr, fp32, per call incl. the device-to-host copy of the results",
           "repeats": a.repeats, "warmup": a.warmup, "bench_step": {"ms_per_step": step_ms, "from": step_file}, "shapes": []}

    for text in a.shapes:
        shape = tuple(int(s) for s in text.split(","))
        g = torch.Generator(device=dev).manual_seed(0)
        sr = torch.rand(*shape, device=dev, generator=g) * 1.4 - 0.2
        hr = torch.rand(*shape, device=dev, generator=g)

        def fused():
            r = VF.psnr_ssim(sr, hr, clamp=(0.0, 1.0))
            both = torch.stack([(10 * torch.log10(1 / (r.mse + 1e-8))).mean(), r.ssim.mean()]).cpu()
            return both[0].item(), both[1].item()

        def stock():
            x, y = sr.detach().clamp(0, 1).contiguous(), hr.detach().contiguous()
            return MC.psnr(x, y).mean().item(), MC.ssim(x, y).mean().item()

        f_ms, f_lo, f_hi, f_out = timed(fused, a.warmup, a.repeats)
        algorithmic = 8 * sr.numel()
        row = {"shape": list(shape), "fused_ms": round(f_ms, 4), "fused_ms_min_max": [round(f_lo, 4), round(f_hi, 4)],
               "algorithmic_bytes": algorithmic, "fused_frac_of_8TBs": round(algorithmic / (f_ms * 1e-3) / PEAK_BYTES_PER_S, 4),
               "fused_psnr_ssim": list(f_out)}
        if not a.no_stock:
            s_ms, s_lo, s_hi, s_out = timed(stock, a.warmup, a.repeats)
            row.update(stock_ms=round(s_ms, 4), stock_ms_min_max=[round(s_lo, 4), round(s_hi, 4)], stock_over_fused=round(s_ms / f_ms, 2),
                       stock_psnr_ssim=list(s_out))
            if step_ms:
                row.update(stock_share_of_bench_step=round(s_ms / step_ms, 4), fused_share_of_bench_step=round(f_ms / step_ms, 5))
        res["shapes"].append(row)
        del sr, hr
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
