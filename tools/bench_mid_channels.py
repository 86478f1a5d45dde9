"""One BasicVSR training step (forward + Charbonnier + backward + fused clip + Adam, bf16, full arena) at mid_channels 16, 32 and
64, in one process: the narrow engine (vsr_basicvsr_narrow_*) against the whole-path one.  Each step is timed with HIP events;
the median of --steps steps after --warmup is reported.  Writes profiles/<--out> (JSON) and prints it.

    python tools/bench_mid_channels.py [--steps 10 --warmup 3 --res-blocks 30 5 --mids 16 32 64 --out mid_channels.json]

For a kernel table of one width: run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python
tools/bench_mid_channels.py --mids 32 --res-blocks 30 --steps 2 --warmup 1 --out mid32_trace.json` and summarise
DIR/run_kernel_stats.csv with --stats-csv (profiles/mid32_kernel_stats.md)."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def step_times(mid, rb, n, t, h, w, steps, warmup, dev):
    import torch
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core.losses import CharbonnierLoss
    from vsrlab_amd.optim import FusedAdam
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    VF.set_arena_mode("full")
    torch.manual_seed(0)
    model = BasicVSR(mid, rb, 4, False, False).to(dev)
    model.compute_dtype = "bf16"
    opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=1.0)
    crit = CharbonnierLoss()
    g = torch.Generator(device="cpu").manual_seed(1234)
    lrs = torch.rand(n, t, 3, h, w, generator=g).to(dev)
    hr = torch.rand(n, t, 3, 4 * h, 4 * w, generator=g).to(dev)
    times, loss = [], None
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = crit(model(lrs), hr)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    out = {"mid": mid, "res_blocks": rb, "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
           "steps": steps, "loss": float(loss.detach())}
    del model, opt, lrs, hr
    torch.cuda.empty_cache()
    return out


def stats_table(path, top=12):
    """Top kernels of a rocprofv3 kernel_stats.csv (Name, Calls, TotalDurationNs, ...)."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    return [{"kernel": r["Name"][:120], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
             "avg_us": float(r["AverageNs"]) / 1e3, "share": float(r["TotalDurationNs"]) / total} for r in rows[:top]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mids", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--res-blocks", type=int, nargs="+", default=[30, 5])
    ap.add_argument("--shape", type=int, nargs=4, default=[1, 7, 540, 960], metavar=("N", "T", "H", "W"))
    ap.add_argument("--out", default="mid_channels.json", help="file name under profiles/")
    ap.add_argument("--stats-csv", default=None, help="summarise a rocprofv3 kernel_stats.csv instead of timing")
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps(stats_table(args.stats_csv), indent=1))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mid_channels needs an MI355X: there is no CPU timing")
    dev = torch.device("cuda:0")
    n, t, h, w = args.shape
    res = []
    for rb in args.res_blocks:
        for mid in args.mids:
            r = step_times(mid, rb, n, t, h, w, args.steps, args.warmup, dev)
            print(json.dumps(r), flush=True)
            res.append(r)
    by = {(r["res_blocks"], r["mid"]): r["median_ms"] for r in res}
    ratios = {f"rb{rb}": {f"mid{m}/mid64": by[(rb, m)] / by[(rb, 64)] for m in args.mids if (rb, 64) in by}
              for rb in args.res_blocks}
    doc = {"workload": f"BasicVSR(mid, rb, x4) bf16 fwd+Charbonnier+bwd+clip+Adam, full arena, clip {n}x{t}x{h}x{w}",
           "timing": "HIP events around each step, median of the timed steps", "results": res, "ratios": ratios}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", args.out), "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({"ratios": ratios}), flush=True)


if __name__ == "__main__":
    main()
