"""The pixel losses and the resize adjoint at size, beside the torch compositions they replace, in one process on one GPU:
  * WL1Loss and rmse_loss, value + gradient w.r.t. the first argument (vsrlab_amd.core.losses; csrc/pixel_losses.hip), fp32 and bf16
    operands, at (1, 7, 3, 2160, 3840), against F.l1_loss / sqrt(F.mse_loss) under autograd;
  * the backward of core.utils.resize for 7 * 3 planes, 540 x 960 <-> 2160 x 3840 in both directions, against the backward of
    F.interpolate(bilinear, align_corners=False).
    python tools/bench_pixel_loss.py [--repeats 20] [--warmup 3] [--out profiles/pixel_loss_bench.json]
The two sides of a pair are timed INTERLEAVED (HIP side, torch side, HIP side, ...: boxes and their load differ);
times are medians of HIP-event intervals around one call each.  Algorithmic bytes: operands read once, gradient written once; the
fraction is of the 6.29 TB/s that a float4 copy measures on this chip.  Prints the JSON and writes it to --out."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BYTES_PER_S = 6.29e12


def interleaved(fns, warmup, repeats):
    """median, min, max milliseconds of each callable, one call of each per round"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts[k].append(t0.elapsed_time(t1))
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def row(name, algorithmic, hip, stock):
    frac = lambda ms: round(algorithmic / (ms * 1e-3) / COPY_BYTES_PER_S, 4)
    return {"case": name, "algorithmic_bytes": algorithmic,
            "hip_ms": round(hip[0], 4), "hip_ms_min_max": [round(hip[1], 4), round(hip[2], 4)], "hip_frac_of_copy_ceiling": frac(hip[0]),
            "torch_ms": round(stock[0], 4), "torch_ms_min_max": [round(stock[1], 4), round(stock[2], 4)],
            "torch_frac_of_copy_ceiling": frac(stock[0]), "torch_over_hip": round(stock[0] / hip[0], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1,7,3,2160,3840")
    ap.add_argument("--low", default="540,960", help="the low-resolution side of the resize pair; the high side is --shape's H, W")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_loss_bench.json"))
    a = ap.parse_args()
    if a.repeats < 10 or a.warmup < 3:
        ap.error("at least 10 repeats after 3 warm-ups")
    shape = tuple(int(s) for s in a.shape.split(","))
    low = tuple(int(s) for s in a.low.split(","))
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_loss needs an MI355X")
    from vsrlab_amd.core.losses import WL1Loss, rmse_loss
    from vsrlab_amd.core.utils import resize
    dev = torch.device("cuda:0")
    res = {"what": "value + gradient w.r.t. x of the pair losses, and the backward alone of the bilinear resize; per call, HIP-event time",
           "shape": list(shape), "repeats": a.repeats, "warmup": a.warmup, "copy_ceiling_bytes_per_s": COPY_BYTES_PER_S, "rows": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def fwd_bwd(fn, x, y):
        def run():
            x.grad = None
            fn(x, y).backward()
        return run

    l1 = WL1Loss()
    for dt in (torch.float32, torch.bfloat16):
        x = torch.rand(*shape, device=dev, generator=g).to(dt).requires_grad_(True)
        y = torch.rand(*shape, device=dev, generator=g).to(dt)
        algorithmic = 3 * x.numel() * x.element_size()
        name = str(dt).split(".")[-1]
        for tag, hip, stock in (("l1", l1, F.l1_loss), ("rmse", rmse_loss, lambda p, q: torch.sqrt(F.mse_loss(p, q)))):
            th, ts = interleaved([fwd_bwd(hip, x, y), fwd_bwd(stock, x, y)], a.warmup, a.repeats)
            res["rows"].append(row(f"{tag} {name}", algorithmic, th, ts))
        del x, y
        torch.cuda.empty_cache()

    planes = shape[:-2]
    high = shape[-2:]
    for src, dst in ((high, low), (low, high)):
        x = torch.rand(*planes, *src, device=dev, generator=g).requires_grad_(True)
        d = torch.rand(*planes, *dst, device=dev, generator=g)
        out_h = resize(x, dst)
        out_t = F.interpolate(x.reshape(-1, 1, *src), size=dst, mode="bilinear", align_corners=False)
        dt = d.reshape(out_t.shape)

        def hip_bwd():
            x.grad = None
            out_h.backward(d, retain_graph=True)

        def torch_bwd():
            x.grad = None
            out_t.backward(dt, retain_graph=True)

        th, ts = interleaved([hip_bwd, torch_bwd], a.warmup, a.repeats)
        res["rows"].append(row(f"resize adjoint {src[0]}x{src[1]} -> {dst[0]}x{dst[1]}", 4 * (x.numel() + d.numel()), th, ts))
        del x, d, out_h, out_t, dt
        torch.cuda.empty_cache()

    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
