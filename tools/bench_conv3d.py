"""The strided Conv3d modules at size, beside the reference's own composition (``F.conv3d`` between transposes + ``pixel_shuffle``, i.e.
MIOpen, as tests/conv3d_common.py restates it), in one process on one GPU:
  * ConvST(64, 64) and PixelShufflePack3D(64, 64, 2) on (2, 7, 64, 180, 320);
  * VRT's Upsample(4, 64) on (1, 64, 6, 64, 64);
each forward and forward + backward, in bf16 and in fp32.
    python tools/bench_conv3d.py [--seconds 1.0] [--warmup 3] [--out profiles/conv3d_bench.json]
GPU only: without a device it fails, and there is no fallback.  The two sides of a pair are timed INTERLEAVED (HIP side, torch side,
HIP side, ...) with device events around one call each, after a warm-up per shape, until each side has run for --seconds at least
(10 rounds at least).  Recorded per leg: median, minimum, maximum and the quartile spread of the rounds.  Algorithmic bytes of a
layer: its input read and its output written once, forward; backward: x and dy read, dx written (weights are noise).  Algorithmic
FLOP: 2 Cin Cout taps per output position forward, three times that forward + backward.  From these the file states the achieved
TB/s and TFLOP/s and which of the two bounds (8 TB/s; 2516 TFLOP/s dense bf16, 157.3 TFLOP/s fp32 on the matrix cores) is the
binding one.  Prints the JSON and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
PEAK_FLOP_PER_S = {"bf16": 2516e12, "fp32": 157.3e12}
# name -> (class, constructor arguments, input shape, layers as (Cin, Cout, taps, then output positions, input elements and output
# elements, each relative to the module's input))
CASES = {
    "ConvST(64,64)": ("ConvST", (64, 64), (2, 7, 64, 180, 320), [(64, 64, 9, 1, 1, 1), (64, 64, 3, 1, 1, 1)]),
    "PixelShufflePack3D(64,64,2)": ("PixelShufflePack3D", (64, 64, 2), (2, 7, 64, 180, 320), [(64, 256, 9, 1, 1, 4), (256, 256, 3, 1, 4, 4)]),
    "Upsample(4,64)": ("Upsample", (4, 64), (1, 64, 6, 64, 64), [(64, 256, 9, 1, 1, 4), (64, 256, 9, 4, 4, 16), (64, 64, 9, 16, 16, 16)]),
}


def work(shape, layers, esize, channels):
    """algorithmic (bytes forward, bytes forward + backward, FLOP forward) of a module; layers: (Cin, Cout, taps, positions, input
    elements, output elements), the last three relative to the module's input"""
    numel = 1
    for n in shape:
        numel *= n
    pos = numel // channels
    fwd = bwd = flop = 0
    for cin, cout, taps, p, n_in, n_out in layers:
        fwd += (n_in + n_out) * numel * esize
        bwd += (2 * n_in + n_out) * numel * esize
        flop += 2 * cin * cout * taps * p * pos
    return fwd, fwd + bwd, flop


def interleaved(fns, warmup, seconds):
    """milliseconds of each callable per round, one call of each per round, until every one has run for `seconds`"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    while min(sum(t) for t in ts) < seconds * 1e3 or len(ts[0]) < 10:
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts[k].append(t0.elapsed_time(t1))
    return [sorted(t) for t in ts]


def stats(t):
    n = len(t)
    return {"median_ms": round(t[n // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
            "quartile_spread_ms": round(t[(3 * n) // 4] - t[n // 4], 4), "rounds": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3d_bench.json"))
    a = ap.parse_args()
    if a.seconds < 1.0 or a.warmup < 1:
        ap.error("at least 1 s per leg after a warm-up")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv3d needs an MI355X")
    import conv3d_common as CC
    from vsrlab_amd.core.modules.conv import ConvST
    from vsrlab_amd.core.modules.upsampling import PixelShufflePack3D
    from vsrlab_amd.vsr.models.VRT.vrt import Upsample
    classes = {"ConvST": ConvST, "PixelShufflePack3D": PixelShufflePack3D, "Upsample": Upsample}
    dev = torch.device("cuda:0")
    res = {"what": "per call, device-event time; the HIP modules beside the reference's composition (F.conv3d between transposes + "
                   "pixel_shuffle: MIOpen) in the same process, legs interleaved",
           "device": torch.cuda.get_device_name(0), "seconds_per_leg": a.seconds, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "matrix_flop_per_s": PEAK_FLOP_PER_S, "rows": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (cls, args, shape, layers) in CASES.items():
        for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
            torch.manual_seed(0)
            model = classes[cls](*args).to(dev)
            x = (torch.rand(*shape, device=dev, generator=g) * 2 - 1).to(dtype).requires_grad_(True)
            # the composition's weights in the activation dtype, as autocast would hand them to MIOpen
            leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in model.named_parameters()}
            CC.MODULE_CASES["_bench"] = (cls, args, shape)

            def ref(inp):
                return CC.module_forward("_bench", inp, leaves)

            with torch.no_grad():
                cot = torch.rand_like(model(x)) * 2 - 1

            def fwd_bwd(fn, params):
                def run():
                    x.grad = None
                    for q in params:
                        q.grad = None
                    fn(x).backward(cot)
                return run

            b_fwd, b_all, flop = work(shape, layers, x.element_size(), 64)
            with torch.no_grad():
                legs = {"forward": (interleaved([lambda: model(x), lambda: ref(x)], a.warmup, a.seconds), b_fwd, flop)}
            legs["forward + backward"] = (interleaved([fwd_bwd(model, list(model.parameters())), fwd_bwd(ref, list(leaves.values()))],
                                                      a.warmup, a.seconds), b_all, 3 * flop)
            for leg, ((th, ts), nbytes, nflop) in legs.items():
                hip, stock = stats(th), stats(ts)
                sec = hip["median_ms"] * 1e-3
                t_mem, t_flop = nbytes / HBM_BYTES_PER_S, nflop / PEAK_FLOP_PER_S[tag]
                slower = hip["median_ms"] - stock["median_ms"] > max(hip["quartile_spread_ms"], stock["quartile_spread_ms"])
                res["rows"].append({"case": name, "input": list(shape), "dtype": tag, "leg": leg, "algorithmic_bytes": nbytes,
                                    "algorithmic_flop": nflop, "bound": "memory" if t_mem >= t_flop else "compute",
                                    "bound_ms": round(max(t_mem, t_flop) * 1e3, 4), "hip": hip, "miopen_composition": stock,
                                    "hip_TB_per_s": round(nbytes / sec / 1e12, 3), "hip_TFLOP_per_s": round(nflop / sec / 1e12, 2),
                                    "hip_frac_of_bound": round(max(t_mem, t_flop) / sec, 4),
                                    "composition_over_hip": round(stock["median_ms"] / hip["median_ms"], 3),
                                    "hip_slower_by_more_than_the_spread": bool(slower)})
                print(json.dumps(res["rows"][-1]), flush=True)
            del CC.MODULE_CASES["_bench"]
            del model, x, cot, leaves
            torch.cuda.empty_cache()

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
