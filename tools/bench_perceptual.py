"""PerceptualLoss (VGG19 features[:35], core/losses.py:29-64) at size: loss + d sr per call on the HIP engine against the stock
PyTorch path (F.conv2d / relu / max_pool2d under bf16 autocast, autograd to sr), keyed random weights.
    python tools/bench_perceptual.py [--shape 1,7,3,2160,3840] [--iters 3] [--dtype bf16] [--no-stock]
Prints one JSON line: ms per call, TFLOP/s (FLOPs counted below), peak memory, for both paths."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def vgg_flops(n, h, w):
    """Multiply-adds x 2 of one call: features[:35] on sr and on hr, plus the data gradient of every conv back to sr."""
    from vsrlab_amd.functional import VGG19_CONVS
    lv = {0: 0, 2: 0, 5: 1, 7: 1, 10: 2, 12: 2, 14: 2, 16: 2, 19: 3, 21: 3, 23: 3, 25: 3, 28: 4, 30: 4, 32: 4, 34: 4}
    fwd = 0
    for idx, co, ci in VGG19_CONVS:
        hh, ww = h, w
        for _ in range(lv[idx]):
            hh, ww = hh // 2, ww // 2
        fwd += 2 * 9 * co * ci * hh * ww
    return n * 3 * fwd                     # sr forward + hr forward + data gradient (same MACs as a forward)


def stock_call(sr, hr, params, weight):
    from perceptual_common import perceptual_terms
    x = sr.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = perceptual_terms(x, hr, params, weight).sum()
    loss.backward()
    return loss.detach(), x.grad


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        del out
    return sorted(ts)[len(ts) // 2] * 1e3, (torch.cuda.max_memory_allocated() - base) / 2**30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1,7,3,2160,3840")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--no-stock", action="store_true")
    a = ap.parse_args()
    shape = tuple(int(s) for s in a.shape.split(","))
    from perceptual_common import keyed_vgg_state_dict, param_list
    from vsrlab_amd import functional as VF
    dev = torch.device("cuda:0")
    params = [p.to(dev) for p in param_list(keyed_vgg_state_dict())]
    g = torch.Generator(device=dev).manual_seed(0)
    sr = torch.rand(*shape, device=dev, generator=g)
    hr = torch.rand(*shape, device=dev, generator=g)
    n, h, w = sr.numel() // (3 * shape[-2] * shape[-1]), shape[-2], shape[-1]
    flops = vgg_flops(n, h, w)

    def hip():
        x = sr.detach().requires_grad_(True)
        loss = VF.perceptual_loss(x, hr, params, 1e-2, compute_dtype=a.dtype)
        loss.backward()
        return loss.detach(), x.grad

    res = {"shape": list(shape), "dtype": a.dtype, "tflop_per_call": flops / 1e12}
    ms, peak = timed(hip, a.iters)
    res.update(hip_ms=ms, hip_tflops=flops / ms / 1e9, hip_peak_gib=peak,
               hip_chunk=VF.perceptual_chunk(n, h, w, VF.resolve_dtype(a.dtype), True))
    if not a.no_stock:
        ms, peak = timed(lambda: stock_call(sr, hr, params, 1e-2), a.iters)
        res.update(stock_ms=ms, stock_tflops=flops / ms / 1e9, stock_peak_gib=peak)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
