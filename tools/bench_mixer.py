"""The DCT-token MLP-Mixer at size, beside the same math in eager PyTorch, in one process on one GPU:
  * EncoderDCT and DecoderIDCT (vsrlab_amd.core.modules.dct_transforms; csrc/token_mixer.hip) against a grouped stride-ps conv2d /
    conv_transpose2d with the permutes that make and unmake the token layout;
  * the residual MLP along each of the three axes on its own, then one MixerBlock forward and forward + backward
    (vsrlab_amd.core.modules.mlp), against F.linear -> GELU -> F.linear -> add on a movedim view (tests/mixer_common.py).
    python tools/bench_mixer.py [--repeats 20] [--warmup 3] [--out profiles/mixer_bench.json]
Shapes: clips (8, 7, 3, 64, 64) and (2, 7, 3, 128, 128) at ps = 4, exp = 2.  The two sides of a pair are timed INTERLEAVED (HIP side,
torch side, HIP side, ...); times are medians of HIP-event intervals around one call each, fp32.  Algorithmic bytes: every activation
read once and written once (a backward: x and dy read, dx written; weights are noise); the fraction is of the 8 TB/s of the HBM's
specification.  Algorithmic FLOP of an axis MLP: 4 D hidden per position forward, 12 D hidden forward + backward (recomputed hidden
vector, d x, weight gradients); the fraction is of the 157.3 TFLOP/s of the fp32 vector unit.  Prints the JSON and writes it to --out."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
FP32_FLOP_PER_S = 157.3e12
SHAPES = ((8, 7, 3, 64, 64), (2, 7, 3, 128, 128))
PS, EXP = 4, 2


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


def row(name, shape, path, nbytes, flop, hip, stock):
    sec = hip[0] * 1e-3
    return {"case": name, "clip": list(shape), "path": path, "algorithmic_bytes": nbytes, "algorithmic_flop": flop,
            "hip_ms": round(hip[0], 4), "hip_ms_min_max": [round(hip[1], 4), round(hip[2], 4)],
            "hip_frac_of_8TBs": round(nbytes / sec / HBM_BYTES_PER_S, 4), "hip_frac_of_fp32_vector_peak": round(flop / sec / FP32_FLOP_PER_S, 4),
            "torch_ms": round(stock[0], 4), "torch_ms_min_max": [round(stock[1], 4), round(stock[2], 4)],
            "torch_over_hip": round(stock[0] / hip[0], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixer_bench.json"))
    a = ap.parse_args()
    if a.repeats < 10 or a.warmup < 3:
        ap.error("at least 10 repeats after 3 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixer needs an MI355X")
    import mixer_common as MC
    from vsrlab_amd.core.modules.dct_transforms import DecoderIDCT, EncoderDCT
    from vsrlab_amd.core.modules.mlp import MixerBlock
    from vsrlab_amd.core.token_ops import axis_mlp, axis_mlp_is_fused
    dev = torch.device("cuda:0")
    res = {"what": "per call, HIP-event time, fp32; the HIP modules beside the same math in eager PyTorch", "ps": PS, "exp": EXP,
           "repeats": a.repeats, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "fp32_vector_flop_per_s": FP32_FLOP_PER_S, "rows": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in SHAPES:
        b, t, c, h, w = shape
        p, ck = (h // PS) * (w // PS), c * PS * PS
        enc, dec = EncoderDCT(PS).to(dev), DecoderIDCT(3, PS, h, w).to(dev)
        w3 = enc.dct_conv.weight
        clip = torch.rand(*shape, device=dev, generator=g)
        with torch.no_grad():
            tok = enc(clip)
            act = 4 * clip.numel()
            th, ts = interleaved([lambda: enc(clip), lambda: MC.encoder(clip, w3, PS).contiguous()], a.warmup, a.repeats)
            res["rows"].append(row("EncoderDCT", shape, "block_dct_kernel", 2 * act, 2 * PS * PS * clip.numel(), th, ts))
            th, ts = interleaved([lambda: dec(tok), lambda: MC.decoder(tok, w3, PS, h // PS, w // PS)], a.warmup, a.repeats)
            res["rows"].append(row("DecoderIDCT", shape, "block_idct_kernel", 2 * act, 2 * PS * PS * clip.numel(), th, ts))

        block = MixerBlock(p, ck, t, EXP).to(dev)
        x = (torch.rand(b, t, p, ck, device=dev, generator=g) * 2 - 1).requires_grad_(True)
        cot = torch.rand(b, t, p, ck, device=dev, generator=g) * 2 - 1
        act = 4 * x.numel()
        params = {f"mixer.0.{n}": v for n, v in block.named_parameters()}

        def eager_block(inp):
            return MC.mixer(inp, params, 1).contiguous()

        def fwd_bwd(fn):
            def run():
                x.grad = None
                for q in block.parameters():
                    q.grad = None
                fn(x).backward(cot)
            return run

        flop_fwd = 0
        for axis, m in ((3, block.channels_mlp), (2, block.patches_mlp), (1, block.time_mlp)):
            d = x.shape[axis]
            ws = [m.mlp[0].weight, m.mlp[0].bias, m.mlp[2].weight, m.mlp[2].bias]
            fused = axis_mlp_is_fused(d, EXP * d)
            flop = 4 * d * EXP * d * (x.numel() // d)
            flop_fwd += flop
            with torch.no_grad():
                th, ts = interleaved([lambda: axis_mlp(x, axis, *ws), lambda: MC.axis_mlp(x, axis, *ws).contiguous()], a.warmup, a.repeats)
            inner = math.prod(x.shape[axis + 1:])
            res["rows"].append(row(f"axis MLP forward, axis {axis} (D = {d}, inner = {inner})", shape,
                                   "axis_mlp_kernel" if fused else "batched matmul", 2 * act, flop, th, ts))
        with torch.no_grad():
            th, ts = interleaved([lambda: block(x), lambda: eager_block(x)], a.warmup, a.repeats)
        res["rows"].append(row("MixerBlock forward", shape, "2 fused axes + matmul patch axis", 3 * 2 * act, flop_fwd, th, ts))
        th, ts = interleaved([fwd_bwd(block), fwd_bwd(eager_block)], a.warmup, a.repeats)
        res["rows"].append(row("MixerBlock forward + backward", shape, "2 fused axes + matmul patch axis", 3 * (2 + 3 + 2) * act, 3 * flop_fwd, th, ts))
        del clip, tok, x, cot, block
        torch.cuda.empty_cache()

    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
