#!/usr/bin/env python3
"""Headline benchmark: LR frames/sec, forward+backward, BasicVSR 4x, 540p 7-frame clips (BASELINE.json).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic clips per GPU (default: two 7-frame 540x960
clips; --clips 1 = the rounds 1-3 workload): HIP forward of
BasicVSR(64, 30, 4) on (2,7,3,540,960), fused Charbonnier loss + its gradient, HIP backward (all
weight gradients, written straight into the optimizer's flat gradient arena), ONE RCCL all-reduce of
that arena when N > 1, and the reference's update_weights tail (core/utils.py:270-280:
clip_grad_norm_(1) + Adam + zero_grad) as the fused HIP step -- kept inside the timed region so that
no training work is skipped.  `--optimizer torch --dp ddp` runs the reference's own stack instead
(torch.optim.Adam, DistributedDataParallel).  Inputs are resident in HBM before the timed region.
Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times --steps steps and prints the headline line (value, ms_per_step).  --full adds what is
measured behind the timed region: the trunk chains live inside one more step (roofline.in_step_live), the dominant kernel's
leg (roofline) and the CPU baseline (cpu_baseline; --no-cpu-baseline drops it).  --dump-outputs DIR writes, on rank 0, what
the last timed step computed (loss, a seeded sample of sr, the updated trainable parameters and Adam's first moment, float32 /
float64 .npy, < 64 MB in all); the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_BF16_PEAK_TF = 2500.0     # dense bf16
PROFILE_JSON = os.path.join("profiles", "r04_roofline.json")     # committed rocprofv3 summary of THIS command (profiles/README.md)


def tree_id():
    """What produced the binary that is running: sha1 over the kernel sources (vsrlab_amd/csrc, include) as they lie in this tree,
    plus the git HEAD that `build()` recorded next to the library (the GPU box has no .git).  profiles/summarize.py stamps the
    same sha1 into the committed profile summary, so replayed counters can be tied to -- or dropped for -- the running code."""
    import glob
    import hashlib
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(ROOT, "vsrlab_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "vsrlab_amd", "csrc", "*.h")) +
                    glob.glob(os.path.join(ROOT, "include", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    out = {"csrc_sha1": h.hexdigest()[:16]}
    try:
        out.update(json.load(open(os.path.join(ROOT, "vsrlab_amd", "lib", "BUILD_INFO.json"))))
    except Exception:
        pass
    return out


def algorithmic_bytes_per_frame(h, w, t, rb, es=2):
    """Layer-boundary-traffic convention of SURVEY.md 8(d) (fwd: read X + write Y per conv, skip read
    per ResidualConv; bwd: dY + saved X + dX per conv, skip grad; warps; SPyNet forward only)."""
    P = h * w
    fwd = bwd = 0.0

    def conv(cin, cout, pix, grad=True):
        nonlocal fwd, bwd
        fwd += (cin + cout) * pix * es
        if grad:
            bwd += (2 * cin + cout) * pix * es

    for _ in range(2):                       # two propagation directions
        conv(67, 64, P)
        for _ in range(rb):
            conv(64, 64, P)
            conv(64, 64, P)
            fwd += 64 * P * es               # skip read
            bwd += 64 * P * es               # skip grad
        fwd += (2 * 64 + 2) * P * es * (t - 1) / t     # flow_warp
        bwd += (3 * 64 + 2) * P * es * (t - 1) / t
    conv(128, 64, P)
    conv(64, 256, P)
    conv(64, 256, 4 * P)
    conv(64, 64, 16 * P)
    conv(64, 3, 16 * P)
    fwd += (3 + 48) * P * es                 # bilinear x4 skip
    hu, wu = -(-h // 32) * 32, -(-w // 32) * 32
    for lvl in range(6):                     # SPyNet, both directions, (t-1)/t pairs per frame
        pix = (hu >> (5 - lvl)) * (wu >> (5 - lvl))
        for ci, co in ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2)):
            fwd += 2 * (ci + co) * pix * es * (t - 1) / t
    return fwd + bwd


def flops_per_frame(h, w, t, rb):
    P = h * w
    f = 0.0
    trunk = 2 * (2 * 67 * 64 * 9 + rb * 2 * 2 * 64 * 64 * 9) * P
    recon = (2 * 128 * 64 + 2 * 64 * 256 * 9 + 4 * 2 * 64 * 256 * 9 + 16 * 2 * 64 * 64 * 9 + 16 * 2 * 64 * 3 * 9) * P
    f += 3 * (trunk + recon)                 # fwd + dgrad + wgrad
    hu, wu = -(-h // 32) * 32, -(-w // 32) * 32
    for lvl in range(6):
        pix = (hu >> (5 - lvl)) * (wu >> (5 - lvl))
        for ci, co in ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2)):
            f += 2 * 2 * ci * co * 49 * pix * (t - 1) / t
    return f


CHAIN_LAYERS, CHAIN_ITERS = 16, 12


def dominant_kernel_roofline(dev, h, w):
    """conv3x3_c64_chain_kernel (bf16): the residual-block convolutions of a frame -- 60 layers forward, 59 data gradients
    backward -- run as ONE launch each inside the engine (csrc/conv3x3_chain.hip); ~40 % of a step's kernel time.  The leg
    launches the same kernel through the C ABI (vsr_conv3x3_c64_chain_fwd) on CHAIN_LAYERS = 16 layers = 8 ResidualConv
    blocks over 17 distinct 66 MB images (1.13 GB: every launch re-reads and re-writes all of them, so no image survives in
    the 256 MiB Infinity Cache from one launch to the next; inside a launch layer l+1 reads what layer l has just written,
    exactly as in the engine), timed with HIP events on the stream it is launched on.  Algorithmic bytes per launch (SURVEY
    8d, per layer): X 64*P*2 + Y 64*P*2, + the identity 64*P*2 on every second layer.  The one-launch-per-layer kernel
    (conv3x3_c64_persist, what the engine ran before round 3's chain and still runs for every other 3x3 64->64 layer) is
    measured beside it, out of cache, under `per_layer_launch`."""
    from vsrlab_amd import functional as VF
    P = h * w
    g = torch.Generator(device="cpu").manual_seed(5)
    ws = [(torch.randn(64, 64, 3, 3, generator=g) * 0.04).to(dev) for _ in range(CHAIN_LAYERS)]
    bs = [torch.zeros(64, device=dev) for _ in range(CHAIN_LAYERS)]
    ch = VF.ResidualChainC64(ws, bs, 1, h, w, dev)
    ch.image(0).copy_(VF.to_pixel_major(torch.randn(1, 64, h, w, device=dev), VF.DT_BF16).reshape(-1))
    for _ in range(2):
        ch.launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CHAIN_ITERS):
        ch.launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / CHAIN_ITERS
    alg_bytes = sum((3 if l & 1 else 2) * 64 * P * 2 for l in range(CHAIN_LAYERS))
    flops = 2.0 * P * 64 * 576 * CHAIN_LAYERS
    gbs = alg_bytes / (ms * 1e-3) / 1e9
    out = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
           "traffic": None,
           "kernel": f"conv3x3_c64_chain_kernel<CHAIN_RELU> ({CHAIN_LAYERS} layers = {CHAIN_LAYERS // 2} ResidualConv blocks per launch, "
                     f"{CHAIN_LAYERS + 1} distinct 66 MB images)",
           "avg_us": round(ms * 1e3, 2), "avg_us_per_layer": round(ms * 1e3 / CHAIN_LAYERS, 2), "layers_per_launch": CHAIN_LAYERS,
           "algorithmic_bytes_per_launch": alg_bytes, "mfma_tflops": round(flops / (ms * 1e-3) / 1e12, 1),
           "mfma_frac": round(flops / (ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF, 4)}
    del ch
    out["per_layer_launch"] = per_layer_kernel_roofline(dev, h, w)
    # Everything above was measured in THIS process.  The PMC counters cannot be (rocprofv3 passes are separate runs): they are
    # replayed from the committed summary of the same command, under their own key and ONLY when that summary was produced from
    # the kernel sources that are running now; `traffic` stays null otherwise.
    tid = tree_id()
    try:
        pj = json.load(open(os.path.join(ROOT, PROFILE_JSON)))
        src = {"file": PROFILE_JSON, "csrc_sha1": pj.get("csrc_sha1"), "git_head": pj.get("git_head"),
               "measured_on": "the builder's gpurun box under rocprofv3, not in this run"}
        if pj.get("csrc_sha1") == tid["csrc_sha1"]:
            out["traffic"] = pj.get("hbm_bytes_per_launch")
            for k in ("in_step", "mfma_busy", "in_kernel_clock_GHz", "roofline_leg_avg_us_rocprof"):
                if k in pj:
                    src[k] = pj[k]
        else:
            src["stale"] = "kernel sources differ from the profiled ones: counters not replayed"
        out["counters_from"] = src
    except Exception:
        pass
    return out


def per_layer_kernel_roofline(dev, h, w, iters=48, nsets=8):
    """conv3x3_c64_persist_kernel (bf16, 3x3, 64->64), one launch per layer: the reconstruction convs and every 3x3 64->64
    layer outside the trunk chains.  Timed with HIP events on the stream it is launched on
    (torch's current stream), same shape and epilogues as inside the engine.  Algorithmic bytes per
    launch: X 64*P*2 + Y 64*P*2 (+ skip 64*P*2 on every second launch).
    The launches rotate through `nsets` = 8 distinct (x, skip, y) buffer sets = 1.6 GB at 540p, far beyond the 256 MiB
    Infinity Cache, so no operand of a launch is cache-resident from an earlier one (round-1 ADVICE: three 66 MB
    buffers were L3-resident and flattered the number)."""
    from vsrlab_amd import functional as VF
    xs = [VF.to_pixel_major(torch.randn(1, 64, h, w, device=dev), VF.DT_BF16) for _ in range(nsets)]
    rs = [VF.to_pixel_major(torch.randn(1, 64, h, w, device=dev), VF.DT_BF16) for _ in range(nsets)]
    ys = [torch.empty_like(xs[0]) for _ in range(nsets)]
    wgt = torch.randn(64, 64, 3, 3, device=dev) * 0.04
    b = torch.zeros(64, device=dev)
    for _ in range(3):
        VF.conv3x3_c64(xs[0], wgt, b, act=1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib = __import__("vsrlab_amd")._lib.load()
    import ctypes
    wpack = torch.empty(9 * 64 * 64, dtype=torch.bfloat16, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # weights are packed by the first call (w given); the timed launches pass w = NULL, so the events bracket
    # conv3x3_c64_persist_kernel launches only, alternating the two trunk epilogues (bias+ReLU / bias+skip)
    lib.vsr_conv3x3_c64_fwd(1, VF._ptr(xs[0]), VF._ptr(wgt), VF._ptr(b), VF._ptr(wpack), VF._ptr(ys[0]), VF._ptr(None), 1, 1, h, w, st)

    def launch(i):
        k = i % nsets
        lib.vsr_conv3x3_c64_fwd(1, VF._ptr(xs[k]), VF._ptr(None), VF._ptr(b), VF._ptr(wpack), VF._ptr(ys[k]), VF._ptr(rs[k] if i & 1 else None),
                                1 if not (i & 1) else 0, 1, h, w, st)
    for i in range(nsets):
        launch(i)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        launch(i)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    P = h * w
    alg_bytes = (64 + 64) * P * 2 + 0.5 * 64 * P * 2          # X + Y (+ skip read on every second launch)
    flops = 2.0 * P * 64 * 576
    gbs = alg_bytes / (ms * 1e-3) / 1e9
    out = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
           "traffic": None, "kernel": "conv3x3_c64_persist_kernel<ACT,RES,MASK> (bias+ReLU / bias+skip alternating, 8 rotating 66 MB buffer sets)",
           "avg_us": round(ms * 1e3, 2), "algorithmic_bytes_per_launch": alg_bytes, "mfma_tflops": round(flops / (ms * 1e-3) / 1e12, 1),
           "mfma_frac": round(flops / (ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF, 4)}
    return out


def chains_in_step_live(model, crit, lrs, hr, opt, args):
    """The dominant kernel INSIDE a step, live: one more forward + backward of the same clip behind the timed region (no collective, no
    optimizer step; rank 0 only) with every trunk-chain launch of the engine bracketed by a pair of HIP events on its stream
    (vsr_debug_chain_timing_begin / _read, csrc/conv3x3_chain.hip).  Algorithmic bytes per launch as in dominant_kernel_roofline plus the
    sign bits (8 bytes per pixel and ReLU layer); call-weighted over the step's launches."""
    import ctypes
    from vsrlab_amd import _lib
    lib = _lib.load()
    if not hasattr(lib, "vsr_debug_chain_timing_begin") or os.environ.get("VSRLAB_AMD_CHAIN", "1") == "0":
        return None
    if lib.vsr_debug_chain_timing_begin() != 0:
        return None
    sr = model(lrs)
    crit(sr, hr).backward()
    torch.cuda.synchronize()
    opt.zero_grad(set_to_none=(args.optimizer == "torch"))
    M = 64
    us, layers, var, px = (ctypes.c_float * M)(), (ctypes.c_int * M)(), (ctypes.c_int * M)(), (ctypes.c_longlong * M)()
    n = lib.vsr_debug_chain_timing_read(us, layers, var, px, M)
    if n <= 0:
        return None
    tot_b = tot_us = 0.0
    per = {"forward": [0.0, 0], "backward": [0.0, 0]}
    for i in range(n):
        P, L = float(px[i]), layers[i]
        skip, even = L // 2, L - L // 2
        tot_b += even * (2 * 64 * P * 2 + 8 * P) + skip * 3 * 64 * P * 2
        tot_us += us[i]
        k = "forward" if var[i] == 0 else "backward"
        per[k][0] += us[i]
        per[k][1] += L
    gbs = tot_b / (tot_us * 1e-6) / 1e9
    return {"what": "every conv3x3_c64_chain_kernel launch of one forward + backward behind the timed region, HIP events on its stream",
            "launches": n, "us_per_layer": {k: round(v[0] / v[1], 2) for k, v in per.items() if v[1]},
            "achieved": round(gbs, 1), "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4)}


def host_cores():
    """CPU share of this job: the affinity mask, capped at 16 (a 1-GPU box's share; os.cpu_count()
    reports the whole host and oversubscribing it makes oneDNN crawl)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


DUMP_SR_SAMPLES = 1 << 20          # sr is 1.4 GB at two 540p clips: a seeded sample of it
DUMP_MAX_ELEMS = 7_000_000         # per flat array (BasicVSR(64, 30) has 4.85 M trainable values, 6.29 M with train_flow)


def dump_outputs(path, loss, sr, model, opt):
    """What the last timed step handed its caller, as float .npy files under `path`: loss (float64), a fixed seeded sample of
    sr, the updated trainable parameters and Adam's exp_avg (both flat, in model.parameters() order; seeded samples past
    DUMP_MAX_ELEMS).  < 64 MB in all."""
    import numpy as np
    os.makedirs(path, exist_ok=True)

    def sample(x, k, seed):
        x = x.reshape(-1)
        if x.numel() <= k:
            return x
        idx = torch.randint(0, x.numel(), (k,), generator=torch.Generator().manual_seed(seed)).sort().values
        return x[idx.to(x.device)]

    params = [p for p in model.parameters() if p.requires_grad]
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_m = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in params])
    arrays = {"loss": loss.detach().double().reshape(1),
              "sr_sample": sample(sr, DUMP_SR_SAMPLES, 11),
              "params": sample(flat_p, DUMP_MAX_ELEMS, 12),
              "adam_exp_avg": sample(flat_m, DUMP_MAX_ELEMS, 12)}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a.cpu().numpy())
    log(f"outputs of the last timed step written to {path}: " + ", ".join(f"{k} {tuple(v.shape)}" for k, v in arrays.items()))


def cpu_baseline(h540, w540):
    """The oracle (CPU restatement of the reference, fp32, "port") on this box's host cores, on a bounded sample
    (BASELINE.md section 4): (i) BASELINE config 1 exactly (n=2, t=5, 64x64, rb=30) fwd+Charbonnier+bwd, best of 2
    after a warm-up; (ii) a 540x960 clip of TWO frames (n=1, t=2, rb=30) fwd+Charbonnier+bwd, ONE run -- the frame size the
    metric is quoted on, with SPyNet (both directions) and the two feature warps and their adjoints inside, as BASELINE.md
    section 4 planned (round 3 timed t=1: no flow path at all); a 7-frame clip needs > 113 GB of saved fp32 activations and
    minutes of CPU time, and the cost is linear in n*t*pixels.  value = (ii)'s LR frames/s."""
    from oracle import basicvsr_oracle as O
    cores = host_cores()
    torch.set_num_threads(cores)
    sd = O.keyed_state_dict(O.basicvsr_param_shapes(64, 30, 4))
    g = torch.Generator().manual_seed(0)
    lrs = torch.rand(2, 5, 3, 64, 64, generator=g)
    hr = torch.rand(2, 5, 3, 256, 256, generator=g)
    best = None
    for i in range(3):
        t0 = time.perf_counter()
        O.fwd_bwd(sd, lrs, hr)
        dt = time.perf_counter() - t0
        if i > 0:
            best = dt if best is None else min(best, dt)
    fps_c1 = 10.0 / best
    lrs = torch.rand(1, 2, 3, h540, w540, generator=g)
    hr = torch.rand(1, 2, 3, 4 * h540, 4 * w540, generator=g)
    t0 = time.perf_counter()
    O.fwd_bwd(sd, lrs, hr)
    dt540 = time.perf_counter() - t0
    return {"value": round(2.0 / dt540, 5), "unit": "LR frames/s", "cores": cores, "kind": "port",
            "sample": f"oracle fp32 fwd+Charbonnier+bwd, rb=30: (i) config 1 (n=2,t=5,64x64) best of 2 after a warm-up {best:.2f} s/step = "
                      f"{fps_c1:.2f} LR frames/s at 64x64 (= {fps_c1 * 64 * 64 / float(h540 * w540):.4f} per-pixel-normalised to {h540}x{w540}); "
                      f"(ii) one {h540}x{w540} clip of 2 frames (n=1,t=2: SPyNet both directions + feature warps included), one run: "
                      f"{dt540:.1f} s for 2 frames = value",
            "config1_frames_per_s": round(fps_c1, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--res-blocks", type=int, default=30)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--optimizer", default="fused", choices=["fused", "torch"],
                    help="fused: vsrlab_amd.optim.FusedAdam (clip + Adam over flat arenas); torch: torch.optim.Adam (no clipping), the round-1 step")
    ap.add_argument("--dp", default="flat", choices=["flat", "ddp"],
                    help="N > 1: flat = one all-reduce over the gradient arena (vsrlab_amd.parallel.FlatGradSync); ddp = torch DistributedDataParallel")
    ap.add_argument("--roofline-only", action="store_true", help="run only the dominant-kernel leg (for rocprofv3 PMC passes)")
    ap.add_argument("--train-flow", action="store_true", help="train_flow=True (conf/experiment/basic.yaml:7): SPyNet is differentiated too (need_backward = 2)")
    ap.add_argument("--clips", type=int, default=2,
                    help="7-frame clips per GPU and step (BASELINE configs[1] '7-frame clips' / configs[3] 'batch-of-clips'; the reference's per-rank "
                         "micro-batch is 8 clips, conf/experiment/basic.yaml:10,25-26).  Two fit one 288 GB GPU in the full arena since round 4 "
                         "(113 GiB per clip) and run ~2 %% faster per frame than one (same kernels on twice the tiles per launch, the trunk chains "
                         "image by image); --clips 1 is the round 1-3 workload")
    ap.add_argument("--arena", default="full", choices=["full", "diet"],
                    help="training workspace of the engine (VsrBasicVSRDesc.arena_mode): full = 113 GiB per clip, all-frames weight-gradient launches "
                         "(the headline configuration); diet = 65 GiB per clip (per-frame weight gradients, HR activations recomputed)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs behind the timed region: roofline.in_step_live, the dominant kernel's leg, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (loss, sr sample, parameters, Adam exp_avg)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.optimizer == "torch" and args.dp == "flat":
        args.dp = "ddp"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if args.roofline_only:
        leg = dominant_kernel_roofline(dev, args.height, args.width)
        leg["tree"] = tree_id()
        print(json.dumps(leg), flush=True)
        return
    dist = None
    use_dist = world > 1 or "RANK" in os.environ     # under torchrun even a 1-rank job takes the DDP / RCCL path
    if use_dist:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)      # "nccl" is RCCL on ROCm

    from vsrlab_amd.core.losses import CharbonnierLoss
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    from vsrlab_amd import functional as VF
    VF.set_arena_mode(args.arena)

    torch.manual_seed(0)
    model = BasicVSR(64, args.res_blocks, 4, False, args.train_flow).to(dev)
    model.compute_dtype = args.dtype
    net = model
    sync = None
    if args.optimizer == "fused":
        from vsrlab_amd.optim import FusedAdam
        # conf/train/optimizer/adam.yaml (lr 1e-4, betas (0.9, 0.99), eps 1e-8) + gradient_clip_val: 1 (conf/train/default.yaml:20)
        opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=1.0)
        if use_dist:
            from vsrlab_amd.parallel import FlatGradSync
            sync = FlatGradSync(opt.flat_grads, params=opt.flat_params, optimizer=opt)    # start-up broadcast + one all-reduce per step
    else:
        if use_dist:
            from torch.nn.parallel import DistributedDataParallel
            net = DistributedDataParallel(model, device_ids=[local_rank], gradient_as_bucket_view=True, broadcast_buffers=False)  # core/utils.py:147-151
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.99))
    crit = CharbonnierLoss()
    n, t, h, w = args.clips, args.frames, args.height, args.width
    # Two clips need 231 GiB of the GPU's 268.  A GPU that is not empty (another process, a smaller part) gets the rounds 1-3 workload
    # instead of an allocation failure in the first warm-up step; the line says so (config.clips_per_gpu, config.clips_note).
    clips_note = None
    if n > 1 and world == 1:
        free_b, _total_b = torch.cuda.mem_get_info(dev)
        need = n * 116.0 * 2 ** 30 * (h * w * t) / (540.0 * 960 * 7) * (args.res_blocks + 3) / 33.0
        if args.arena == "full" and args.dtype == "bf16" and free_b < need:
            clips_note = f"--clips {n} needs ~{need / 2 ** 30:.0f} GiB, {free_b / 2 ** 30:.0f} GiB free: ran 1 clip per GPU"
            log(clips_note)
            n = 1
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)             # one distinct clip per rank (weak scaling)
    lrs = torch.rand(n, t, 3, h, w, generator=g).to(dev)
    hr = torch.rand(n, t, 3, 4 * h, 4 * w, generator=g).to(dev)

    def step(keep_sr=False):
        sr = net(lrs)
        loss = crit(sr, hr)
        loss.backward()
        if sync is not None:
            sync.all_reduce()
        opt.step()
        opt.zero_grad(set_to_none=(args.optimizer == "torch"))
        return loss, (sr.detach() if keep_sr else None)

    for i in range(args.warmup):
        step()
        if rank == 0:
            torch.cuda.synchronize()
            log(f"warm-up step {i} done")
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    keep_last = args.dump_outputs is not None and rank == 0     # sr of the last step only: no step runs beside a kept one
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss, sr = step(keep_sr=keep_last and i == args.steps - 1)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    loss_val = float(loss.item())
    ms_per_step = elapsed / args.steps * 1e3
    if rank == 0:
        log(f"timed region: {ms_per_step:.1f} ms/step")
        if keep_last:
            dump_outputs(args.dump_outputs, loss, sr, model, opt)
            del sr
    frames_per_s = world * n * t * args.steps / elapsed

    if rank == 0:
        out = {
            "metric": "LR frames/sec fwd+bwd, BasicVSR 4x 540p 7-frame clip, 1->8 MI355X",
            "value": round(frames_per_s, 3), "unit": "LR frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic (torch.rand clips, random-init weights)",
            "config": {"workload": f"BasicVSR(mid=64,res_blocks={args.res_blocks},x4) fwd+Charbonnier+bwd+clip+Adam, "
                                   f"{h}x{w}->{4 * h}x{4 * w}, {t}-frame clip, {n} clip{'s' if n > 1 else ''} per GPU (BASELINE configs[1]{'/[3]' if world > 1 else ''})",
                       "clips_per_gpu": n, **({"clips_note": clips_note} if clips_note else {}), "frames": t, "lr_size": [h, w], "res_blocks": args.res_blocks,
                       "parallelism": (f"dp{world} (clip-level; " + ("one RCCL all-reduce of the flat gradient arena per step)" if sync is not None
                                                                        else "DDP grad all-reduce over RCCL)")) if world > 1 else "single GPU",
                       "optimizer_in_timed_region": "fused clip_grad_norm(1)+Adam (HIP)" if args.optimizer == "fused" else "torch.optim.Adam",
                       "arena": args.arena, "train_flow": bool(args.train_flow), "peak_hbm_GiB": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1)},
            "loss": round(loss_val, 6), "tree": tree_id(),
        }
        # the trunk chains hand tiles between workgroups inside a launch; a wait that timed out would have left wrong results behind
        from vsrlab_amd import functional as _VF
        out["config"]["trunk_chains"] = os.environ.get("VSRLAB_AMD_CHAIN", "1") != "0" and args.dtype == "bf16"
        if _VF.chain_timeouts() != 0:
            raise RuntimeError(f"vsrlab_amd: {_VF.chain_timeouts()} chain dependency waits timed out: the run is void")
        bpf = algorithmic_bytes_per_frame(h, w, t, args.res_blocks, 2 if args.dtype == "bf16" else 4)
        fpf = flops_per_frame(h, w, t, args.res_blocks)
        out["path_roofline"] = {"algorithmic_GB_per_frame": round(bpf / 1e9, 3), "TFLOP_per_frame": round(fpf / 1e12, 3),
                                "achieved_GBs_per_gpu": round(bpf * frames_per_s / world / 1e9, 1),
                                "hbm_frac": round(bpf * frames_per_s / world / 1e9 / HBM_PEAK_GBS, 4),
                                "achieved_TFLOPs_per_gpu": round(fpf * frames_per_s / world / 1e12, 1)}
        if args.full:
            # (not under stock DDP at world > 1: a backward outside its forward would meet the reducer's hooks)
            live = chains_in_step_live(model, crit, lrs, hr, opt, args) if args.dtype == "bf16" and (world == 1 or sync is not None) else None
            if args.dtype == "bf16":                             # the dominant kernel's leg: rank 0's GPU, after the timed region, at every N
                out["roofline"] = dominant_kernel_roofline(dev, h, w)
                log(f"dominant kernel: {out['roofline']['avg_us']} us")
                if live is not None:
                    out["roofline"]["in_step_live"] = live
            if world == 1 and not args.no_cpu_baseline:          # the CPU baseline: rank 0 at N = 1 only
                out["cpu_baseline"] = cpu_baseline(h, w)
        print(json.dumps(out), flush=True)
    if dist:
        # ranks 1..N-1 wait here while rank 0 runs its post-timing legs (in_step_live, the dominant kernel's leg) on its GPU:
        # nobody tears the process group down under a rank that is still working
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
