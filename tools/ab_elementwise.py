"""Interleaved A/B of builds of the flow-warp kernels and the batched weight pack of csrc/elementwise.hip (the style of tools/ab_conv.py:
variants x rounds in ONE process, on random data).

    python tools/ab_elementwise.py rounds out.json name=lib_a.so name=lib_b.so ...      (library paths as given)

Every library is loaded side by side (ctypes); each round times `iters` launches of every library back to back, per kernel and dtype, at
the bench's LR size (8 x 180 x 320, 64 channels; the gather adjoint also at 32 and 16) over 4 rotating buffer sets: flow_warp forward,
its scatter adjoint, its flow gradient, the gather adjoint (flows in +-3: nothing is far, as for SPyNet's flows) and pack_multi_kernel
on 64 tensors of 64 x 64 x 3 x 3.  Prints and stores the median and the minimum per launch in microseconds."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = ctypes.c_void_p
BF16, F32 = 1, 0


class PackDesc(ctypes.Structure):                    # VsrPackDesc, csrc/kernels.h
    _fields_ = [("w", P), ("dst", P), ("total", ctypes.c_int), ("blk0", ctypes.c_int)] + \
               [(k, ctypes.c_short) for k in ("KK", "RP", "CPd", "r_real", "c_real", "I_total", "i_off", "o_mul", "o_add")] + \
               [("mode", ctypes.c_ubyte), ("dtype", ctypes.c_ubyte)]


def main():
    from vsrlab_amd import _lib
    assert (_lib.DT_BF16, _lib.DT_F32) == (BF16, F32)
    rounds, out_path = int(sys.argv[1]), sys.argv[2]
    names, libs = zip(*[(a.split("=")[0], ctypes.CDLL(os.path.abspath(a.split("=")[1]))) for a in sys.argv[3:]])
    n, h, w, nsets, iters = 8, 180, 320, 4, 48
    dev = torch.device("cuda:0")
    st = P(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    flow = [(torch.rand(n, 2, h, w, device=dev, generator=g) * 6 - 3) for _ in range(nsets)]
    S = torch.zeros(n * h * w * 64, dtype=torch.int64, device=dev)      # the far accumulator: stays zero, the flows are near
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    legs = {}
    for dt, tdt, dn in ((F32, torch.float32, "fp32"), (BF16, torch.bfloat16, "bf16")):
        for C in (64, 32, 16):
            pm = lambda: [torch.randn(n, h, (w + 31) // 32, C // 8, 32, 8, device=dev, generator=g).to(tdt) for _ in range(nsets)]
            a, b, o = pm(), pm(), pm()
            legs[f"warp_bwd_gather_kernel<{dn}, {C}>"] = lambda lib, i, a=a, b=b, o=o, dt=dt, C=C: lib.vsr_debug_warp_bwd_gather_c(
                dt, P(a[i].data_ptr()), P(flow[i].data_ptr()), P(b[i].data_ptr()), P(S.data_ptr()), P(cnt.data_ptr()), P(o[i].data_ptr()), n, h, w, C, st)
            if C != 64:
                continue
            acc = torch.zeros(n, h, w, C, device=dev)
            df = torch.empty(n, 2, h, w, device=dev)
            legs[f"warp_fwd_kernel<{dn}>"] = lambda lib, i, a=a, o=o, dt=dt: lib.vsr_flow_warp_fwd_ex(
                dt, P(a[i].data_ptr()), P(flow[i].data_ptr()), P(o[i].data_ptr()), n, h, w, 64, 0, st)
            legs[f"warp_bwd_kernel<{dn}>"] = lambda lib, i, a=a, acc=acc, dt=dt: lib.vsr_flow_warp_bwd_ex(
                dt, P(a[i].data_ptr()), P(flow[i].data_ptr()), P(acc.data_ptr()), n, h, w, 64, 0, st)
            legs[f"warp_bwd_flow_kernel<{dn}>"] = lambda lib, i, a=a, b=b, df=df, dt=dt: lib.vsr_flow_warp_bwd_flow_ex(
                dt, P(a[i].data_ptr()), P(b[i].data_ptr()), P(flow[i].data_ptr()), P(df.data_ptr()), n, h, w, 64, 0, st)
    wsrc = torch.randn(64, 64, 64, 3, 3, device=dev, generator=g)
    wdst = torch.empty(64, 9 * 64 * 64, dtype=torch.bfloat16, device=dev)
    descs = (PackDesc * 64)()
    for k in range(64):
        descs[k] = PackDesc(wsrc[k].data_ptr(), wdst[k].data_ptr(), 9 * 64 * 64, 0, 9, 64, 64, 64, 64, 64, 0, 1, 0, k & 1, BF16)
    legs["pack_multi_kernel"] = lambda lib, i: lib._Z21vsr_launch_pack_multiPK11VsrPackDesciP12ihipStream_t(descs, 64, st)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {k: {nm: [] for nm in names} for k in legs}
    for k, launch in legs.items():
        for i in range(200):                         # the clock settles under load
            assert launch(libs[i % len(libs)], i % nsets) == 0, k
        torch.cuda.synchronize()
        for r in range(rounds):
            for nm, lib in zip(names, libs):
                for i in range(nsets):
                    launch(lib, i)
                e0.record()
                for i in range(iters):
                    launch(lib, i % nsets)
                e1.record()
                torch.cuda.synchronize()
                res[k][nm].append(e0.elapsed_time(e1) / iters * 1e3)
    assert int(cnt.item()) == 0, "a far source: the gather legs timed its atomics too"
    out = {k: {nm: {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2)} for nm, v in by.items()} for k, by in res.items()}
    for k, by in out.items():
        print(f"{k:36s} " + " | ".join(f"{nm} med {v['median_us']:8.2f} min {v['min_us']:8.2f} us" for nm, v in by.items()), flush=True)
    with open(out_path, "w") as f:
        json.dump({"shape": [n, h, w], "rounds": rounds, "iters": iters, "per_launch": out}, f, indent=1)


if __name__ == "__main__":
    main()
