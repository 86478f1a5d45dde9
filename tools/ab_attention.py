"""A/B of builds of csrc/window_attention.hip in ONE process (the style of tools/ab_elementwise.py): bit identity first, then time.

    python tools/ab_attention.py rounds out.json parent=lib_a.so parent2=copy_of_lib_a.so new=lib_b.so

Every library is loaded side by side (ctypes); `parent2` is a second copy of the parent's file under another name.

Part 1, bit identity (`parent` against `new`): every case of MATRIX and BIG of tests/test_attention_gpu.py and its Nq = 160 forward case,
fp32 and bf16, through tests/attention_common.run_hip on the same seeded inputs.  out, lse, dq, dk, dv must be equal bit for bit; dbias
too where B = 1 (every address then receives one non-zero add in either kernel family, so the atomics' order cannot matter; for B > 1 the
suite's fp64 criterion is the check).  The first difference ends the run with a non-zero status, before any timing.

Part 2, time per launch: the config-5 stage shape of tools/bench_attention.py (7360 windows x 128 tokens, 6 heads, head_dim 20, bias +
packed mask), the 64-token mutual shape without bias, and for the per-(window, head) kernels N = 192 self, N = 256 self and the N = 384
window's mutual attention (Nq = Nk = 192) at the window counts the same 16 x 184 x 320 clip gives windows of depth 3, 4 and 6; forward and
backward, both element types.  After a warm-up, each round times `iters` launches of every library back to back over 3 rotating buffer
sets.  Per leg the noise is the larger of |median(parent) - median(parent2)| and half the interquartile range of parent's rounds; the leg
passes if median(new) <= max(median(parent), median(parent2)) + noise."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NSETS = 3


def bit_identity(parent, new, dev):
    import attention_common as AC
    from test_attention_gpu import BIG, MATRIX
    nq160 = AC.Case("g8-fwd-nq160", 5, 3, 20, 192, 160, 128, 32, 64, 0, mask="dense", nW=2, Nm=192, wide=True, seed=40)
    rows = []
    for c, backward in [(c, True) for c in MATRIX + BIG] + [(nq160, False)]:
        qkv, dout, bias, mask = AC.make_case(c)
        for dtype in ("fp32", "bf16"):
            a = AC.run_hip(c, qkv, dout, bias, mask, dtype, dev, backward=backward, lib=parent)
            b = AC.run_hip(c, qkv, dout, bias, mask, dtype, dev, backward=backward, lib=new)
            keys = [k for k in ("out", "lse", "dq", "dk", "dv") if k in a] + (["dbias"] if c.B == 1 and "dbias" in a else [])
            assert set(a) == set(b)
            for k in keys:
                if not torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)):
                    n = int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum())
                    print(f"AB_ATTN DIFFERENT {c.name} {dtype} {k}: {n} of {a[k].numel()} elements", flush=True)
                    sys.exit(1)
            rows.append({"case": c.name, "dtype": dtype, "equal": keys})
            print(f"AB_ATTN equal {c.name} {dtype} {' '.join(keys)}", flush=True)
    return rows


def legs(dev):
    """Yields (name, forward launch, backward launch); a launch is (lib, buffer set) -> status."""
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    from vsrlab_amd._lib import AttnDesc
    P, st = VF._ptr, VF._stream()
    g = torch.Generator(device=dev).manual_seed(0)
    nW = 920
    #        name           B     N   Nq  q0  heads hd  bias   mask
    shapes = [("p128-cfg5", 7360, 128, 128, 0, 6, 20, True, "packed"),
              ("p64-mutual", 7360, 128, 64, 64, 6, 20, False, "packed"),
              ("g12-self-192", 5520, 192, 192, 0, 6, 20, True, "dense"),
              ("g16-self-256", 3680, 256, 256, 0, 6, 20, True, "dense"),
              ("g12-mutual-384", 2760, 384, 192, 192, 6, 20, False, "dense")]
    for name, B, N, Nq, q0, heads, hd, has_bias, mform in shapes:
        C = heads * hd
        dense = torch.where(torch.rand(nW, N, N, device=dev, generator=g) < 0.3, -100.0, 0.0)
        if mform == "packed":
            m = torch.empty(nW, N, N // 32, dtype=torch.int32, device=dev)
            assert _lib.load().vsr_mask_pack(P(dense), P(m), nW, N, st) == 0
        else:
            m = dense
        bias = torch.randn(heads, Nq, Nq, device=dev, generator=g) if has_bias else None
        dbias = torch.zeros_like(bias) if has_bias else None
        for dn, tdt, dt in (("bf16", torch.bfloat16, VF.DT_BF16), ("fp32", torch.float32, VF.DT_F32)):
            d = AttnDesc(B, N, heads, hd, q0, 0, 0, Nq, Nq, C, 0, nW, N, hd ** -0.5, dt, int(mform == "packed"), -100.0 if mform == "packed" else 0.0)
            qkv = [torch.randn(B, N, 3, heads, hd, device=dev, generator=g).to(tdt) for _ in range(NSETS)]
            do = [torch.randn(B, N, C, device=dev, generator=g).to(tdt) for _ in range(NSETS)]
            o = [torch.empty(B, N, C, dtype=tdt, device=dev) for _ in range(NSETS)]
            dqkv = [torch.zeros_like(t) for t in qkv]
            lse = [torch.empty(B, heads, Nq, device=dev) for _ in range(NSETS)]
            delta = [torch.empty(B, heads, Nq, device=dev) for _ in range(NSETS)]
            fwd = lambda lib, i, d=d, qkv=qkv, o=o, lse=lse, bias=bias, m=m: lib.vsr_window_attention_fwd(
                ctypes.byref(d), P(qkv[i]), P(bias), P(m), P(o[i]), P(lse[i]), st)
            bwd = lambda lib, i, d=d, qkv=qkv, do=do, lse=lse, delta=delta, dqkv=dqkv, bias=bias, dbias=dbias, m=m: lib.vsr_window_attention_bwd(
                ctypes.byref(d), P(qkv[i]), P(bias), P(m), P(do[i]), P(lse[i]), P(delta[i]), P(dqkv[i]), P(dbias), st)
            yield f"{name} {dn}", fwd, bwd


def time_legs(rounds, names, libs, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}
    for shape, fwd, bwd in legs(dev):
        for i in range(NSETS):                             # lse of every set, for the backward
            assert fwd(libs[0], i) == 0, shape
        for pname, launch in (("fwd", fwd), ("bwd", bwd)):
            leg = f"{shape} {pname}"
            for i in range(12):                            # the clock settles under load
                assert launch(libs[i % len(libs)], i % NSETS) == 0, leg
            torch.cuda.synchronize()
            e0.record(); launch(libs[0], 0); e1.record()
            torch.cuda.synchronize()
            iters = max(3, min(48, int(40.0 / max(e0.elapsed_time(e1), 1e-3))))          # about 40 ms per measurement
            t = {nm: [] for nm in names}
            for r in range(rounds):
                for nm, lib in zip(names, libs):
                    e0.record()
                    for i in range(iters):
                        launch(lib, i % NSETS)
                    e1.record()
                    torch.cuda.synchronize()
                    t[nm].append(e0.elapsed_time(e1) / iters * 1e3)
            med = {nm: float(np.median(v)) for nm, v in t.items()}
            q1, q3 = np.percentile(t["parent"], [25, 75])
            noise = max(abs(med["parent"] - med["parent2"]), 0.5 * float(q3 - q1))
            ok = med["new"] <= max(med["parent"], med["parent2"]) + noise
            res[leg] = {"iters": iters, "noise_us": round(noise, 2), "verdict": "pass" if ok else "slower",
                        **{nm: {"median_us": round(med[nm], 2), "min_us": round(float(np.min(v)), 2)} for nm, v in t.items()}}
            print(f"AB_ATTN {leg:28s} " + " | ".join(f"{nm} med {med[nm]:9.2f} min {np.min(t[nm]):9.2f}" for nm in names) +
                  f" | noise {noise:7.2f} us  {res[leg]['verdict']}", flush=True)
        torch.cuda.empty_cache()
    return res


def main():
    rounds, out_path = int(sys.argv[1]), sys.argv[2]
    names, libs = zip(*[(a.split("=")[0], ctypes.CDLL(os.path.abspath(a.split("=")[1]))) for a in sys.argv[3:]])
    assert names == ("parent", "parent2", "new"), names
    dev = torch.device("cuda:0")
    equal = bit_identity(libs[0], libs[2], dev)
    per_launch = time_legs(rounds, names, libs, dev)
    with open(out_path, "w") as f:
        json.dump({"rounds": rounds, "nsets": NSETS, "bit_identical": equal, "per_launch": per_launch}, f, indent=1)
    slower = [k for k, v in per_launch.items() if v["verdict"] != "pass"]
    print("AB_ATTN slower legs:", slower or "none", flush=True)
    sys.exit(2 if slower else 0)


if __name__ == "__main__":
    main()
