"""The tables of profiles/attention_parity.md from the ATTN_PARITY lines that tests/test_attention_gpu.py prints:
    pytest tests/test_attention_gpu.py -m gpu -s > attn.log ; python tools/attention_parity_table.py attn.log"""
import re, sys, collections
rows = collections.OrderedDict()
for l in open(sys.argv[1]):
    m = re.search(r"ATTN_PARITY (\S+) (\S+) (\S+) l2_hip (\S+) l2_same (\S+) ratio (\S+) row_hip (\S+) row_same (\S+) ratio (\S+)", l)
    if m:
        name, dt, k = m.group(1, 2, 3)
        rows.setdefault((name, dt), {})[k] = tuple(float(x) for x in m.group(4, 5, 6, 7, 8, 9))
order = ["out", "lse", "dq", "dk", "dv", "dbias", "dqkv_self", "dqkv_mut", "dtable"]
out = []
for dt in ("fp32", "bf16"):
    if not any(d == dt for _, d in rows):
        continue
    out.append(f"\n### {dt} build (floor {'2e-4' if dt == 'fp32' else '1e-3'})\n")
    out.append("Per tensor: relative L2 against fp64, `HIP / same-precision`.  Then the worst per-tensor ratio `HIP / max(same, floor)` in relative L2 and")
    out.append("in the worst-row measure (max|err| over the tensor's max|ref|), with the tensor that has it and its two worst-row errors.\n")
    out.append("| case | " + " | ".join(["tensors (rel L2, HIP / same)", "worst L2 ratio", "worst row ratio", "row err HIP / same"]) + " |")
    out.append("|---|---|---|---|---|")
    for (name, d), t in rows.items():
        if d != dt: continue
        ks = [k for k in order if k in t]
        cell = "; ".join(f"{k} {t[k][0]:.1e} / {t[k][1]:.1e}" for k in ks)
        wl = max(ks, key=lambda k: t[k][2]); wr = max(ks, key=lambda k: t[k][5])
        out.append(f"| {name} | {cell} | {t[wl][2]:.2f} ({wl}) | {t[wr][5]:.2f} ({wr}) | {t[wr][3]:.1e} / {t[wr][4]:.1e} |")
    sub = [t for (n, d), t in rows.items() if d == dt]
    out.append(f"\nWorst over the {dt} cases: L2 ratio {max(v[2] for t in sub for v in t.values()):.2f}, row ratio {max(v[5] for t in sub for v in t.values()):.2f}, "
               f"largest HIP worst-row error {max(v[3] for t in sub for v in t.values()):.2e}.")
print("\n".join(out))
