"""The tables of profiles/hr_tail_parity.md from the HR_TAIL_RATIO lines that tests/test_hr_tail_gpu.py prints:
    pytest tests/test_hr_tail_gpu.py -m gpu -s > hr_tail.log ; python tools/hr_tail_parity_table.py hr_tail.log
One table per hook: rows = shape, columns = build; a cell is the worst err / bound over the hook's cases and outputs at that shape
(the case and output that has it) and, after the slash, the worst share of the accumulation term 2 K 2^-24 A alone."""
import collections
import re
import sys

cells = collections.OrderedDict()
for line in open(sys.argv[1]):
    m = re.search(r"HR_TAIL_RATIO hip (\w+)\[([0-9x]+),(\w+)((?:,[^\]]*)?)\] (\w+): worst err/bound (\S+) at .* accumulation share (\S+)", line)
    if m:
        hook, shape, dt, opts, out, ratio, acc = m.groups()
        cells.setdefault(hook, collections.OrderedDict()).setdefault(shape, {}).setdefault(dt, []).append((float(ratio), float(acc), opts.lstrip(","), out))
for hook, shapes in cells.items():
    dts = [d for d in ("bf16", "fp32") if any(d in v for v in shapes.values())]
    print(f"\n### {hook}\n")
    print("| shape | " + " | ".join(f"{d}: err / bound (case, output) / accumulation share" for d in dts) + " |")
    print("|---|" + "---|" * len(dts))
    for shape, per in shapes.items():
        row = []
        for d in dts:
            if d not in per:
                row.append("")
                continue
            r = max(per[d])
            row.append(f"{r[0]:.3f} ({r[2] or 'defaults'}, {r[3]}) / {max(v[1] for v in per[d]):.3f}")
        print(f"| {shape} | " + " | ".join(row) + " |")
    worst_acc = max(v[1] for per in shapes.values() for vs in per.values() for v in vs)
    print(f"\nWorst accumulation share over {hook}: {worst_acc:.3f}" + ("  **(above 0.5: the factor 2 is the only margin)**" if worst_acc > 0.5 else ""))
