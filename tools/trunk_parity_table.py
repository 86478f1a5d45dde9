"""The tables of profiles/trunk_parity.md from the TRUNK_RATIO lines that tests/test_trunk_gpu.py prints:
    pytest tests/test_trunk_gpu.py -m gpu -s > trunk.log ; python tools/trunk_parity_table.py trunk.log
One table per hook: rows = shape, columns = mid-channel width and build.  A cell of the rand family is the worst err / bound over the
hook's cases and outputs at that shape (the case and output that has it) and, after the slash, the worst share of the accumulation
term 2 K 2^-24 A alone; the cell of the grid family beside it counts the outputs that were held to exactness (bound 0) and came back
equal to the fp64 reference / its bf16 rounding."""
import collections
import re
import sys

cells = collections.OrderedDict()
for line in open(sys.argv[1]):
    m = re.search(r"TRUNK_RATIO hip (\w+)\[([0-9x]+),(\w+)((?:,[^\]]*)?)\] (\w+): worst err/bound (\S+) at .* accumulation share (\S+)", line)
    if not m:
        continue
    hook, shape, dt, opts, out, ratio, acc = m.groups()
    o = dict(kv.split("=") for kv in opts.lstrip(",").split(",") if "=" in kv)
    fam, width = o.pop("family", "rand"), o.pop("C", "64")
    rest = ",".join(f"{k}={v}" for k, v in o.items())
    cells.setdefault(hook, collections.OrderedDict()).setdefault(shape, {}).setdefault((int(width), dt), {}).setdefault(fam, []).append(
        (float(ratio), float(acc), rest, out))
for hook, shapes in cells.items():
    cols = sorted({k for per in shapes.values() for k in per}, key=lambda k: (-k[0], k[1]))
    print(f"\n### {hook}\n")
    print("| shape | " + " | ".join(f"C={w} {d}: rand err / bound (case, output) / accumulation share; grid exact" for w, d in cols) + " |")
    print("|---|" + "---|" * len(cols))
    for shape, per in shapes.items():
        row = []
        for k in cols:
            fams = per.get(k, {})
            cell = ""
            if "rand" in fams:
                r = max(fams["rand"])
                cell = f"{r[0]:.3f} ({r[2] or 'defaults'}, {r[3]}) / {max(v[1] for v in fams['rand']):.3f}"
            if "grid" in fams:
                ok = sum(1 for v in fams["grid"] if v[0] == 0.0)
                cell += f"; {ok} of {len(fams['grid'])}"
            row.append(cell)
        print(f"| {shape} | " + " | ".join(row) + " |")
    rand = [v for per in shapes.values() for fams in per.values() for v in fams.get("rand", [])]
    grid = [v for per in shapes.values() for fams in per.values() for v in fams.get("grid", [])]
    if rand:
        worst_acc = max(v[1] for v in rand)
        print(f"\nWorst err / bound over {hook}: {max(v[0] for v in rand):.3f}; worst accumulation share: {worst_acc:.3f}" +
              ("  **(above 0.5: the factor 2 is the only margin)**" if worst_acc > 0.5 else ""))
    if grid:
        print(f"Held to exactness: {len(grid)} outputs, {sum(1 for v in grid if v[0] == 0.0)} equal.")
