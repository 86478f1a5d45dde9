"""The tables of profiles/spynet_parity.md from the SPY_RATIO lines that tests/test_spynet_gpu.py prints:
    pytest tests/test_spynet_gpu.py -m gpu -s > spynet.log ; python tools/spynet_parity_table.py spynet.log
One table per hook: rows = shape (the 7x7 hooks: N x H x W; the planar launches: P or planes x h x w), columns = build.  A cell is the
worst err / bound over the hook's cases and outputs at that shape (the case and output that has it), then the worst share of the
accumulation term 2 K 2^-24 A alone and the worst share of the coordinate term alone; for the three 7x7 hooks `n of m` counts the grid
family's outputs that were held to exactness and came back equal to the fp64 reference / its bf16 rounding.  The last lines count the
tests, the outputs checked and the outputs held to exactness."""
import collections
import re
import sys

cells = collections.OrderedDict()
tests = None
for line in open(sys.argv[1]):
    m = re.search(r"^(\d+) passed", line) or re.search(r" (\d+) passed", line)
    if m:
        tests = line.strip().strip("= ")
    m = re.search(r"SPY_RATIO hip (\w+)\[([0-9x]+),(\w+)((?:,[^\]]*)?)\] (\w+): worst err/bound (\S+) at .* accumulation share (\S+), coordinate share ([0-9.a-z]+)"
                  r"(?:, equal (\d+) of (\d+))?", line)
    if not m:
        continue
    hook, shape, dt, opts, out, ratio, acc, coord, eq, of = m.groups()
    o = dict(kv.split("=") for kv in opts.lstrip(",").split(",") if "=" in kv)
    fam = o.pop("family", "rand")
    rest = ",".join(f"{k}={v}" for k, v in o.items())
    cells.setdefault(hook, collections.OrderedDict()).setdefault(shape, {}).setdefault(dt, {}).setdefault(fam, []).append(
        (float(ratio), float(acc), float(coord), rest, out, eq == of))
checked = exact = exact_ok = 0
for hook, shapes in cells.items():
    cols = sorted({k for per in shapes.values() for k in per})
    print(f"\n### {hook}\n")
    print("| shape | " + " | ".join(f"{d}: err / bound (case, output) / accumulation share / coordinate share; grid exact" for d in cols) + " |")
    print("|---|" + "---|" * len(cols))
    for shape, per in shapes.items():
        row = []
        for k in cols:
            fams = per.get(k, {})
            cell = ""
            if "rand" in fams:
                r = max(fams["rand"])
                cell = f"{r[0]:.3f} ({r[3] or 'defaults'}, {r[4]}) / {max(v[1] for v in fams['rand']):.3f} / {max(v[2] for v in fams['rand']):.3f}"
            if "grid" in fams:
                cell += ("; " if cell else "") + f"{sum(1 for v in fams['grid'] if v[0] == 0.0 and v[5])} of {len(fams['grid'])}"
            row.append(cell)
        print(f"| {shape} | " + " | ".join(row) + " |")
    rand = [v for per in shapes.values() for fams in per.values() for v in fams.get("rand", [])]
    grid = [v for per in shapes.values() for fams in per.values() for v in fams.get("grid", [])]
    checked += len(rand) + len(grid)
    if rand:
        print(f"\nWorst err / bound over {hook}: {max(v[0] for v in rand):.3f}; worst accumulation share: {max(v[1] for v in rand):.3f}; "
              f"worst coordinate share: {max(v[2] for v in rand):.3f}")
    if grid:
        ok = sum(1 for v in grid if v[0] == 0.0 and v[5])
        exact, exact_ok = exact + len(grid), exact_ok + ok
        print(f"Held to exactness: {len(grid)} outputs, {ok} equal.")
print(f"\nOutputs checked: {checked}; held to exactness: {exact}, equal: {exact_ok}." + (f"  pytest: {tests}." if tests else ""))
