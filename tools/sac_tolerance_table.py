"""Condenses the per-comparison lines tests/test_gpu_sac_policy.py prints (``pytest -s``; lines containing ``SACTOL``) into the
table kept in profiles/: per case the forward outputs and the loss values, per tensor name the worst case over all cases, and
every comparison that used more than half of its bound.

    python tools/sac_tolerance_table.py <pytest log> > profiles/sac_mlp_tolerance_table.txt
"""

import re
import sys

LINE = re.compile(r"SACTOL (\S+)\s+(\S+)\s+ref32-ref64 ([0-9.e+-]+)\s+ours-ref64 ([0-9.e+-]+)\s+bound ([0-9.e+-]+)")


def main(path):
    rows = [(m.group(1), m.group(2), float(m.group(3)), float(m.group(4)), float(m.group(5)))
            for m in map(LINE.search, open(path, errors="replace")) if m]
    shares = [l[l.index("SACTOL"):].strip() for l in open(path, errors="replace") if "excluded share" in l and "{" not in l]
    fmt = "{:30s} {:46s} {:>12s} {:>12s} {:>12s} {:>9s}"
    print(f"{len(rows)} comparisons; every one is |HIP module (MI355X, f32) - reference f64| against bound = max(4 x |reference f32 - reference f64|,")
    print("floor); outputs in the max-norm with floor 1e-6 max|x|, gradients in the 2-norm with floor 1e-6 ||g||")
    over = [r for r in rows if r[3] > r[4]]
    print(f"over the bound: {len(over)}")
    print()
    print("== forward outputs and loss values, per case ==")
    print(fmt.format("case", "tensor", "ref32-ref64", "ours-ref64", "bound", "ours/bnd"))
    for c, n, r, o, b in rows:
        if "/" not in n or n.startswith("q") or n.endswith(("/loss", "/entropy", "/d_actions", "losses")) or c in ("stale", "predict"):
            print(fmt.format(c, n, f"{r:.3e}", f"{o:.3e}", f"{b:.3e}", f"{o / b:.2f}" if b else "-"))
    print()
    print("== share of logprob elements excluded as ill-conditioned (1 - a_n^2 < 1e-3 on the f64 reference) ==")
    for s in dict.fromkeys(shares):
        print(s.replace("SACTOL ", ""))
    print()
    print("== every tensor, worst case over the cases ==")
    print(fmt.format("cases", "tensor", "max ref dev", "max ours", "", "max o/b"))
    worst = {}
    for c, n, r, o, b in rows:
        w = worst.setdefault(n, [0, 0.0, 0.0, 0.0])
        w[0] += 1
        w[1], w[2], w[3] = max(w[1], r), max(w[2], o), max(w[3], o / b if b else 0.0)
    for n, w in worst.items():
        print(fmt.format(str(w[0]), n, f"{w[1]:.3e}", f"{w[2]:.3e}", "", f"{w[3]:.2f}"))
    print()
    print("== comparisons that used more than half of their bound ==")
    for c, n, r, o, b in rows:
        if b and o > 0.5 * b:
            print(fmt.format(c, n, f"{r:.3e}", f"{o:.3e}", f"{b:.3e}", f"{o / b:.2f}"))


if __name__ == "__main__":
    main(sys.argv[1])
