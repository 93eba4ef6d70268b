"""Settled SCF cycles of a bench trace, launch by launch, AVERAGED: cycle_means.py <..._kernel_trace.csv> [cycles]

From `rocprofv3 --kernel-trace --output-format csv -- python bench.py --steps 20 --warmup 5`: the last `cycles`
(default 20: the timed ones) intervals between consecutive J/K kernel launches that have the launch sequence of the
last one.  Prints, in the format of cycle_gaps.py, the mean gap before and the mean duration of every launch of the
cycle, then the settled period: the median start-to-start time of consecutive J/K launches (all in us)."""
import csv
import re
import statistics
import sys


def short(n):
    return n.replace("(anonymous namespace)::", "").replace("void ", "")[:50]


def main():
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(sys.argv[1]))]
    want = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows.sort(key=lambda r: r[1])
    idx = [i for i, r in enumerate(rows) if re.search(r"jk_(s4|m4|m8|sym|dense)_kernel", r[0])]
    cycles = [rows[a:b + 1] for a, b in zip(idx[:-1], idx[1:])]  # (each ends with the next cycle's J/K launch)
    names = [short(r[0]) for r in cycles[-1]]
    same = [c for c in cycles if [short(r[0]) for r in c] == names][-want:]
    for k, name in enumerate(names):
        gap = statistics.mean((c[k][1] - c[k - 1][2]) / 1e3 for c in same) if k else 0.0
        dur = statistics.mean((c[k][2] - c[k][1]) / 1e3 for c in same)
        print(f"  gap {gap:6.1f} dur {dur:7.1f} {name}")
    print("period", round(statistics.median((c[-1][1] - c[0][1]) / 1e3 for c in same), 3), "cycles", len(same))


if __name__ == "__main__":
    main()
