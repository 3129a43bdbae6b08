"""Compare the per-kernel CALL COUNTS of two `rocprofv3 --kernel-trace --stats` runs (their kernel_stats.csv), name by name.

    python tools/kernel_call_counts.py BEFORE_kernel_stats.csv AFTER_kernel_stats.csv

A refactor of the launch sequences (csrc/api.hip) must leave them equal: the same kernels, each launched as often.  Prints one line per
kernel whose count differs, then a summary; exit status 1 when anything differs.  Durations are not compared (two runs, two boxes)."""
import csv
import sys


def counts(path):
    with open(path, newline="") as f:
        return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}


def main(before, after):
    a, b = counts(before), counts(after)
    diff = [(n, a.get(n, 0), b.get(n, 0)) for n in sorted(set(a) | set(b)) if a.get(n, 0) != b.get(n, 0)]
    for n, x, y in diff:
        print(f"DIFFERS {x} -> {y}: {n[:160]}")
    print(f"{len(a)} kernel names / {sum(a.values())} launches before, {len(b)} / {sum(b.values())} after: "
          + ("call counts equal, name by name" if not diff else f"{len(diff)} names differ"))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
