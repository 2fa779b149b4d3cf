"""Launch groups out of a rocprofv3 kernel trace (--kernel-trace --output-format csv):
    python scripts/kernel_groups.py <kernel_trace.csv> <name substring> [<name substring> ...]
For every kernel whose name contains one of the substrings, the launches are grouped by (kernel, grid size) and each group
prints calls, mean and min - max in us, longest group first.  Kernels whose launches share one grid (the BatchNorm passes'
capped grids) are split by duration instead: pass name:N to cut the sorted durations into runs of N launches (N = traced
steps), so the first run is "the longest launch of every step"."""
import csv
import sys
from collections import defaultdict


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    groups = defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        for w in wanted:
            sub, _, n = w.partition(":")
            if sub in name:
                key = (sub, name, "" if n else f"{r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']}", int(n or 0))
                groups[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for (sub, name, grid, n), d in groups.items():
        if n:
            d = sorted(d, reverse=True)
            for i in range(0, min(len(d), 4 * n), n):
                out.append((sub, name, f"rank {i // n}", d[i:i + n]))
        else:
            out.append((sub, name, f"grid {grid}", d))
    out.sort(key=lambda t: (t[0], -sum(t[3]) / len(t[3])))
    for sub, name, what, d in out:
        print(f"{sub:28s} {what:22s} calls {len(d):4d}  mean {sum(d) / len(d):8.1f} us  ({min(d):.1f} - {max(d):.1f})  {name[:70]}")


if __name__ == "__main__":
    main()
