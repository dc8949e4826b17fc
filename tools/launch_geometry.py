#!/usr/bin/env python3
"""Launch geometry of two runs of the same workload, to show that a host-side change left every grid, block and LDS size alone
(the kernels of a grid-stride pass give the right answer on the wrong grid, so the tests cannot see it).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python ...        once per revision (kernel trace only)
    python tools/launch_geometry.py --compare BEFORE_kernel_trace.csv AFTER_kernel_trace.csv [--distinct]

Each trace is reduced to the multiset of (kernel name, grid x/y/z, workgroup x/y/z, LDS bytes) over its dispatches; --distinct
compares the sets of distinct tuples instead (for a workload whose number of dispatches depends on its data).  Exit code 1 when
they differ.  A path may be a directory: every *kernel_trace.csv below it is read (one per process of the run)."""
import csv
import sys
from collections import Counter
from pathlib import Path

FIELDS = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
          "LDS_Block_Size")


def geometry(path):
    """Counter of the (name, grid, workgroup, LDS) tuples of the dispatches of one trace file or directory of them"""
    path = Path(path)
    files = sorted(path.rglob("*kernel_trace.csv")) if path.is_dir() else [path]
    if not files:
        raise SystemExit(f"{path}: no *kernel_trace.csv")
    out = Counter()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                out[(row[FIELDS[0]],) + tuple(int(row[k]) for k in FIELDS[1:])] += 1
    return out


def main(argv):
    if len(argv) < 3 or argv[0] != "--compare":
        print(__doc__)
        return 2
    before, after = geometry(argv[1]), geometry(argv[2])
    distinct = "--distinct" in argv[3:]
    if distinct:
        before, after = Counter(set(before)), Counter(set(after))
    what = "distinct tuples" if distinct else "dispatches"
    print(f"before: {sum(before.values())} {what}, {len({k[0] for k in before})} kernels; "
          f"after: {sum(after.values())} {what}, {len({k[0] for k in after})} kernels")
    bad = 0
    for key in sorted(set(before) | set(after)):
        if before[key] != after[key]:
            bad += 1
            name, *geo = key
            print(f"  {before[key]:6d} -> {after[key]:6d}  grid {geo[0:3]} workgroup {geo[3:6]} lds {geo[6]}  {name[:120]}")
    print("launch geometry: " + (f"{bad} tuples differ" if bad else "equal"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
