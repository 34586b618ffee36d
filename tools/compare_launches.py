#!/usr/bin/env python3
"""Two rocprofv3 --kernel-trace outputs (directories, csv) of the same leg: are the launches the same?  Sorted by start time,
the sequence of (kernel name, grid, workgroup, LDS bytes) must be identical.  Prints the launch counts and "identical", or
the first launch that differs -- and then whether the sequences of every hardware queue, each sorted by start time and the
queues taken in the order of their first launch, are identical: launches of two queues (a copy beside a kernel) may start
in either order from run to run, launches of one queue may not.  Two traces of the SAME tree give the noise of a session.
usage: compare_launches.py <label> <dir of the parent's trace> <dir of this commit's trace>"""
import csv
import glob
import sys


def launches(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    shape = [c for c in rows[0] if c.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    queues = {}
    for r in rows:
        queues.setdefault(r.get("Queue_Id", "0"), []).append((r["Kernel_Name"],) + tuple(r[c] for c in shape))
    return [(r["Kernel_Name"],) + tuple(r[c] for c in shape) for r in rows], list(queues.values())


label, (a, qa), (b, qb) = sys.argv[1], launches(sys.argv[2]), launches(sys.argv[3])
if a == b:
    print("%-20s launches %6d / %6d   identical" % (label, len(a), len(b)))
    sys.exit(0)
i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
print("%-20s launches %6d / %6d   order differs from launch %d on; per queue (%d / %d queues): %s"
      % (label, len(a), len(b), i, len(qa), len(qb), "identical" if qa == qb else "DIFFERENT"))
for name, s in (("parent", a), ("this", b)):
    print("   %-7s %s" % (name, (s[i][0][:60],) + s[i][1:] if i < len(s) else None))
sys.exit(0 if qa == qb else 1)
