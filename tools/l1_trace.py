#!/usr/bin/env python
"""Level-1 interval of a rocprofv3 --kernel-trace --memory-copy-trace run of bench.py: every kernel and copy of the LAST
step's level 1 in start order, with the gap in front of each (time in which neither a kernel nor a copy ran: the host was
waited for, or the next command had not been submitted yet), and the totals against the interval's wall time.
The interval starts at the end of the last level-0 kernel (k_l0_scale) and ends with the last event of the trace.
Usage: l1_trace.py <dir> [out.md]"""
import csv
import glob
import sys


def nm(r):
    return r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].replace("void ", "").strip()


def main(d, out=None):
    ev = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            g = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
            wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), nm(r), "%d x %d" % (g // max(1, wg), wg)))
    for f in glob.glob(d + "/**/*memory_copy_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r.get("Direction", r.get("Kind", "?")), ""))
    ev.sort()
    l0 = [i for i, e in enumerate(ev) if e[2] == "k_l0_scale"]
    i0 = l0[-1] + 1
    t_prev = ev[l0[-1]][1]
    t0 = t_prev
    lines = ["| # | kernel / copy | workgroups x threads | gap before us | us |", "|---:|---|---:|---:|---:|"]
    agg, busy, gaps = {}, 0.0, 0.0
    for k, (s, e, name, grid) in enumerate(ev[i0:]):
        gap = max(0.0, (s - t_prev) / 1e3)
        us = (e - s) / 1e3
        lines.append("| %d | %s | %s | %.1f | %.1f |" % (k, name, grid, gap, us))
        a = agg.setdefault(name, [0, 0.0])
        a[0] += 1
        a[1] += us
        busy += max(0.0, (e - max(s, t_prev)) / 1e3)
        gaps += gap
        t_prev = max(t_prev, e)
    lines += ["", "interval (end of the last k_l0_scale to the end of the last event): %.1f us; device busy: %.1f us; gaps: %.1f us; events: %d"
              % ((t_prev - t0) / 1e3, busy, gaps, len(ev) - i0), "", "| kernel / copy | count | total us |", "|---|---:|---:|"]
    for n, (c, us) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        lines.append("| %s | %d | %.1f |" % (n, c, us))
    txt = "\n".join(lines)
    print(txt)
    if out:
        open(out, "w").write(txt + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None)
