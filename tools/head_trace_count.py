#!/usr/bin/env python3
"""Kernel launches per training step, dense against sparse vocabulary head, from ONE kernel trace of tools/head_bench.py --blocks.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/head_bench.py --blocks --steps 6 --warmup 2
    python tools/head_trace_count.py DIR/**/*kernel_trace.csv [--out profiles/NAME.json]

Phase 0 of every backward pass launches exactly one of k_dlogits_tb (dense head) / k_dlogits_sel (sparse head).  The dispatches, in
start order, from one such launch up to the next are one step's worth of launches (the rest of a backward, the optimizer, the next
forward) when both ends are the same kernel; a cycle that holds a CIDEr-D kernel belongs to the SCST step, the others to the XE step.
Reported per (workload, setting): the median and the min / max launch count over its cycles, and the kernels whose per-cycle count
differs between the two settings of a workload."""
import argparse
import collections
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", nargs="+")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for path in a.trace:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    names = [n for _, n in rows]
    kind = lambda n: "sparse" if "k_dlogits_sel" in n else "dense" if "k_dlogits_tb" in n else None
    marks = [i for i, n in enumerate(names) if kind(n)]
    cycles = collections.defaultdict(list)
    for lo, hi in zip(marks, marks[1:]):
        if kind(names[lo]) != kind(names[hi]):
            continue                                        # the seam between two blocks
        cyc = names[lo:hi]
        wl = "scst" if any("cider" in n.lower() for n in cyc) else "xe"
        cycles[(wl, kind(names[lo]))].append(collections.Counter(n.split("(")[0] for n in cyc))
    res = {}
    for (wl, k), cs in sorted(cycles.items()):
        tot = [sum(c.values()) for c in cs]
        res.setdefault(wl, {})[k] = {"cycles": len(cs), "launches_per_step_median": statistics.median(tot), "min": min(tot), "max": max(tot)}
    for wl in res:
        if len(res[wl]) == 2:
            med = {k: {n: statistics.median(c[n] for c in cycles[(wl, k)]) for n in set().union(*cycles[(wl, k)])} for k in ("dense", "sparse")}
            diff = {n: [med["dense"].get(n, 0), med["sparse"].get(n, 0)] for n in set(med["dense"]) | set(med["sparse"])
                    if med["dense"].get(n, 0) != med["sparse"].get(n, 0)}
            res[wl]["kernels_that_differ_dense_sparse"] = dict(sorted(diff.items()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
