#!/usr/bin/env python3
"""ws_gram_kernel per class of build, the opening and the chains of a cold path, from rocprofv3 kernel traces (csv).

A path opens with solve_begin_kernel; its ws_gram_kernel launches are, in order, the opening (a fresh selection), the first
append (to at most 8 tiles on the headline) and the second (to 9-11 tiles).  Per trace: median, smallest and largest launch
of each class over the paths, the launches and the kernel time before the first xtr18_mfma_kernel, and the kernel time of the
two chains between the passes (after an xtr18_mfma_kernel up to the next one, the rowdot / resid kernels included).

usage: python tools/gram_pipeline_summary.py <label>=<kernel_trace.csv> [...]"""
import csv
import statistics
import sys

CLASSES = ("opening", "append to <= 8 tiles", "append to 9-11 tiles")


def short(name):
    return name.split("(")[0].replace("slm::", "").replace("void ", "")


def paths(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = [(short(r["Kernel_Name"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    starts = [i for i, (nm, _) in enumerate(seq) if nm == "solve_begin_kernel"]
    return [seq[a:b] for a, b in zip(starts, starts[1:] + [len(seq)])]


def stats(v):
    return f"median {statistics.median(v):6.1f}   smallest {min(v):6.1f}   largest {max(v):6.1f}   ({len(v)} launches)"


for arg in sys.argv[1:]:
    label, path = arg.split("=", 1)
    grams = {c: [] for c in CLASSES}
    before, before_n, chains = [], [], ([], [])
    used = 0
    for p in paths(path):
        names = [nm for nm, _ in p]
        x = [i for i, nm in enumerate(names) if nm == "xtr18_mfma_kernel"]
        g = [d for nm, d in p if nm.startswith("ws_gram_kernel")]
        if len(x) != 3 or len(g) != 3:
            continue  # (not a headline path of three passes and three builds)
        used += 1
        for c, d in zip(CLASSES, g):
            grams[c].append(d)
        before.append(sum(d for _, d in p[:x[0]]))
        before_n.append(x[0])
        for k in (0, 1):
            chains[k].append(sum(d for _, d in p[x[k] + 1:x[k + 1]]))
    print(f"{label}: {used} paths of three passes")
    for c in CLASSES:
        print(f"  ws_gram_kernel, {c:22s} (us)  {stats(grams[c])}")
    print(f"  launches before the first xtr18_mfma     {sorted(set(before_n))}")
    print(f"  kernels before the first xtr18_mfma (us)  {stats(before)}")
    for k in (0, 1):
        print(f"  chain {k + 1}, sum of kernel times (us)        {stats(chains[k])}")
