#!/usr/bin/env python3
"""The workload and the reading of profiles/align_group_trace_g1.txt: one Gaussian-eval pair (N 2000, d 128 + 128, topk 10) through
the single alignment calls and through umlh.align.measure_pairs with one member.

    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python3 scripts/trace_align_group.py
    python3 scripts/trace_align_group.py --post DIR

Without arguments: 30 evaluations through align.cka + align.mutual_knn, then 30 through measure_pairs, back to back without a host
wait.  --post: per kernel of an evaluation its average duration and the idle time of the device in front of it over the last 25
whole evaluations of each path, then the small host-to-device copies (the descriptor uploads)."""
import glob
import os
import re
import sqlite3
import sys


def workload():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "unpaired-multimodal-learning_amd")):
        sys.path.insert(0, p)
    import torch
    from umlh import align
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0)
    a = torch.randn(2000, 128, device="cuda:0", generator=g)
    b = a * 0.5 + torch.randn(2000, 128, device="cuda:0", generator=g)
    for _ in range(3):
        align.cka(a, b); align.mutual_knn(a, b, 10); align.measure_pairs([(a, b)])
    torch.cuda.synchronize()
    for _ in range(30):
        align.cka(a, b); align.mutual_knn(a, b, 10)
    torch.cuda.synchronize()
    for _ in range(30):
        align.measure_pairs([(a, b)])
    torch.cuda.synchronize()


def post(src):
    db = glob.glob(src + "/**/*.db", recursive=True)[0]
    c = sqlite3.connect(db)
    rows = c.execute("select name, grid_x/workgroup_x, grid_y/workgroup_y, grid_z/workgroup_z, start, end from kernels order by start").fetchall()
    def short(n):
        m = re.search(r"(knn_\w+|cka_\w+|mutual_\w+)", n)
        return m.group(1) if m else None
    rows = [(short(r[0]),) + tuple(r[1:]) for r in rows if short(r[0])]
    for name, pick, first in (("single calls", lambda k: not k.endswith("_pairs"), "cka_colsum"), ("measure_pairs, one member", lambda k: k.endswith("_pairs"), "cka_colsum_pairs")):
        seq = [r for r in rows if pick(r[0])]
        starts = [i for i, r in enumerate(seq) if r[0] == first][-26:]            # the last 25 whole evaluations
        evs = [seq[a:b] for a, b in zip(starts[:-1], starts[1:])]
        per = len(evs[0])
        assert all(len(e) == per for e in evs), [len(e) for e in evs]
        print(f"== {name}: {len(evs)} back-to-back evaluations of {per} kernels, averages")
        tot = 0.0
        for i in range(per):
            d = sum(e[i][5] - e[i][4] for e in evs) / len(evs)
            gap = sum((e[i][4] - e[i - 1][5]) for e in evs if i > 0) / len(evs) if i else sum(evs[j][0][4] - evs[j - 1][-1][5] for j in range(1, len(evs))) / (len(evs) - 1)
            r = evs[0][i]
            print("%2d %-22s %4dx%3dx%3d  kernel %7.2f us  idle before it %7.2f us" % (i, r[0], r[1], r[2], r[3], d / 1e3, gap / 1e3))
            tot += d
        span = (evs[-1][-1][5] - evs[0][0][4]) / len(evs)
        print("kernel sum %.2f us, first start to last end %.2f us per evaluation" % (tot / 1e3, span / 1e3))

    try:
        cur = c.execute("select * from memory_copies")
    except sqlite3.Error:
        print("== no memory-copy trace in this run")
        return
    cols = [d[0] for d in cur.description]
    rows = cur.fetchall()
    if "start" not in cols or "end" not in cols or not rows:
        print("== no memory-copy trace in this run")
        return
    si, ei = cols.index("start"), cols.index("end")
    szi = cols.index("size") if "size" in cols else None
    small = [r for r in rows if szi is None or r[szi] <= 4096][-25:]
    if small:
        d = [(r[ei] - r[si]) / 1e3 for r in small]
        print("== the last %d copies of <= 4096 bytes (the descriptor uploads): avg %.2f us (min %.2f, max %.2f)" % (len(d), sum(d) / len(d), min(d), max(d)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--post":
        post(sys.argv[2])
    else:
        workload()
