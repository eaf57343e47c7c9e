#!/usr/bin/env python3
"""What lies between the ring kernels of consecutive rangeproof steps, from one rocprofv3 trace of the headline.

    rocprofv3 --kernel-trace --hip-trace --output-format csv -d DIR -o rp -- python bench.py --gpus 1 --steps 6 --warmup 2
    python tools/rp_step_gap.py DIR [--steps 6] > profiles/rp_step_gap_<when>.txt

For each of the last `steps` pairs of consecutive k_rp_rings_shared dispatches: the end of the first, the start of the second, every
dispatch on the same queue in between (result memset, k_rp_rings, k_rp_final, mailbox clear), when the k_rp_sum the second one waits
for ended (the side stage's last kernel), and the HIP calls the host made between the two launches (event records and stream waits
become barrier packets on the queue; the kernel trace does not show them, the call list does).
"""
import csv
import glob
import os
import statistics
import sys


def rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def find(d, suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    return hits[-1] if hits else None


def short(name):
    name = name.split("(")[0]
    return name if len(name) <= 48 else name[:45] + "..."


def main():
    d = sys.argv[1]
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 6
    kt = find(d, "kernel_trace.csv")
    ht = find(d, "hip_api_trace.csv")
    if not kt:
        sys.exit("no *kernel_trace.csv under " + d)
    K = [dict(name=r["Kernel_Name"], q=r.get("Queue_Id", ""), s=r.get("Stream_Id", ""), corr=int(r["Correlation_Id"]),
              t0=int(r["Start_Timestamp"]), t1=int(r["End_Timestamp"])) for r in rows(kt)]
    K.sort(key=lambda r: r["t0"])
    H = []
    if ht:
        H = [dict(fn=r["Function"], tid=r.get("Thread_Id", ""), corr=int(r["Correlation_Id"]), t0=int(r["Start_Timestamp"])) for r in rows(ht)]
        H.sort(key=lambda r: r["t0"])
    rings = [r for r in K if r["name"].startswith("k_rp_rings_shared")]
    sums = [r for r in K if r["name"].startswith("k_rp_sum")]
    if len(rings) < 2:
        sys.exit("fewer than two k_rp_rings_shared dispatches in the trace")
    pairs = list(zip(rings[:-1], rings[1:]))[-steps:]
    origin = pairs[0][0]["t0"]
    us = lambda t: (t - origin) / 1e3
    gaps, inside, late = [], [], []
    print("# gaps between consecutive k_rp_rings_shared dispatches, last %d pairs of %d dispatches; times in us from the first listed start" % (len(pairs), len(rings)))
    for a, b in pairs:
        gap = (b["t0"] - a["t1"]) / 1e3
        gaps.append(gap)
        print("\nstep pair: rings %.1f .. %.1f us (%.3f ms)  ->  next rings starts %.1f us   gap %.1f us" % (us(a["t0"]), us(a["t1"]), (a["t1"] - a["t0"]) / 1e6, us(b["t0"]), gap))
        busy = 0.0
        for r in K:
            if r is a or r is b or r["q"] != a["q"] or r["t0"] < a["t1"] or r["t1"] > b["t0"]:
                continue
            busy += (r["t1"] - r["t0"]) / 1e3
            print("    same queue   %-48s %9.1f .. %9.1f us  (%.1f us)" % (short(r["name"]), us(r["t0"]), us(r["t1"]), (r["t1"] - r["t0"]) / 1e3))
        inside.append(busy)
        for r in K:
            if r["q"] == a["q"] or r["t1"] <= a["t1"] or r["t0"] >= b["t0"]:
                continue
            print("    other queue  %-48s %9.1f .. %9.1f us  (%.1f us)" % (short(r["name"]), us(r["t0"]), us(r["t1"]), (r["t1"] - r["t0"]) / 1e3))
        prev = [s for s in sums if s["t1"] <= b["t0"]]
        if prev:
            s = prev[-1]
            late.append((s["t1"] - a["t1"]) / 1e3)
            print("    k_rp_sum of the next step ended %.1f us  (%+.1f us against the end of this ring kernel)" % (us(s["t1"]), late[-1]))
        if H:
            calls = [h for h in H if a["corr"] < h["corr"] < b["corr"]]
            seq = []
            for h in calls:
                if seq and seq[-1][0] == h["fn"]:
                    seq[-1][1] += 1
                else:
                    seq.append([h["fn"], 1])
            print("    host calls between the two launches: " + ", ".join("%s x%d" % (f, c) if c > 1 else f for f, c in seq))
    med = statistics.median
    print("\n# summary: gap median %.1f us (min %.1f, max %.1f); kernels and memsets inside it median %.1f us; the rest (packets, idle) median %.1f us"
          % (med(gaps), min(gaps), max(gaps), med(inside), med([g - i for g, i in zip(gaps, inside)])))
    if late:
        n_late = sum(x > 0 for x in late)
        print("# k_rp_sum of the next step ended %+.1f us (median; max %+.1f) against the end of the ring kernel in front of it: the side stage is late in %d of %d pairs"
              " (a pair behind a host synchronisation -- the end of the warm-up -- has no call in flight and is late by construction)" % (med(late), max(late), n_late, len(late)))


if __name__ == "__main__":
    main()
