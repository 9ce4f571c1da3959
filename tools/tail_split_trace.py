#!/usr/bin/env python3
"""Where the kernels of a frame lie in time, from a rocprofv3 kernel trace of bench.py:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 bench.py --gpus 1 --steps 20 --warmup 5 ...
    python3 tools/tail_split_trace.py DIR [frames, default 20]

A frame is one or two launches of the integrate kernel (K2, or K2a and K2b of a split frame) and one or two of the
epilogue (K3, or K3a and K3b).  Of two integrate launches the one that starts first is K2a: it is enqueued first, and the
side stream waits for the fork event and zeroes its head word before K2b.  A launch's start stamp is when its dispatch
began, not when its first wavefront got a slot: K2b's dispatch begins tens of microseconds after K2a's and then waits for
the slots K2a's wavefronts leave, so what shows when K2b really ran is K2a's end (K3a starts there) against K2b's end.
For the last `frames` frames of the trace: start and end of each launch relative to the frame's first start, the frame's
span (first start to last end of these kernels), how long K2b went on after K2a's end, and how long K3a and K2b ran side
by side.  Microseconds; mean (min ... max)."""
import csv
import glob
import os
import sys


def launches(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {d}")
    out = []
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                kind = "K2" if "k_kerr_direct" in name else ("K3" if "k_epilogue_frame" in name else None)
                if kind:
                    out.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), kind))
    return sorted(out)


def frames_of(ls):
    frames, cur = [], []
    for ev in ls:
        if ev[2] == "K2" and any(e[2] == "K3" for e in cur):
            frames.append(cur)
            cur = []
        cur.append(ev)
    if cur:
        frames.append(cur)
    return frames


def stat(v):
    return f"{sum(v) / len(v):9.1f} ({min(v):.1f} ... {max(v):.1f})"


def main():
    d = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    fr = frames_of(launches(d))[-n:]
    cols = {}
    for f in fr:
        t0 = min(e[0] for e in f)
        k2 = sorted(e for e in f if e[2] == "K2")
        k3 = sorted(e for e in f if e[2] == "K3")
        row = {"span": (max(e[1] for e in f) - t0) / 1e3}
        names = (["K2a", "K2b"] if len(k2) == 2 else ["K2"]) + (["K3a", "K3b"] if len(k3) == 2 else ["K3"])
        for nm, e in zip(names, k2 + k3):
            row[nm + " start"], row[nm + " end"] = (e[0] - t0) / 1e3, (e[1] - t0) / 1e3
        if len(k2) == 2:
            row["K2b end after K2a end"] = (k2[1][1] - k2[0][1]) / 1e3
        if len(k2) == 2 and len(k3) == 2:
            row["K3a beside K2b"] = max(0, min(k3[0][1], k2[1][1]) - max(k3[0][0], k2[1][0])) / 1e3
        for k, v in row.items():
            cols.setdefault(k, []).append(v)
    print(f"{len(fr)} frames; us relative to the frame's first kernel start, mean (min ... max)")
    for k, v in cols.items():
        print(f"  {k:28s} {stat(v)}" + ("" if len(v) == len(fr) else f"   [{len(v)} frames]"))


if __name__ == "__main__":
    main()
