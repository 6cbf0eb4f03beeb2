#!/usr/bin/env python3
"""Per-stage kernel times of Tracking's per-frame chain from a kernel trace of
tools/track_timing.py --no-host:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o track -- \\
      python tools/track_timing.py --no-host --reps 20
  python tools/track_trace_stats.py DIR/.../track_kernel_trace.csv > profiles/track_stage_stats.csv

rocprofv3's own stats file has one row per kernel name, so the two proj_kernel
launches of call 1 (the search and the idle retry), the one of call 2 and the
two poseopt_kernel launches share rows.  This reads the dispatch records in
start order and names each proj_kernel / poseopt_kernel launch after the glue
kernel it follows.  Output: kernel, calls, avg, median, min, max in microseconds.
"""
import collections
import csv
import re
import statistics
import sys

STAGE = re.compile(r"(initial_\w+?_kernel|local_\w+?_kernel|proj_kernel|poseopt_kernel|update_last_frame_kernel)")


def main():
    with open(sys.argv[1], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out, prev = collections.OrderedDict(), None
    for r in rows:
        m = STAGE.search(r["Kernel_Name"])
        if not m:
            continue
        name = m.group(1)
        if name in ("proj_kernel", "poseopt_kernel"):
            if prev is None:
                continue
            name = f"{name} after {prev}"
        else:
            prev = name
        out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("kernel,calls,avg_us,median_us,min_us,max_us")
    for k, v in out.items():
        print(f"{k},{len(v)},{statistics.mean(v):.2f},{statistics.median(v):.2f},{min(v):.2f},{max(v):.2f}")
    print(f"sum of medians,,,{sum(statistics.median(v) for v in out.values()):.2f},,")


if __name__ == "__main__":
    main()
