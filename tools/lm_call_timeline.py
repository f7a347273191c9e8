"""Timelines of the last three calls of tools/lm_call_probe.py from its rocprofv3 kernel-trace CSV, in the format of tools/step_timeline.py
(start offset, idle gap before the kernel, duration, name).  The probe synchronises the stream and pauses for 5 ms before each of these calls, and no gap inside
a call comes near that (they are a few microseconds of launch latency), so a call begins after an
idle gap of more than SPLIT_US."""
import csv, sys
SPLIT_US = 2000.0
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
starts = [0]
for i in range(1, len(rows)):
    if (int(rows[i]["Start_Timestamp"]) - max(int(r["End_Timestamp"]) for r in rows[max(0, i - 4):i])) / 1e3 > SPLIT_US:
        starts.append(i)
starts.append(len(rows))
titles = ["call without fetch", "call with fetch", "call with fetch (second)"]
for title, a, b in zip(titles, starts[-4:-1], starts[-3:]):
    print("-- %s: %d stream operations" % (title, b - a))
    t0 = int(rows[a]["Start_Timestamp"]); prev_end = t0
    gaps = 0.0
    for r in rows[a:b]:
        n = r["Kernel_Name"].replace("void ", "").replace("vba::", "").split("(")[0]
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        gap = (s - prev_end) / 1e3
        gaps += max(gap, 0.0)
        print("%9.1f us  +%6.1f gap  %7.1f us  %s" % ((s - t0) / 1e3, gap, (e - s) / 1e3, n[:60]))
        prev_end = max(prev_end, e)
    print("idle gaps %.1f us of %.1f us" % (gaps, (prev_end - t0) / 1e3))
