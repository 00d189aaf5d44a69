"""One frame of a rocprofv3 --kernel-trace CSV as a timeline: every kernel of the frame whose span is the median of the run,
with its start relative to the frame's first kernel, its duration, the gap to the end of the kernel before it (negative: they
overlapped) and the queue it ran on; then the median duration of every kernel by its place in the frame.
usage: python profiles/timeline.py <kernel_trace.csv>"""
import collections
import csv
import statistics
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
frames, cur = [], None
for r in rows:
    name = r["Kernel_Name"].split("(")[0]
    if name.endswith("k_frame_init"):
        cur = []
        frames.append(cur)
    if cur is not None:
        cur.append((name[-40:], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?")))
        if name.endswith("k_frame_done"):
            cur = None
frames = [f for f in frames if f[-1][0].endswith("k_frame_done")]
if not frames:
    sys.exit("no complete frame in the trace")
span = lambda f: max(k[2] for k in f) - f[0][1]
mid = sorted(frames, key=span)[len(frames) // 2]
t0, last_end = mid[0][1], mid[0][1]
for name, a, b, q in mid:
    print("%-40s queue %-3s start %7.1f us  dur %6.1f us  gap %7.1f us" % (name, q, (a - t0) / 1e3, (b - a) / 1e3, (a - last_end) / 1e3))
    last_end = max(last_end, b)
print("frame span %.1f us (median of %d frames: %.1f us)" % (span(mid) / 1e3, len(frames), statistics.median(span(f) for f in frames) / 1e3))
# by place in the frame: the i-th launch of a kernel name within its frame
by_place = collections.defaultdict(list)
for f in frames:
    seen = collections.Counter()
    for name, a, b, q in f:
        by_place[(name, seen[name])].append((b - a) / 1e3)
        seen[name] += 1
order = []
for name, a, b, q in mid:
    order.append(name)
seen = collections.Counter()
for name in order:
    v = by_place[(name, seen[name])]
    print("  %-40s #%d  n=%4d median %7.1f us  min %7.1f" % (name, seen[name], len(v), statistics.median(v), min(v)))
    seen[name] += 1
