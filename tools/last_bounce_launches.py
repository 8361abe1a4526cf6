"""Time of the last bounce's launches in a rocprofv3 kernel trace of a bench run
(`rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python bench.py`).

    python tools/last_bounce_launches.py kernel_trace.csv [--skip-frames 20]

The launches of a lane come in order on its queue.  The last k_shade of a frame is the LAST instance (k_shade<.., true, ..>), and the trace
launch in front of it on the same queue is the last bounce's: k_trace_fused (closest-hit rays of that bounce + shadow rays of the one
before) or, with the terminal query in effect, k_trace_fused_terminal.  Prints launches, mean and median duration per launch of those two
and of the other fused / shade launches, over the frames behind the first `--skip-frames` of every lane.  The lanes of a frame overlap,
so a launch's duration includes what it waited for the other lanes' launches."""
import argparse
import csv
import re
import statistics
from collections import defaultdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip-frames", type=int, default=20)
    args = ap.parse_args()
    per_queue = defaultdict(list)
    for r in csv.DictReader(open(args.trace)):
        m = re.search(r"(k_trace_\w+|k_shade)<([^>]*)>", r["Kernel_Name"])
        if m:
            per_queue[r["Queue_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(1), m.group(2)))
    groups = defaultdict(list)
    for launches in per_queue.values():
        launches.sort()
        frame, traces = 0, []
        for s, e, name, targs in launches:
            keep = frame >= args.skip_frames
            if name != "k_shade":
                traces.append((e - s, name))
            elif targs.split(",")[1].strip() == "true":      # the LAST instance ends the frame of this lane
                if keep:
                    groups["k_shade, last bounce"].append(e - s)
                    for d, n in traces[:-1]:
                        groups[f"{n}, other bounces"].append(d)
                    if traces:
                        groups[f"{traces[-1][1]}, last bounce"].append(traces[-1][0])
                frame, traces = frame + 1, []
            elif keep:
                groups["k_shade, other bounces"].append(e - s)
    print(f"# {args.trace}: {len(per_queue)} queues, frames behind the first {args.skip_frames} of each; microseconds per launch")
    for k in sorted(groups):
        v = groups[k]
        print(f"{k:44s} launches {len(v):6d}  mean {statistics.mean(v) / 1e3:9.2f}  median {statistics.median(v) / 1e3:9.2f}")


if __name__ == "__main__":
    main()
