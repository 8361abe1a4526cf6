"""How the lanes of a one-frame-at-a-time frame start, from a rocprofv3 kernel trace of a bench run
(`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python bench.py`): DESIGN.md section 29.

    python tools/primary_start_trace.py DIR/.../t_kernel_trace.csv [--skip-frames 20]

A lane is a hardware queue; its pass is the run of launches that ends in k_resolve.  Busy stretches of the GPU separated by more than 10 us of
idle time are frames; those whose passes sit on `--lanes` distinct queues are counted (the pipelined and two-in-flight regions of the bench
overlap frames and drop out).  Per lane, medians over the frames: launches per pass, the start of the closest-hit launch of bounce 0
(k_trace_closest or k_trace_closest_primary) after the frame's first kernel, and the kernel time of k_raygen, of that launch and of the
k_shade launch behind it.  A launch's time includes what it waited for the other lanes' launches."""
import argparse
import csv
import re

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip-frames", type=int, default=20)
    ap.add_argument("--lanes", type=int, default=4)
    args = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(args.trace)):
        m = re.search(r"(k_[a-z_0-9]+)", r["Kernel_Name"])
        if m:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(1), r.get("Queue_Id", "0")))
    rows.sort()
    stretches = []      # [start, end, rows]
    for row in rows:
        if stretches and row[0] <= stretches[-1][1] + 10_000:
            stretches[-1][1] = max(stretches[-1][1], row[1]); stretches[-1][2].append(row)
        else:
            stretches.append([row[0], row[1], [row]])
    frames = []
    for s, e, rs in stretches:
        queues = {}
        for row in rs:
            queues.setdefault(row[3], []).append(row)
        lanes = []
        for q in queues.values():      # a pass: up to its k_resolve (the frame's last lane may be followed by a tonemap or a copy)
            ends = [i for i, row in enumerate(q) if row[2] == "k_resolve"]
            if len(ends) == 1 and any(row[2].startswith("k_trace_closest") for row in q[:ends[0]]):
                lanes.append(q[:ends[0] + 1])
        if len(lanes) == args.lanes:
            frames.append((s, e, sorted(lanes, key=lambda q: q[0][0])))
    frames = frames[args.skip_frames:]
    if not frames:
        print("no frames of %d lanes found" % args.lanes)
        return
    print(f"# {len(frames)} frames of {args.lanes} lanes behind the first {args.skip_frames}; busy stretch per frame: mean {np.mean([e - s for s, e, _ in frames]) / 1e6:.4f} ms; "
          f"launches per frame: {np.mean([sum(len(q) for q in l) for _, _, l in frames]):.1f}")
    for lane in range(args.lanes):      # lanes in the order their first kernel starts
        n, first, ray, clo, sha, chain = [], [], [], [], [], None
        for s, e, lanes in frames:
            q = lanes[lane]
            n.append(len(q))
            ray.append(sum(b - a for a, b, k, _ in q if k == "k_raygen"))
            i = next(i for i, row in enumerate(q) if row[2].startswith("k_trace_closest"))
            first.append(q[i][0] - s)
            clo.append(q[i][1] - q[i][0])
            j = next(j for j in range(i, len(q)) if q[j][2] == "k_shade")
            sha.append(q[j][1] - q[j][0])
            chain = chain or " ".join(k[2:] for _, _, k, _ in q)
        med = lambda v: float(np.median(v)) / 1e3
        print(f"lane {lane}: launches {np.median(n):.0f}; closest-hit launch of bounce 0 starts {med(first):7.1f} us after the frame's first kernel; "
              f"k_raygen {med(ray):6.1f} us, that launch {med(clo):6.1f} us, the k_shade behind it {med(sha):6.1f} us   [{chain}]")
    # the merged ray generation of a short frame runs on the first lane's queue ahead of the fork: it shows as that lane's k_raygen


if __name__ == "__main__":
    main()
