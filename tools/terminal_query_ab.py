"""A/B record of the terminal query (trhip_pt_set_terminal_query).

    python tools/terminal_query_ab.py [--frames 50] [--workloads sponza_teapots,sponza_class,test_glb] [--out profiles/r9/terminal_query_ab.txt]

Per workload: the bench scene at 1920x1080, 4 bounces, 1 spp, rendered by one RtRenderer with TRHIP_TERMINAL_QUERY_OFF and _AUTO
alternating (off, auto, off, auto) on the same scene.  Per mode: ms per frame as bench.py times it (warmed, host wall time from before
render() to after the sync, one frame at a time, `--frames` frames per pass; mean and the spread of the pass means), kernel ms per frame
from detailed timing (trhip_pt_get_timings: the launches run alone, one lane), and from a counted frame the node visits and triangle
tests per ray (closest-hit and shadow rays together, as trhip_counters has them), the rays that ended blocked and the rays that took the
per-ray fallback.  The record is written afresh, its first line naming the build and the device.  This compares the two modes of ONE
build; whether the build is faster than its parent is a matter for bench.py with both libraries (TRHIP_LIB)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AUTO, OFF = 0, 1


def measure(workload, frames, W=1920, H=1080, passes=2):
    from tauray_amd import renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_SCANLINE
    sc = scenes.WORKLOADS[workload](W, H)
    ctx = R.Context(0)
    rr = R.RtRenderer(ctx, sc, R.options_for_scene(sc, max_bounces=4), (W, H), strategy=DISTRIBUTION_SCANLINE)
    row = dict(workload=workload, triangles=sc.triangle_count)

    def set_mode(mode):
        for s in rr.slots:
            s.pt.set_terminal_query(mode)

    per_mode = {OFF: [], AUTO: []}
    for p in range(passes):
        for mode in (OFF, AUTO):
            set_mode(mode)
            for _ in range(10):
                rr.reset_accumulation(); rr.render()
            rr.sync()
            times = []
            for _ in range(frames):
                t0 = time.perf_counter()
                rr.reset_accumulation(); rr.render(); rr.sync()
                times.append((time.perf_counter() - t0) * 1e3)
            per_mode[mode].append(times)
    for mode, name in ((OFF, "off"), (AUTO, "auto")):
        set_mode(mode)
        means = [float(np.mean(t)) for t in per_mode[mode]]
        row[name] = dict(ms_per_frame=round(float(np.mean(means)), 4), pass_means=[round(m, 4) for m in means],
                         spread_ms=round(max(means) - min(means), 4), p50=round(float(np.median(np.concatenate(per_mode[mode]))), 4))
        rr.set_profiling(False, True)
        rr.reset_counters()
        for _ in range(5):
            rr.reset_accumulation(); rr.render()
        t = rr.timings()
        row[name]["kernel_ms_per_frame"] = {k: round(v / 5, 4) for k, v in t.items() if k.endswith("_ms") and v}
        rr.set_profiling(True, False)
        rr.reset_counters()
        rr.reset_accumulation(); rr.render()
        c = rr.counters()
        tc = [s.pt.terminal_counters() for s in rr.slots]
        rays = max(1, int(c["closest_rays"]) + int(c["shadow_rays"]))
        row[name].update(in_effect=max(x["in_effect"] for x in tc), emitter_triangles=tc[0]["emitter_triangles"], closest_rays=int(c["closest_rays"]),
                         shadow_rays=int(c["shadow_rays"]), surface_hits=int(c["surface_hits"]), node_visits=int(c["node_visits"]), tri_tests=int(c["tri_tests"]),
                         node_visits_per_ray=round(c["node_visits"] / rays, 3), tri_tests_per_ray=round(c["tri_tests"] / rays, 3),
                         blocked_rays=sum(x["blocked_rays"] for x in tc), fallback_rays=sum(x["fallback_rays"] for x in tc),
                         stack_overflows=int(c["stack_overflows"]))
        rr.set_profiling(False, False)
    rr.close()
    return row


def header():
    """What the record was measured with: the library's build id, the device, the date."""
    from tauray_amd import _lib, renderer as R
    ctx = R.Context(0)
    info = ctx.info()
    name = info.get("name", "")
    return dict(record="terminal_query_ab", build_id=f"{_lib.lib().trhip_build_id():016x}", device=name.decode() if isinstance(name, bytes) else name,
                date=time.strftime("%Y-%m-%d %H:%M:%S %Z"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--workloads", default="sponza_teapots,sponza_class,test_glb")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "terminal_query_ab.txt"))
    args = ap.parse_args()
    rows = []
    for w in args.workloads.split(","):
        row = measure(w, args.frames)
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:     # a fresh record per run, headed by what produced it
        f.write(json.dumps(header()) + "\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
