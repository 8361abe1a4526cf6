"""A/B record of the sphere-light modes (trhip_scene_set_light_accel).

    python tools/light_accel_ab.py [--frames 50] [--lights 0,4,16,64,256,1024,4096] [--out profiles/r8/sphere_light_accel.txt]

Per light count L: sponza_lights(L) at 1920x1080, 4 bounces, 1 spp, rendered by one RtRenderer, with TRHIP_LIGHT_ACCEL_LOOP and _TREE
alternating (loop, tree, loop, tree) on the same scene.  Per mode: ms per frame as bench.py times it (warmed, host wall time from before
render() to after the sync, one frame at a time, `--frames` frames per pass; mean and the spread of the pass means), the closest-hit
kernel ms per frame from detailed timing (trhip_pt_get_timings), sphere tests and light-tree node visits per closest-hit ray (count_work),
walks that ran out of stack and fell back to the loop, and the tree's build and refit times (trhip_scene_get_light_accel; refit =
trhip_scene_update_lights with every light moved by 1 mm).  The record is written afresh, its first line naming the build and the device.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOOP, TREE = 1, 2


def measure(L, frames, W=1920, H=1080, passes=2):
    from tauray_amd import renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_SCANLINE
    sc = scenes.sponza_lights(L, seed=1, width=W, height=H)
    ctx = R.Context(0)
    rr = R.RtRenderer(ctx, sc, R.options_for_scene(sc, max_bounces=4), (W, H), strategy=DISTRIBUTION_SCANLINE)
    ss = rr.scene_update
    row = dict(lights=L, sphere_lights=int((sc.point_lights["radius"] != 0).sum()) if L else 0)
    ss.set_light_accel(TREE)
    info = ss.light_accel()
    row.update(tree_build_ms=round(info["last_ms"], 3), tree_nodes=info["node_count"], tree_bytes=info["tree_bytes"])
    if L:
        refits = []
        for k in range(5):
            moved = sc.point_lights.copy()
            moved["pos"] += np.float32(0.001 * (k + 1))
            ss.update_lights(moved)
            refits.append(ss.light_accel()["last_ms"])
        ss.update_lights(sc.point_lights)
        row["tree_refit_ms"] = round(float(np.median(refits)), 3)
    per_mode = {LOOP: [], TREE: []}
    for p in range(passes):
        for mode in (LOOP, TREE):
            ss.set_light_accel(mode)
            for _ in range(10):
                rr.reset_accumulation(); rr.render()
            rr.sync()
            times = []
            for _ in range(frames):
                t0 = time.perf_counter()
                rr.reset_accumulation(); rr.render(); rr.sync()
                times.append((time.perf_counter() - t0) * 1e3)
            per_mode[mode].append(times)
    for mode, name in ((LOOP, "loop"), (TREE, "tree")):
        ss.set_light_accel(mode)
        means = [float(np.mean(t)) for t in per_mode[mode]]
        row[name] = dict(ms_per_frame=round(float(np.mean(means)), 4), pass_means=[round(m, 4) for m in means],
                         spread_ms=round(max(means) - min(means), 4), p50=round(float(np.median(np.concatenate(per_mode[mode]))), 4))
        rr.set_profiling(False, True)
        rr.reset_counters()
        for _ in range(5):
            rr.reset_accumulation(); rr.render()
        t = rr.timings()
        row[name]["closest_ms_per_frame"] = round(t.get("trace_closest_ms", 0.0) / 5, 4)
        row[name]["kernel_ms_per_frame"] = {k: round(v / 5, 4) for k, v in t.items() if k.endswith("_ms") and v}
        rr.set_profiling(True, False)
        rr.reset_counters()
        rr.reset_accumulation(); rr.render()
        c = rr.counters()
        lc = [s.pt.light_counters() for s in rr.slots]
        tests = sum(x["sphere_tests"] for x in lc)
        nodes = sum(x["node_visits"] for x in lc)
        rays = max(1, int(c["closest_rays"]))
        row[name].update(sphere_tests_per_ray=round(tests / rays, 3), light_nodes_per_ray=round(nodes / rays, 3),
                         walk_fallbacks=sum(x["walk_fallbacks"] for x in lc), stack_overflows=int(c["stack_overflows"]))
        rr.set_profiling(False, False)
    rr.close()
    return row


def header():
    """What the record was measured with: the library's build id, the device, the date."""
    from tauray_amd import _lib, renderer as R
    ctx = R.Context(0)
    info = ctx.info()
    name = info.get("name", "")
    return dict(record="sphere_light_accel", build_id=f"{_lib.lib().trhip_build_id():016x}", device=name.decode() if isinstance(name, bytes) else name,
                date=time.strftime("%Y-%m-%d %H:%M:%S %Z"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--lights", default="0,4,16,64,256,1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "sphere_light_accel.txt"))
    args = ap.parse_args()
    rows = []
    for L in (int(x) for x in args.lights.split(",")):
        row = measure(L, args.frames)
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:     # a fresh record per run, headed by what produced it
        f.write(json.dumps(header()) + "\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
