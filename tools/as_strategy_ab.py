"""A/B record of the acceleration-structure strategies (trhip_scene_set_accel_strategy).

    python tools/as_strategy_ab.py [--frames 40] [--out profiles/r7/as_strategy_ab.txt]

Per scene (sponza_teapots with the 50 teapots on one span, and sponza_class) at 1920x1080, 4 bounces, 1 spp, and per strategy
(all-merged; per-mesh; static-merged-dynamic-per-mesh with the teapots dynamic): accel bytes (node + record bytes of both levels), the
full build's device ms, the rigid update (10 teapots moved, then trhip_scene_update_instances + trhip_scene_refit_accel; teapot scene
only), ms per frame one frame at a time as bench.py defines it (RtRenderer.render() + sync, host wall time, after warm-up frames), and
the trhip_pt_get_timings kernel ms per frame.  The two-level kernels run without the quad-cooperative tail: `--lib` names a library built
with -DTR_QUAD_SWITCH=0 (make -C tauray_amd/csrc variant NAME=noquad EXTRA=-DTR_QUAD_SWITCH=0) for the all-merged row with the tail off.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRATEGY_NAMES = {0: "all-merged", 1: "per-mesh", 2: "static-merged-dynamic-per-mesh"}


def measure(scene_name, strategies, frames, W=1920, H=1080):
    from tauray_amd import renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_SCANLINE
    sc = scenes.sponza_teapots(width=W, height=H, share_teapot_mesh=True) if scene_name == "teapots" else scenes.sponza_class(width=W, height=H)
    n = len(sc.instances)
    teapot = np.zeros(n, np.uint8)
    if scene_name == "teapots":
        teapot[-50:] = 1
    ctx = R.Context(0)
    rows = []
    for strategy in strategies:
        dyn = teapot if strategy == 2 else None
        ss = R.SceneStage(ctx, sc, as_strategy=strategy, dynamic=dyn)
        lay = ss.layout()
        row = dict(scene=scene_name, strategy=STRATEGY_NAMES[strategy], triangles=int(sc.triangle_count), blas_count=lay["blas_count"],
                   tlas_leaves=lay["tlas_leaf_count"], accel_bytes=int(lay["node_bytes"] + lay["record_bytes"]),
                   build_ms=round(ss.accel["build_ms"], 3))
        if scene_name == "teapots":
            upd = []
            inst = sc.instances.copy()
            for k in range(6):
                inst["model"][-10:, 3, 0] += np.float32(0.01)       # ten teapots move along x
                t0 = time.perf_counter()
                ss.update_instances(inst, refit=True)
                wall = (time.perf_counter() - t0) * 1e3
                l2 = ss.layout()
                upd.append((wall, l2["blas_ms"] + l2["tlas_ms"], l2["blas_updated"]))
            upd = upd[1:]
            row.update(rigid_update_wall_ms=round(float(np.median([u[0] for u in upd])), 3),
                       rigid_update_device_ms=round(float(np.median([u[1] for u in upd])), 3), rigid_update_blases=upd[-1][2])
        del ss
        # frames as bench.py times them: RtRenderer, one at a time, host wall time from before render() to after the sync
        rr = R.RtRenderer(ctx, sc, R.options_for_scene(sc, max_bounces=4), (W, H), strategy=DISTRIBUTION_SCANLINE, as_strategy=strategy, dynamic=dyn)
        for _ in range(20):
            rr.reset_accumulation(); rr.render()
        rr.sync()
        times = []
        for _ in range(frames):
            t0 = time.perf_counter()
            rr.reset_accumulation(); rr.render(); rr.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        c = rr.counters()
        row.update(ms_per_frame=round(float(np.mean(times)), 4), ms_per_frame_p50=round(float(np.median(times)), 4), stack_overflows=int(c["stack_overflows"]))
        rr.set_profiling(False, True)
        k = 10
        for _ in range(k):
            rr.reset_accumulation(); rr.render()
        t = rr.timings()
        row["kernel_ms_per_frame"] = {name: round(v / k, 4) for name, v in t.items() if name.endswith("_ms") and v}
        rr.set_profiling(False, False)
        rr.close()
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "as_strategy_ab.txt"))
    ap.add_argument("--lib", default=None, help="library for the all-merged row without the quad tail (TRHIP_LIB of a child)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        scene, strategies = args.child.split(":")
        print(json.dumps(measure(scene, [int(s) for s in strategies.split(",")], args.frames)))
        return
    rows = []
    for scene in ("teapots", "sponza_class"):
        runs = [(None, "0,1,2")] + ([(args.lib, "0")] if args.lib else [])
        for lib, strategies in runs:
            env = dict(os.environ)
            if lib:
                env["TRHIP_LIB"] = lib
            out = subprocess.run([sys.executable, __file__, "--child", f"{scene}:{strategies}", "--frames", str(args.frames)], env=env,
                                 capture_output=True, text=True, timeout=400)
            if out.returncode != 0:
                raise RuntimeError(f"{scene} {lib}: exit {out.returncode}\n{out.stderr[-2000:]}")
            got = json.loads(out.stdout.strip().splitlines()[-1])
            for r in got:
                r["library"] = "quad tail off (-DTR_QUAD_SWITCH=0)" if lib else "default"
            rows += got
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
