#!/usr/bin/env python3
"""ReSTIR DI's light selection (trhip_restir_di_set_light_selection) on sponza_lights_powers - sponza_lights with
the lamps' powers log-uniform over three decades - at 1920 x 1080 with 64 and with 4096 lights: device ms of the canonical kernel and of
the stage at the defaults, uniform against power (warm-up frames first, then --frames timed frames of a running sequence; median with the
spread, min ... max, next to it), the host time of set_light_selection("power") and of a refresh that rebuilds, and - with --quality -
the frame-8 mean squared error at 128 x 72 against a 4096 spp direct-stage image for uniform and for power at the uniform fractions
0.05, 0.1 and 0.25, over 8 seeds.  No threshold: the record is profiles/r27/restir_light_selection.txt.

With TRHIP_LIB naming an older build of the library and --selections uniform, the same uniform rows come from that build: the uniform
mode's times against the parent commit.

usage: python tools/restir_light_selection_probe.py [--lights 64,4096] [--frames 20] [--warmup 5] [--selections uniform,power] [--quality]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = (0.05, 0.1, 0.25)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return f"{np.median(v):8.3f} ({v.min():.3f} ... {v.max():.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lights", default="64,4096")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--selections", default="uniform,power")
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    selections = [s for s in a.selections.split(",") if s]

    from tauray_amd import _lib, renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_DUPLICATE, DistributionParams

    w, h = 1920, 1080
    ctx = R.Context(0)
    for lights in (int(n) for n in a.lights.split(",")):
        scene = scenes.sponza_lights_powers(lights, 1, w, h)
        ss = R.SceneStage(ctx, scene)
        base = R.options_for_scene(scene)
        print(f"== {scene.name} ({ss.accel['triangle_count']} triangles, {len(scene.point_lights)} point lights), {w} x {h}, {a.warmup} warm-up and {a.frames} timed frames, "
              f"library {os.path.basename(_lib.LIB_PATH)}, build {_lib.lib().trhip_build_id():016x}")
        print("   device ms, median (min ... max)")
        out = ctx.alloc(w * h * 16).zero()
        for selection in selections:
            more = dict(light_selection=selection) if selection != "uniform" else {}      # an older library has no setter: uniform is never told
            st = R.RestirDiStage(ctx, ss, (w, h), 1, R.restir_di_options(min_ray_dist=base.min_ray_dist, **more), base.projection)
            rows = []
            for f in range(a.warmup + a.frames):
                st.run([0], out)
                ctx.sync()
                if f >= a.warmup:
                    t = st.timings()
                    rows.append((t["canonical_ms"], t["spatial_ms"], t["total_ms"]))
            rows = np.array(rows)
            print(f"restir-di defaults, light selection {selection}: [restir di canonical] {spread(rows[:, 0])}  [restir di spatial] {spread(rows[:, 1])}  stage {spread(rows[:, 2])}")
            if selection == "power":
                st.reset()
                set_ms, refresh_ms = [], []
                lamps = np.array(scene.point_lights, copy=True)
                for k in range(5):
                    ctx.sync()
                    t0 = time.perf_counter()
                    st.set_light_selection("power", 0.1)
                    set_ms.append((time.perf_counter() - t0) * 1e3)
                    moved = lamps.copy()
                    moved["color"] = np.roll(lamps["color"], k + 1, axis=0)      # other weights: the refresh rebuilds
                    ss.update_lights(moved, scene.directional_lights)
                    ctx.sync()
                    t0 = time.perf_counter()
                    rebuilt = st.refresh_light_selection()
                    refresh_ms.append((time.perf_counter() - t0) * 1e3)
                    assert rebuilt
                    t0 = time.perf_counter()
                    again = st.refresh_light_selection()
                    skipped_ms = (time.perf_counter() - t0) * 1e3
                    assert not again
                ss.update_lights(lamps, scene.directional_lights)
                print(f"   host ms of 5 calls: set_light_selection(power) {spread(set_ms)}; a refresh that rebuilds {spread(refresh_ms)}; the last refresh that skips {skipped_ms:.3f}")
            st.close()
        out.free()

        if a.quality:
            qw, qh = 128, 72
            qscene = scenes.sponza_lights_powers(lights, 1, qw, qh)
            qs = R.SceneStage(ctx, qscene)
            buf = ctx.alloc(qw * qh * 16).zero()
            dist = DistributionParams((qw, qh), DISTRIBUTION_DUPLICATE, 0, 1, True)
            st = R.DirectStage(ctx, qs, R.options_for_scene(qscene, samples_per_pixel=4096, samples_per_pass=1, rng_seed=999), dist)
            st.run(buf)
            ref = buf.download((qh, qw, 4))[..., :3].astype(np.float64)
            st.close()

            def restir_mse(seed, **more):
                st = R.RestirDiStage(ctx, qs, (qw, qh), 1, R.restir_di_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, **more))
                for _ in range(9):
                    st.run([0], buf)
                mse = np.mean((buf.download((qh, qw, 4))[..., :3].astype(np.float64) - ref) ** 2)
                st.close()
                return mse
            cases = [("uniform", {})] + [(f"power, uniform_fraction {f}", dict(light_selection="power", uniform_fraction=f)) for f in FRACTIONS]
            uniform = None
            for name, more in cases:
                mse = [restir_mse(seed, **more) for seed in range(1, 9)]
                uniform = np.mean(mse) if uniform is None else uniform
                print(f"quality at {qw} x {qh}, {lights} lights, 8 seeds, frame 8 of the defaults, MSE against the direct stage at 4096 spp: {name}: {np.mean(mse):.4e} "
                      f"(per seed {np.min(mse):.4e} ... {np.max(mse):.4e}); against uniform: ratio {np.mean(mse) / uniform:.3f}")
            buf.free()


if __name__ == "__main__":
    main()
