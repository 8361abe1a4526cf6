#!/usr/bin/env python3
"""ReSTIR DI's sphere lights as area lights (trhip_restir_di_set_sphere_lights) on sponza_lights with 64 lamps -
nine in ten of them have a radius, log-uniform in 1e-3 .. 0.2 - at 1920 x 1080: device ms of the canonical kernel, the spatial kernel
and the stage at the defaults in point and in area mode (warm-up frames first, then --frames timed frames of a running sequence; median
with the spread, min ... max, next to it; --repeats stages one after the other, each with its own median, give the run-to-run spread).
With --quality: the frame-8 mean squared error at 128 x 72 against a 4096 spp direct-stage image of both modes at equal candidates, over
8 seeds.  No threshold: the record is profiles/r29/restir_sphere_lights.txt.

With TRHIP_LIB naming an older build of the library and --modes point, the rows come from that build (it is never told a mode): the
default frame's times against the parent commit.

usage: python tools/restir_sphere_lights_probe.py [--frames 20] [--warmup 5] [--repeats 3] [--modes point,area] [--quality]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return f"{np.median(v):8.3f} ({v.min():.3f} ... {v.max():.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="point,area")
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]

    from tauray_amd import _lib, renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_DUPLICATE, DistributionParams

    w, h = 1920, 1080
    ctx = R.Context(0)
    scene = scenes.sponza_lights(64, 1, w, h)
    ss = R.SceneStage(ctx, scene)
    base = R.options_for_scene(scene)
    with_radius = int((scene.point_lights["radius"] != 0).sum())
    print(f"== {scene.name} ({ss.accel['triangle_count']} triangles, {len(scene.point_lights)} point lights, {with_radius} of them with a radius), "
          f"{w} x {h}, {a.warmup} warm-up and {a.frames} timed frames, {a.repeats} stages a mode, library {os.path.basename(_lib.LIB_PATH)}, build {_lib.lib().trhip_build_id():016x}")
    print("   device ms, median (min ... max)")
    out = ctx.alloc(w * h * 16).zero()
    for mode in modes:
        more = dict(sphere_lights=mode) if mode != "point" else {}      # an older library has no setter: point is never told
        medians = []
        for rep in range(a.repeats):
            st = R.RestirDiStage(ctx, ss, (w, h), 1, R.restir_di_options(min_ray_dist=base.min_ray_dist, **more), base.projection)
            rows = []
            for f in range(a.warmup + a.frames):
                st.run([0], out)
                ctx.sync()
                if f >= a.warmup:
                    t = st.timings()
                    rows.append((t["canonical_ms"], t["spatial_ms"], t["total_ms"]))
            st.close()
            rows = np.array(rows)
            medians.append(np.median(rows, 0))
            print(f"restir-di defaults, {mode}, stage {rep}: [restir di canonical] {spread(rows[:, 0])}  [restir di spatial] {spread(rows[:, 1])}  stage {spread(rows[:, 2])}")
        medians = np.array(medians)
        print(f"   {mode}: medians of the {a.repeats} stages: canonical {spread(medians[:, 0])}  spatial {spread(medians[:, 1])}  stage {spread(medians[:, 2])}")
    out.free()

    if a.quality:
        qw, qh = 128, 72
        qscene = scenes.sponza_lights(64, 1, qw, qh)
        qs = R.SceneStage(ctx, qscene)
        buf = ctx.alloc(qw * qh * 16).zero()
        dist = DistributionParams((qw, qh), DISTRIBUTION_DUPLICATE, 0, 1, True)
        st = R.DirectStage(ctx, qs, R.options_for_scene(qscene, samples_per_pixel=4096, samples_per_pass=1, rng_seed=999), dist)
        st.run(buf)
        ref = buf.download((qh, qw, 4))[..., :3].astype(np.float64)
        st.close()
        first = None
        for mode in modes:
            mse = []
            for seed in range(1, 9):
                st = R.RestirDiStage(ctx, qs, (qw, qh), 1, R.restir_di_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, sphere_lights=mode))
                for _ in range(9):
                    st.run([0], buf)
                mse.append(np.mean((buf.download((qh, qw, 4))[..., :3].astype(np.float64) - ref) ** 2))
                st.close()
            first = np.mean(mse) if first is None else first
            print(f"quality at {qw} x {qh}, 8 seeds, frame 8 of the defaults (4 candidates), MSE against the direct stage at 4096 spp: {mode}: {np.mean(mse):.4e} "
                  f"(per seed {np.min(mse):.4e} ... {np.max(mse):.4e}); against {modes[0]}: ratio {np.mean(mse) / first:.3f}")
        buf.free()


if __name__ == "__main__":
    main()
