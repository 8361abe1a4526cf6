#!/usr/bin/env python3
"""ReSTIR DI on sponza_lights at 1920 x 1080: device ms of the two kernels and of the stage, for candidates 1 / 4 / 8 at the default two
spatial samples and for spatial samples 0 / 2 / 4 at the default four candidates, with the direct stage at samples_per_pixel = candidates
next to them.  Warm-up frames first, then --frames timed frames of a running sequence (temporal reuse has history); every figure is the
median with the spread (min ... max) next to it.  With --quality it also prints the mean squared error against a converged direct-stage
image that tests/test_restir_di.py asserts on (128 x 72, 8 seeds).  No threshold: the record, profiles/r16/restir_di.txt, is the next
change's baseline.

With --visibility MODE[,MODE...] (per-target, shared, sampled: trhip_restir_di_set_visibility) a block of rows per mode follows: the five
configurations above, the candidate sweep on to 32 and --restir=32,4; with --quality also the mode's MSE at the defaults and, for shared
and sampled when per-target is among the modes, at the candidate count of the sweep whose stage time is closest to per-target's at the
defaults.  The record: profiles/r26/restir_di_visibility.txt.

usage: python tools/restir_di_probe.py [--lights 64] [--frames 20] [--warmup 5] [--quality] [--visibility MODE[,MODE...]]
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
    ap.add_argument("--lights", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--visibility", default="", help="per-target, shared, sampled: a block of rows per mode")
    a = ap.parse_args()
    modes = [m for m in a.visibility.split(",") if m]

    from tauray_amd import _lib, renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_DUPLICATE, DistributionParams

    w, h = 1920, 1080
    scene = scenes.sponza_lights(a.lights, 1, w, h)
    ctx = R.Context(0)
    ss = R.SceneStage(ctx, scene)
    base = R.options_for_scene(scene)
    print(f"== {scene.name} ({ss.accel['triangle_count']} triangles, {len(scene.point_lights)} point lights), {w} x {h}, {a.warmup} warm-up and {a.frames} timed frames, "
          f"build {_lib.lib().trhip_build_id():016x}")
    print("   device ms, median (min ... max)")
    out = ctx.alloc(w * h * 16).zero()

    def restir(candidates, spatial, **more):
        st = R.RestirDiStage(ctx, ss, (w, h), 1, R.restir_di_options(candidates=candidates, spatial_samples=spatial, min_ray_dist=base.min_ray_dist, **more), base.projection)
        rows = []
        for f in range(a.warmup + a.frames):
            st.run([0], out)
            ctx.sync()
            if f >= a.warmup:
                t = st.timings()
                rows.append((t["canonical_ms"], t["spatial_ms"], t["total_ms"]))
        st.close()
        rows = np.array(rows)
        return rows[:, 0], rows[:, 1], rows[:, 2]

    def direct(spp):
        st = R.DirectStage(ctx, ss, R.copy_options(base, samples_per_pixel=spp, samples_per_pass=1), DistributionParams((w, h), DISTRIBUTION_DUPLICATE, 0, 1, True))
        rows = []
        for f in range(a.warmup + a.frames):
            st.reset_accumulated_samples()
            st.run(out)
            ctx.sync()
            if f >= a.warmup:
                rows.append(st.timings()["path_tracing_ms"])
        st.close()
        return rows

    for candidates, spatial in ((1, 2), (4, 2), (8, 2), (4, 0), (4, 4)):
        c, s, t = restir(candidates, spatial)
        print(f"restir-di candidates {candidates} spatial_samples {spatial}: [restir di canonical] {spread(c)}  [restir di spatial] {spread(s)}  stage {spread(t)}")
    for spp in (1, 4, 8):
        print(f"direct stage samples_per_pixel {spp}: {spread(direct(spp))}")
    stage_ms = {}       # (mode, candidates) at two spatial samples -> median stage ms
    for mode in modes:
        for candidates, spatial in ((1, 2), (4, 2), (8, 2), (32, 2), (4, 0), (4, 4), (32, 4)):
            c, s, t = restir(candidates, spatial, visibility=mode)
            if spatial == 2:
                stage_ms[(mode, candidates)] = float(np.median(t))
            print(f"restir-di visibility {mode} candidates {candidates} spatial_samples {spatial}: [restir di canonical] {spread(c)}  [restir di spatial] {spread(s)}  stage {spread(t)}")
    out.free()

    if a.quality:
        qw, qh = 128, 72
        qscene = scenes.sponza_lights(a.lights, 1, qw, qh)
        qs = R.SceneStage(ctx, qscene)
        buf = ctx.alloc(qw * qh * 16).zero()
        dist = DistributionParams((qw, qh), DISTRIBUTION_DUPLICATE, 0, 1, True)

        def direct_image(spp, seed):
            st = R.DirectStage(ctx, qs, R.options_for_scene(qscene, samples_per_pixel=spp, samples_per_pass=1, rng_seed=seed), dist)
            st.run(buf)
            img = buf.download((qh, qw, 4))[..., :3].astype(np.float64)
            st.close()
            return img
        ref = direct_image(4096, 999)

        def restir_mse(seed, **more):
            st = R.RestirDiStage(ctx, qs, (qw, qh), 1, R.restir_di_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, **more))
            for _ in range(9):
                st.run([0], buf)
            mse = np.mean((buf.download((qh, qw, 4))[..., :3].astype(np.float64) - ref) ** 2)
            st.close()
            return mse
        mse_r, mse_d = [], []
        for seed in range(1, 9):
            mse_r.append(restir_mse(seed))
            mse_d.append(np.mean((direct_image(4, seed) - ref) ** 2))
        print(f"quality at {qw} x {qh}, 8 seeds, MSE against the direct stage at 4096 spp: restir-di defaults, frame 8: {np.mean(mse_r):.4e}; direct stage at 4 spp: {np.mean(mse_d):.4e}; "
              f"ratio {np.mean(mse_r) / np.mean(mse_d):.3f}")
        for mode in modes:
            counts = [4]
            if mode != "per-target" and ("per-target", 4) in stage_ms:
                counts.append(min((1, 4, 8, 32), key=lambda c: abs(stage_ms[(mode, c)] - stage_ms[("per-target", 4)])))
            for candidates in counts:
                mse = [restir_mse(seed, visibility=mode, candidates=candidates) for seed in range(1, 9)]
                note = "" if candidates == 4 else f" (the count whose stage time, {stage_ms[(mode, candidates)]:.3f} ms, is closest to per-target's {stage_ms[('per-target', 4)]:.3f} ms at the defaults)"
                print(f"quality at {qw} x {qh}, 8 seeds, visibility {mode}, candidates {candidates}{note}, frame 8: MSE {np.mean(mse):.4e} "
                      f"(per seed {np.min(mse):.4e} ... {np.max(mse):.4e}); against the direct stage at 4 spp: ratio {np.mean(mse) / np.mean(mse_d):.3f}")


if __name__ == "__main__":
    main()
