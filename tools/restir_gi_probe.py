#!/usr/bin/env python3
"""ReSTIR GI on sponza_lights at 1920 x 1080: device ms of the three kernels and of the stage at the defaults and at spatial samples 0 / 2 /
4, with the ReSTIR DI stage (the renderer's direct half) and the path tracer at 1 sample per pixel with the same number of bounces
(max_bounces = 3: direct light plus one bounce) next to them.  Warm-up frames first, then --frames timed frames of a running sequence
(temporal reuse has history); every figure is the median with the spread (min ... max) next to it.  With --quality it also prints, at
128 x 72 over 8 seeds, the mean squared error of frame 8 of the restir-gi renderer's frame (DI + GI) and of the path tracer at 1 spp
against the path tracer's converged frame (the mean of 4096 frames at 1 spp, non-finite samples left out), and of the GI stage alone with and without reuse
against its own converged indirect light, as tests/test_restir_gi.py asserts on.  No threshold: the comparison points are the same
commit's DI stage and path tracer in the same process, and the record, profiles/r20/restir_gi.txt, is the next change's baseline.
With --bounces 1,2,3,4 the stage at its defaults is timed once per listed path length (trhip_restir_gi_set_bounces) next to the path
tracer at the matching max_bounces (bounces + 2), and --quality adds, per listed length above 1, the GI stage's image mean and the two
mean squared errors against its own converged image at that length (profiles/r24/restir_gi_bounces.txt).

usage: python tools/restir_gi_probe.py [--lights 64] [--frames 20] [--warmup 5] [--quality] [--bounces 1,2,3,4]
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
    ap.add_argument("--bounces", default="1", help="comma-separated path lengths of the GI stage, each 1..8")
    a = ap.parse_args()
    lengths = [int(b) for b in a.bounces.split(",")]
    if not lengths or any(b < 1 or b > 8 for b in lengths):
        ap.error("--bounces: every length is a whole number in 1..8")

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

    def restir_gi(spatial, temporal=True, bounces=1):
        st = R.RestirGiStage(ctx, ss, (w, h), 1, R.restir_gi_options(spatial_samples=spatial, temporal_reuse=temporal, min_ray_dist=base.min_ray_dist, bounces=bounces),
                             base.projection)
        rows = []
        for f in range(a.warmup + a.frames):
            st.run([0], None, out)
            ctx.sync()
            if f >= a.warmup:
                t = st.timings()
                rows.append((t["initial_ms"], t["temporal_ms"], t["spatial_ms"], t["total_ms"]))
        st.close()
        return np.array(rows).T

    def restir_di():
        st = R.RestirDiStage(ctx, ss, (w, h), 1, R.restir_di_options(min_ray_dist=base.min_ray_dist), base.projection)
        rows = []
        for f in range(a.warmup + a.frames):
            st.run([0], out)
            ctx.sync()
            if f >= a.warmup:
                rows.append(st.timings()["total_ms"])
        st.close()
        return rows

    def path_tracer(bounces):
        st = R.PathTracerStage(ctx, ss, R.copy_options(base, samples_per_pixel=1, samples_per_pass=1, max_bounces=bounces), DistributionParams((w, h), DISTRIBUTION_DUPLICATE, 0, 1, True))
        rows = []
        for f in range(a.warmup + a.frames):
            st.reset_accumulated_samples()
            st.run(out)
            ctx.sync()
            if f >= a.warmup:
                rows.append(st.timings()["path_tracing_ms"])
        st.close()
        return rows

    for spatial, temporal in ((2, True), (0, True), (4, True), (0, False)):
        i, t, s, total = restir_gi(spatial, temporal)
        print(f"restir-gi spatial_samples {spatial} temporal_reuse {'on' if temporal else 'off'}: [restir gi initial] {spread(i)}  [restir gi temporal] {spread(t)}  "
              f"[restir gi spatial] {spread(s)}  stage {spread(total)}")
    print(f"restir-di stage at its defaults (4 candidates, 2 spatial samples): {spread(restir_di())}")
    for bounces in (2, 3):
        print(f"path tracer, 1 spp, max_bounces {bounces}: {spread(path_tracer(bounces))}")
    if lengths != [1]:
        for b in lengths:
            i, t, s, total = restir_gi(2, True, b)
            print(f"restir-gi bounces {b} at its defaults: [restir gi initial] {spread(i)}  stage {spread(total)}  |  path tracer, 1 spp, max_bounces {b + 2}: "
                  f"{spread(path_tracer(b + 2))}")
    out.free()

    if a.quality:
        qw, qh = 128, 72
        qscene = scenes.sponza_lights(a.lights, 1, qw, qh)
        qs = R.SceneStage(ctx, qscene)
        buf = ctx.alloc(qw * qh * 16).zero()
        dist = DistributionParams((qw, qh), DISTRIBUTION_DUPLICATE, 0, 1, True)

        def traced(spp, seed):
            st = R.PathTracerStage(ctx, qs, R.options_for_scene(qscene, samples_per_pixel=spp, samples_per_pass=1, max_bounces=3, rng_seed=seed), dist)
            st.run(buf)
            img = buf.download((qh, qw, 4))[..., :3].astype(np.float64)
            st.close()
            return img
        # The path tracer's estimator yields a rare non-finite sample (tools/find_nonfinite.py), which an accumulation keeps: the converged
        # frame is the mean of N frames at 1 spp, each with a seed of its own, over the samples that are finite
        N = 4096
        total, count = np.zeros((qh, qw, 3)), np.zeros((qh, qw, 1))
        for seed in range(5001, 5001 + N):
            one = traced(1, seed)
            fin = np.isfinite(one).all(-1, keepdims=True)
            total += np.where(fin, one, 0.0)
            count += fin
        ref = total / np.maximum(count, 1)
        ok = count[..., 0] > 0
        print(f"quality at {qw} x {qh}, 8 seeds; the path tracer's converged frame: {N} frames at 1 spp, max_bounces 3, {int(count.size * N - count.sum())} non-finite samples left out")
        gi_ref = np.zeros((qh, qw, 3))
        N = 2048
        for seed in range(1001, 1001 + N):
            st = R.RestirGiStage(ctx, qs, (qw, qh), 1, R.restir_gi_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, spatial_samples=0, temporal_reuse=False))
            st.run([0], None, buf)
            gi_ref += buf.download((qh, qw, 4))[..., :3].astype(np.float64) / N
            st.close()
        mse = dict(renderer=[], pt=[], gi=[], gi_alone=[])
        for seed in range(1, 9):
            rr = R.RestirGiRenderer(ctx, qs, qscene, (qw, qh), R.restir_gi_options(rng_seed=seed, min_ray_dist=base.min_ray_dist),
                                    R.restir_di_options(rng_seed=seed, min_ray_dist=base.min_ray_dist))
            for _ in range(9):
                rr.render(tonemap=False)
            frame = rr.download("color")[0][..., :3].astype(np.float64)
            rr.close()
            one = traced(1, seed)
            both = ok & np.isfinite(one).all(-1)
            mse["renderer"].append(np.mean((frame[both] - ref[both]) ** 2))
            mse["pt"].append(np.mean((one[both] - ref[both]) ** 2))
            for name, options, frames in (("gi", {}, 9), ("gi_alone", dict(spatial_samples=0, temporal_reuse=False), 1)):
                st = R.RestirGiStage(ctx, qs, (qw, qh), 1, R.restir_gi_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, **options))
                for _ in range(frames):
                    st.run([0], None, buf)
                mse[name].append(np.mean((buf.download((qh, qw, 4))[..., :3].astype(np.float64) - gi_ref) ** 2))
                st.close()
        print(f"MSE of a frame against the path tracer's converged frame: restir-gi renderer (DI + GI) at its defaults, frame 8: {np.mean(mse['renderer']):.4e}; "
              f"path tracer at 1 spp, max_bounces 3: {np.mean(mse['pt']):.4e}; ratio {np.mean(mse['renderer']) / np.mean(mse['pt']):.3f}")
        print(f"   (the path tracer sees the sphere lights as spheres, the two stages light with points: part of the renderer's error is that difference, not noise)")
        print(f"MSE of the indirect light against the GI stage's own converged image ({N} frames without reuse): defaults, frame 8: {np.mean(mse['gi']):.4e}; "
              f"no reuse: {np.mean(mse['gi_alone']):.4e}; ratio {np.mean(mse['gi']) / np.mean(mse['gi_alone']):.3f}")
        for b in (b for b in lengths if b > 1):
            own, N = np.zeros((qh, qw, 3)), 1024
            for seed in range(1001, 1001 + N):
                st = R.RestirGiStage(ctx, qs, (qw, qh), 1, R.restir_gi_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, spatial_samples=0, temporal_reuse=False, bounces=b))
                st.run([0], None, buf)
                own += buf.download((qh, qw, 4))[..., :3].astype(np.float64) / N
                st.close()
            err = dict(gi=[], gi_alone=[])
            for seed in range(1, 9):
                for name, options, frames in (("gi", {}, 9), ("gi_alone", dict(spatial_samples=0, temporal_reuse=False), 1)):
                    st = R.RestirGiStage(ctx, qs, (qw, qh), 1, R.restir_gi_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, bounces=b, **options))
                    for _ in range(frames):
                        st.run([0], None, buf)
                    err[name].append(np.mean((buf.download((qh, qw, 4))[..., :3].astype(np.float64) - own) ** 2))
                    st.close()
            print(f"bounces {b}: indirect image mean {own.mean():.4e} ({own.mean() / gi_ref.mean():.3f} x one bounce's, {N} frames without reuse); MSE against it: "
                  f"defaults, frame 8: {np.mean(err['gi']):.4e}; no reuse: {np.mean(err['gi_alone']):.4e}; ratio {np.mean(err['gi']) / np.mean(err['gi_alone']):.3f}")


if __name__ == "__main__":
    main()
