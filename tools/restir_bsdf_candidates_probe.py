#!/usr/bin/env python3
"""ReSTIR DI's BSDF candidates (trhip_restir_di_set_bsdf_candidates) on sponza_lights with 64 lamps - the atrium
has an emissive mesh and an environment map next to them - at 1920 x 1080: device ms of the canonical kernel and of the stage at the
defaults with B = 0, 1, 2 BSDF candidates (warm-up frames first, then --frames timed frames of a running sequence; median with the
spread, min ... max, next to it), the canonical kernel's cost per BSDF candidate, and k_restir_gi_initial next to it, which traces the
same kind of ray once a pixel.  With --quality: the frame-8 mean squared error at 128 x 72 against a 4096 spp direct-stage image at
equal M = L + B, (4, 0) against (3, 1) and (2, 2), over 8 seeds.  No threshold: the record is profiles/r28/restir_bsdf_candidates.txt.

With TRHIP_LIB naming an older build of the library and --bsdf 0, the B = 0 rows come from that build: the default frame's times against
the parent commit.

usage: python tools/restir_bsdf_candidates_probe.py [--frames 20] [--warmup 5] [--bsdf 0,1,2] [--quality]
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
    ap.add_argument("--bsdf", default="0,1,2")
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    counts = [int(n) for n in a.bsdf.split(",") if n]

    from tauray_amd import _lib, renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_DUPLICATE, DistributionParams

    w, h = 1920, 1080
    ctx = R.Context(0)
    scene = scenes.sponza_lights(64, 1, w, h)
    ss = R.SceneStage(ctx, scene)
    base = R.options_for_scene(scene)
    print(f"== {scene.name} ({ss.accel['triangle_count']} triangles, {len(scene.point_lights)} point lights, {ss.accel['tri_light_count']} triangle lights, an environment map), "
          f"{w} x {h}, {a.warmup} warm-up and {a.frames} timed frames, library {os.path.basename(_lib.LIB_PATH)}, build {_lib.lib().trhip_build_id():016x}")
    print("   device ms, median (min ... max)")
    out = ctx.alloc(w * h * 16).zero()
    canonical = {}
    for n in counts:
        more = dict(bsdf_candidates=n) if n else {}      # an older library has no setter: B = 0 is never told
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
        canonical[n] = float(np.median(rows[:, 0]))
        print(f"restir-di defaults (L = 4), B = {n}: [restir di canonical] {spread(rows[:, 0])}  [restir di spatial] {spread(rows[:, 1])}  stage {spread(rows[:, 2])}")
    if 0 in canonical and len(canonical) > 1:
        print("   the canonical kernel's cost per BSDF candidate: " + ", ".join(f"B = {n}: {(canonical[n] - canonical[0]) / n:.3f} ms" for n in counts if n))
    st = R.RestirGiStage(ctx, ss, (w, h), 1, R.restir_gi_options(min_ray_dist=base.min_ray_dist), base.projection)
    rows = []
    for f in range(a.warmup + a.frames):
        st.run([0], None, out)
        ctx.sync()
        if f >= a.warmup:
            rows.append(st.timings()["initial_ms"])
    st.close()
    print(f"restir-gi defaults: [restir gi initial] {spread(rows)}  (the first hit, one cosine-hemisphere closest-hit ray and its light sample)")
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

        def restir_mse(seed, **more):
            st = R.RestirDiStage(ctx, qs, (qw, qh), 1, R.restir_di_options(rng_seed=seed, min_ray_dist=base.min_ray_dist, **more))
            for _ in range(9):
                st.run([0], buf)
            mse = np.mean((buf.download((qh, qw, 4))[..., :3].astype(np.float64) - ref) ** 2)
            st.close()
            return mse
        first = None
        for n_light, n_bsdf in ((4, 0), (3, 1), (2, 2)):
            mse = [restir_mse(seed, candidates=n_light, bsdf_candidates=n_bsdf) for seed in range(1, 9)]
            first = np.mean(mse) if first is None else first
            print(f"quality at {qw} x {qh}, 8 seeds, frame 8 of the defaults at M = 4, MSE against the direct stage at 4096 spp: L = {n_light}, B = {n_bsdf}: {np.mean(mse):.4e} "
                  f"(per seed {np.min(mse):.4e} ... {np.max(mse):.4e}); against L = 4, B = 0: ratio {np.mean(mse) / first:.3f}")
        buf.free()


if __name__ == "__main__":
    main()
