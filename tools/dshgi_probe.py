#!/usr/bin/env python3
"""One DDISH-GI frame of sponza_class at 1920 x 1080 with a 16 x 16 x 16 grid of light probes over the scene's bounds: device ms of the bake,
of the direct stage and of k_dshgi_indirect, in both interpolation modes and at orders 2 and 4 - next to k_gbuffer for the same frame (the
first hit alone: the difference is the cost of the lookup) and the path tracer's frame at the same depth.  With --end-to-end it also prints
the image means of the lit box of tests/test_dshgi.py.  No threshold: the record, profiles/r17/dshgi.txt, is the next change's baseline.

usage: python tools/dshgi_probe.py [--resolution 16] [--samples 512] [--bounces 4] [--frames 5] [--end-to-end]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--end-to-end", action="store_true")
    a = ap.parse_args()

    from tauray_amd import _lib, renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_DUPLICATE, DistributionParams
    from tauray_amd.scene import ShGrid

    w, h = 1920, 1080
    scene = scenes.sponza_class(width=w, height=h)
    ctx = R.Context(0)
    ss = R.SceneStage(ctx, scene)
    lo, hi = np.array(ss.accel["bounds_min"], dtype=np.float64), np.array(ss.accel["bounds_max"], dtype=np.float64)
    half = 0.5 * (hi - lo)
    transform = np.eye(4)
    transform[:3, :3] = np.diag(half)
    transform[:3, 3] = 0.5 * (hi + lo)
    opt = R.options_for_scene(scene, max_bounces=a.bounces)
    print(f"== sponza_class ({ss.accel['triangle_count']} triangles), {w} x {h}, {a.resolution}^3 probes x {a.samples} samples, {a.bounces} bounces, "
          f"build {_lib.lib().trhip_build_id():016x}")
    for order in (2, 4):
        for visibility in (False, True):
            scene.sh_grids = [ShGrid(resolution=(a.resolution,) * 3, transform=transform, scaling=tuple(half))]
            sh = dict(max_bounces=a.bounces, samples_per_probe=a.samples, sh_order=order, film=R.FILM_POINT, temporal_ratio=0.0, nee_point=opt.nee_point,
                      nee_directional=opt.nee_directional, nee_envmap=opt.nee_envmap, nee_triangles=opt.nee_triangles)
            rr = R.DshgiRenderer(ctx, ss, scene, (w, h), opt, sh=sh, use_probe_visibility=visibility)
            rr.render()      # the first frame allocates the path state and loads the code objects
            ctx.sync()
            rows = []
            for _ in range(a.frames):
                rr.render()
                ctx.sync()
                t = rr.timings()
                rows.append((t["bake"][0]["total_ms"], t["direct"]["path_tracing_ms"], t["indirect"]["total_ms"]))
            best = np.min(np.array(rows), axis=0)
            img = rr.download("color")
            print(f"order {order}, {'probe visibility' if visibility else 'trilinear'}: bake {best[0]:.3f} ms, direct stage {best[1]:.3f} ms, k_dshgi_indirect {best[2]:.3f} ms "
                  f"(min of {a.frames}; k_dshgi_indirect per frame: {' '.join(f'{r[2]:.3f}' for r in rows)}); image mean {float(img[..., :3].mean()):.5f}")
            rr.close()

    # the first hit alone: k_gbuffer writing pos only (a host clock around 20 launches that end in a synchronise)
    gb = R.GbufferStage(ctx, ss, (w, h), opt.projection, opt.min_ray_dist)
    targets = {"pos": ctx.alloc(w * h * 16).zero()}
    gb.run([0], targets)
    ctx.sync()
    per = []
    for _ in range(a.frames):
        t0 = time.perf_counter()
        for _ in range(20):
            gb.run([0], targets)
        ctx.sync()
        per.append((time.perf_counter() - t0) * 1e3 / 20)
    print(f"k_gbuffer, the same frame (pos target): {' '.join(f'{m:.3f}' for m in per)} ms per launch (min {min(per):.3f})")

    pt = R.PathTracerStage(ctx, ss, opt, DistributionParams((w, h), DISTRIBUTION_DUPLICATE, 0, 1, True))
    color = ctx.alloc(w * h * 16).zero()
    pt.run(color)
    ctx.sync()
    ms = []
    for _ in range(a.frames):
        pt.reset_accumulated_samples()
        pt.run(color)
        ms.append(pt.timings()["path_tracing_ms"])
    print(f"path tracer, the same frame, 1 spp, {a.bounces} bounces: {' '.join(f'{m:.3f}' for m in ms)} ms per frame (min {min(ms):.3f})")
    pt.close()

    if a.end_to_end:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_dshgi as T
        fresh = R.Context(0)
        full, direct_only, ref = T._end_to_end_means(R, fresh)
        print(f"lit box (tests/test_dshgi.py): image mean dshgi {full:.6f}, direct alone {direct_only:.6f}, path tracer {ref:.6f}: off by "
              f"{abs(full - ref) / ref:.4%} with the indirect term, {abs(direct_only - ref) / ref:.4%} without")


if __name__ == "__main__":
    main()
