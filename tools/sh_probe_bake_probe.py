#!/usr/bin/env python3
"""Bakes a 16 x 16 x 16 grid of light probes with 512 samples each in sponza_class (the grid's box is the scene's bounds) and prints the
device time of the stage, of its kernels and the rays per second from the stage's counters - next to the camera path tracer's rate on
the same scene in the same process.  The path-id order of a batch is a compile-time choice of the library (TR_SH_SAMPLE_MAJOR,
csrc/sh_probes.h): run the tool once per build, the other one through TRHIP_LIB=tauray_amd/libtrhip_sample_major.so (the Makefile
links it next to libtrhip.so), with --label saying which.  The record is profiles/r16/sh_probes.txt.

usage: python tools/sh_probe_bake_probe.py [--label TEXT] [--resolution 16] [--samples 512] [--order 2] [--bounces 4] [--renders 5] [--hash]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--renders", type=int, default=5)
    ap.add_argument("--hash", action="store_true", help="print a hash of the first render's grid (the same bits for both path-id orders)")
    a = ap.parse_args()

    from tauray_amd import _lib, renderer as R, scenes
    from tauray_amd.distribution import DISTRIBUTION_DUPLICATE, DistributionParams
    from tauray_amd.scene import ShGrid

    scene = scenes.sponza_class()
    ctx = R.Context(0)
    ss = R.SceneStage(ctx, scene)
    lo, hi = np.array(ss.accel["bounds_min"], dtype=np.float64), np.array(ss.accel["bounds_max"], dtype=np.float64)
    half = 0.5 * (hi - lo)
    transform = np.eye(4)
    transform[:3, :3] = np.diag(half)
    transform[:3, 3] = 0.5 * (hi + lo)
    grid = ShGrid(resolution=(a.resolution,) * 3, transform=transform, scaling=tuple(half))
    weights = R.options_for_scene(scene)
    options = dict(max_bounces=a.bounces, samples_per_probe=a.samples, sh_order=a.order, film=R.FILM_POINT, temporal_ratio=0.0,
                   nee_point=weights.nee_point, nee_directional=weights.nee_directional, nee_envmap=weights.nee_envmap, nee_triangles=weights.nee_triangles)
    print(f"== {a.label or os.environ.get('TRHIP_LIB', 'libtrhip.so')}: {a.resolution}^3 probes x {a.samples} samples, order {a.order}, {a.bounces} bounces, "
          f"sponza_class ({ss.accel['triangle_count']} triangles), build {_lib.lib().trhip_build_id():016x}")

    st = R.ShPathTracerStage(ctx, ss, grid, options)
    st.run()      # the first render allocates the path state and classifies the streams
    ctx.sync()
    if a.hash:
        print(f"grid sha256 {hashlib.sha256(st.download('grid').tobytes()).hexdigest()[:16]}, half {hashlib.sha256(st.download('half').tobytes()).hexdigest()[:16]}")
    base = st.counters()
    ms = []
    for _ in range(a.renders):
        st.run()
        ms.append(st.timings()["total_ms"])
    c = st.counters()
    rays = (c["closest_rays"] + c["shadow_rays"] - base["closest_rays"] - base["shadow_rays"]) / a.renders
    best = min(ms)
    print(f"stage, lanes automatic: {' '.join(f'{m:.3f}' for m in ms)} ms per render (min {best:.3f}); {rays / 1e6:.2f} Mrays per render "
          f"({(c['closest_rays'] - base['closest_rays']) / a.renders / 1e6:.2f} closest, {(c['shadow_rays'] - base['shadow_rays']) / a.renders / 1e6:.2f} shadow); "
          f"{rays / best / 1e3:.0f} Mray/s")
    # per kernel: one lane, one stream, an event pair around every launch
    st.set_profiling(detailed_timing=True)
    st.run()
    t = st.timings()
    names = ("raygen_ms", "trace_closest_ms", "trace_shadow_ms", "shade_ms", "project_ms")
    print("kernels alone (detailed timing: one lane, launches serialised): " + ", ".join(f"{n[:-3]} {t[n]:.3f} ms" for n in names) +
          f"; total {t['total_ms']:.3f} ms; trace {rays / max(t['trace_closest_ms'] + t['trace_shadow_ms'], 1e-9) / 1e3:.0f} Mray/s")
    st.close()

    # the camera path tracer on the same scene: 1920 x 1080, one sample per pixel, the same bounces
    w, h = 1920, 1080
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=a.bounces), DistributionParams((w, h), DISTRIBUTION_DUPLICATE, 0, 1, True))
    color = ctx.alloc(w * h * 16).zero()
    pt.run(color)
    ctx.sync()
    pt.reset_counters()
    ms = []
    for _ in range(a.renders):
        pt.reset_accumulated_samples()
        pt.run(color)
        ms.append(pt.timings()["path_tracing_ms"])
    c = pt.counters()
    rays = (c["closest_rays"] + c["shadow_rays"]) / a.renders
    print(f"camera path tracer, 1920x1080, 1 spp: {' '.join(f'{m:.3f}' for m in ms)} ms per frame (min {min(ms):.3f}); {rays / 1e6:.2f} Mrays per frame; "
          f"{rays / min(ms) / 1e3:.0f} Mray/s")
    pt.close()


if __name__ == "__main__":
    main()
