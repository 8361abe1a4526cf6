#!/usr/bin/env python3
"""Sparse light field against the full render, BASELINE config 5's shape: sponza_class at 1920x1080, the 9 x 5 camera grid (spacing 0.02,
recentering distance 5), the centre row's nine views active (RtRenderer(spatial_reprojection=[18..26])).

One process, two renderers on one device; after 3 warm-up frames of each, `--rounds` rounds alternate a full and a sparse frame.  A frame's
time is host wall time around render() + sync (the frame's launches back to back, nothing else on the device).  Per-stage device times come
from the stages' own event timers (path tracer, spatial stage); the G-buffer pass has none and is timed on the host around its launch + sync.
RMS: the reprojected views `--rms-views` against `--reference-spp` samples of the same views, next to a 1-spp path-traced render of them.

The figures go into the section of profiles/r11/reprojection.txt between the two marker lines below (the rest of the file is kept).

    python tools/sparse_lightfield_probe.py [--out profiles/r11/reprojection.txt] [--rounds 10] [--rms-views 0,13,31,44]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "== tools/sparse_lightfield_probe.py", "== end of tools/sparse_lightfield_probe.py"


def write_section(path, text):
    """Replaces the probe's section of the file (or appends it)."""
    old = open(path).read() if os.path.exists(path) else ""
    section = BEGIN + "\n" + text + END + "\n"
    if BEGIN in old and END in old:
        head, rest = old.split(BEGIN, 1)
        new = head + section + rest.split(END + "\n", 1)[-1]
    else:
        new = old + ("\n" if old and not old.endswith("\n\n") else "") + section
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "reprojection.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--rms-views", default="0,13,31,44")
    ap.add_argument("--reference-spp", type=int, default=1024)
    args = ap.parse_args()

    from tauray_amd import renderer as R
    from tauray_amd import scenes
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    from tauray_amd.scene import generate_camera_grid

    W, H, V = args.width, args.height, 45
    sources = list(range(18, 27))
    scene = scenes.sponza_class(width=W, height=H)
    scene.cameras = generate_camera_grid(scene.cameras[0], 9, 5, 0.02, 0.02, 5.0)
    opt = R.options_for_scene(scene, max_bounces=args.bounces)
    ctx = R.Context(0)
    full = R.RtRenderer(ctx, scene, opt, (W, H), viewports=V, use_torch=False)
    sparse = R.RtRenderer(ctx, scene, opt, (W, H), viewports=V, use_torch=False, spatial_reprojection=sources)

    def frame(r):
        r.sync()
        t0 = time.perf_counter()
        r.render(tonemap=False)
        r.sync()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(3):
        frame(full)
        frame(sparse)
    t_full, t_sparse, pt_full, pt_sparse, spatial_ms = [], [], [], [], []
    for _ in range(args.rounds):
        t_full.append(frame(full))
        pt_full.append(full.timings()["path_tracing_ms"])
        t_sparse.append(frame(sparse))
        pt_sparse.append(sparse.timings()["path_tracing_ms"])
        spatial_ms.append(sparse.post.spatial.timings()["total_ms"])
    gb = []
    for _ in range(args.rounds):
        ctx.sync()
        t0 = time.perf_counter()
        sparse.post.gbuffer.run(sparse.post.spatial.destinations, sparse.post.destination_targets)
        ctx.sync()
        gb.append((time.perf_counter() - t0) * 1e3)
    dec = sparse.post.spatial.decisions()
    filled = float((dec["kind"] != 0).mean())
    sparse_frame = sparse.download("color")
    ss = sparse.scene_update

    def fmt(name, xs):
        return f"{name}: median {np.median(xs):.3f} ms [min {min(xs):.3f} .. max {max(xs):.3f}] over {len(xs)} rounds"
    lines = [f"sparse light field probe: sponza_class {W}x{H}, 45 views (9 x 5 grid, spacing 0.02), {args.bounces} bounces, 1 spp, sources {sources}",
             fmt("full frame (45 views path traced), host wall time", t_full),
             fmt("sparse frame (9 views path traced + G-buffer pass of 36 + spatial stage), host wall time", t_sparse),
             f"ratio full / sparse (medians): {np.median(t_full) / np.median(t_sparse):.2f}",
             fmt("  path tracer, 45 views (stage timer)", pt_full),
             fmt("  path tracer, 9 views (stage timer)", pt_sparse),
             fmt("  G-buffer pass, 36 views (host wall time around launch + sync)", gb),
             fmt("  spatial stage (stage timer)", spatial_ms),
             f"destination pixels filled (reprojected or copied sky): {filled:.2%}"]

    # RMS of reprojected views against many samples of the same views, next to a 1-spp path-traced render of them
    dup = DistributionParams((W, H), DISTRIBUTION_DUPLICATE, 0, 1, True)
    one_spp = full.download("color")
    for v in [int(x) for x in args.rms_views.split(",") if x != ""]:
        if v in sources:
            continue
        pt = R.PathTracerStage(ctx, ss, opt, dup)
        pt.set_shard(viewport_base=v, viewport_stride=1)
        buf = ctx.alloc(W * H * 16).zero()
        for _ in range(args.reference_spp):
            pt.run(buf, 1)
        ref = buf.download((H, W, 4))
        pt.close()
        rp = sparse_frame[v]
        ok = np.isfinite(ref).all(-1) & np.isfinite(rp).all(-1) & np.isfinite(one_spp[v]).all(-1)

        def rms(a):
            d = (a[..., :3].astype(np.float64) - ref[..., :3])[ok]
            return float(np.sqrt((d * d).mean()))
        lines.append(f"view {v}: RMS against {args.reference_spp} spp over the {ok.mean():.1%} of its pixels that were filled: reprojected {rms(rp):.4f}, "
                     f"1 spp path traced {rms(one_spp[v]):.4f}")
    full.close()
    sparse.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    write_section(args.out, text)


if __name__ == "__main__":
    main()
