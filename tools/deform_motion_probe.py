#!/usr/bin/env python3
"""What the motion of deforming meshes costs (trhip_scene_set_deformation_motion / trhip_scene_latch_positions, k_latch_positions;
DESIGN.md section 24), on the mesh of tools/morph_probe.py: a 1000 x 1000 grid (1 M vertices, 2 M triangles) with a two-joint skin and 8
morph targets, all active.

  * `trhip_scene_latch_positions` alone: host wall time of one call (it synchronises the device before and after its kernel), next to a
    device-to-device copy of as many bytes as the plane holds, timed the same way, and the bytes the kernel asks for (12 read and 12
    written per vertex; the reads are 12 of every 48 bytes, so the memory system fetches more) over 8 TB/s, as profiles/r18/morph.txt does.
  * one frame of the mesh, morph + skin + refit, with and without the latch in front.
  * the consumers with the switch on and off: the launch of feature 8 (screen motion) and a path-traced frame with the screen_motion
    target, 1920 x 1080, wall time of launch + synchronisation.

    python tools/deform_motion_probe.py [--out profiles/r19/deform_motion.txt] [--calls 20]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_probe as MP      # noqa: E402 - the mesh

TARGETS, HBM_BYTES_PER_S, SIZE = 8, 8e12, (1920, 1080)


def measure(calls):
    from tauray_amd import _lib
    from tauray_amd import renderer as R
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    N = MP.N
    ctx = R.Context(0)
    sc, skins = MP.scene()
    sc.cameras[0].set_aspect(SIZE[0] / SIZE[1])
    ss = R.SceneStage(ctx, sc, deformation_motion=True)
    rng = np.random.default_rng(1)
    planes = [rng.random((TARGETS, N * N, 3), dtype=np.float32) * np.float32(0.01) for _ in range(3)]
    ss.set_skin(0, skins)
    ss.set_morph_targets(0, *planes)
    del planes
    joints = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)

    def pose(k):
        joints[1, :3, 3] = (0.1 + 0.01 * (k % 5), 0.0, 0.2)
        ss.morph(0, np.full(TARGETS, 0.5 + 0.01 * (k % 7), np.float32), refit=None)
        ss.skin(0, joints, refit=None)
        ss._accel_after_change(True)

    def timed(fn):
        out = []
        for k in range(calls + 3):
            ctx.sync()
            t0 = time.perf_counter()
            fn(k)
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out[3:])), float(min(out[3:]))
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f})"
    plane = N * N * 12
    pose(0)
    latch = timed(lambda k: ss.latch_positions())
    src, dst = ctx.alloc(plane).zero(), ctx.alloc(plane).zero()
    L = _lib.lib()
    copy = timed(lambda k: _lib.check(L.trhip_copy_peer(ctx.h, dst.data_ptr(), ctx.h, src.data_ptr(), plane, None)))
    floor = 2 * plane / HBM_BYTES_PER_S * 1e3
    frame_plain = timed(lambda k: pose(k))
    frame_latch = timed(lambda k: (ss.latch_positions(), pose(k)))
    lines = [f"device: {ctx.info()}",
             f"mesh: {N * N} vertices, {len(sc.indices) // 3} triangles, a two-joint skin and {TARGETS} morph targets x 3 planes, all active; {calls} calls, 3 warm-up; wall ms, median (min)",
             f"  trhip_scene_latch_positions (k_latch_positions) {fmt(latch)}   asks for {2 * plane / 1e6:.0f} MB: 12 of every 48 bytes of {N * N * 48 / 1e6:.0f} MB read, {plane / 1e6:.0f} MB written",
             f"  device-to-device copy of {plane / 1e6:.0f} MB (reads and writes {2 * plane / 1e6:.0f} MB) {fmt(copy)}",
             f"  {2 * plane / 1e6:.0f} MB at 8 TB/s: {floor:.4f} ms ({(N * N * 48 + plane) / HBM_BYTES_PER_S * 1e3:.4f} ms if every vertex is fetched whole); latch call / copy call: {latch[0] / copy[0]:.2f}",
             f"  frame: morph + skin + refit {fmt(frame_plain)}; latch + morph + skin + refit {fmt(frame_latch)}; difference {frame_latch[0] - frame_plain[0]:+.4f}",
             f"  the plane: {plane / 1e6:.0f} MB next to {N * N * 48 / 1e6:.0f} MB of vertices", ""]
    # the consumers
    dist = DistributionParams(SIZE, DISTRIBUTION_DUPLICATE, 0, 1, True)
    buf = ctx.alloc(SIZE[0] * SIZE[1] * 16).zero()
    feature = R.FeatureStage(ctx, ss, 8, dist)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=4), dist)
    targets = {"color": ctx.alloc(SIZE[0] * SIZE[1] * 16).zero(), "screen_motion": ctx.alloc(SIZE[0] * SIZE[1] * 8).zero()}

    def pt_frame(k):
        pt.reset_accumulated_samples()
        pt.run_targets(targets)
    results = {}
    for rnd in range(2):      # on, off, on, off: the second pair is the one to read, the first warms both up
        for on in (True, False):
            ss.set_deformation_motion(on)
            if on:
                ss.latch_positions()
                pose(rnd + 1)
            results[on] = (timed(lambda k: feature.run(buf)), timed(pt_frame))
    lines += [f"consumers at {SIZE[0]} x {SIZE[1]}, launch + synchronisation, wall ms, median (min):",
              f"  feature 8 (k_feature)                      switch on {fmt(results[True][0])}   off {fmt(results[False][0])}",
              f"  path-traced frame with screen_motion       switch on {fmt(results[True][1])}   off {fmt(results[False][1])}", ""]
    pt.close()
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "deform_motion.txt"))
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    text = measure(args.calls)
    print(text)
    write_section(args.out, "== tools/deform_motion_probe.py\n", text)


def write_section(path, header, text):
    """The file holds other records too (the resource report, the bench comparison): sections start with a line `== ...`; this one is
    replaced where it stands, or added at the end."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    old = open(path).read() if os.path.exists(path) else ""
    start = old.find(header)
    if start < 0:
        new = old + ("" if not old or old.endswith("\n\n") else "\n") + header + text
    else:
        end = old.find("\n== ", start + len(header))
        new = old[:start] + header + text + (old[end + 1:] if end >= 0 else "")
    with open(path, "w") as f:
        f.write(new)


if __name__ == "__main__":
    main()
