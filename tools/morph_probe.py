#!/usr/bin/env python3
"""Time of k_morph (tauray_amd/csrc/morph.h, bvh_build.hip) on the GPU next to k_skinning on the same mesh: a 1000 x 1000 grid (1 M vertices,
2 M triangles) with 64 morph targets (position, normal and tangent planes: 2.3 GB) of which 8 have a non-zero weight, and a two-joint skin.

  * `trhip_scene_morph` and `trhip_scene_skin` alone: host wall time of one call (both synchronise the device before and after their kernel)
    in a process that keeps no per-triangle vertex records (TRHIP_NO_SHADE_TRIS=1), so that a call is its kernel, the copy of its small
    list and the two synchronisations; next to it a device-to-device copy of as many bytes as k_morph moves, timed the same way (the floor
    of such a call), and the bytes over 8 TB/s, the HBM rate the round-6 roofline is read against.
  * one frame of such a mesh in a process with the records: morph + skin + refit, each step and the sum.

    python tools/morph_probe.py [--out profiles/r18/morph.txt] [--calls 20]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, TARGETS, ACTIVE, HBM_BYTES_PER_S = 1000, 64, 8, 8e12


def scene():
    from tauray_amd import scene as S
    u, v = np.meshgrid(np.linspace(-1, 1, N, dtype=np.float32), np.linspace(-1, 1, N, dtype=np.float32))
    vert = np.zeros(N * N, dtype=S.VERTEX)
    vert["pos"] = np.stack([u.reshape(-1), v.reshape(-1), np.zeros(N * N, np.float32)], axis=1)
    vert["normal"], vert["tangent"] = (0, 0, 1), (1, 0, 0, 1)
    vert["uv"] = vert["pos"][:, :2] * 0.5 + 0.5
    a = (np.arange(N - 1, dtype=np.uint32)[:, None] * N + np.arange(N - 1, dtype=np.uint32)[None]).reshape(-1)
    idx = np.stack([a, a + 1, a + N, a + 1, a + N + 1, a + N], axis=1).reshape(-1)
    cam = S.Camera(transform=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0], [0, 0, 0, 1.0]]), fov=40.0)
    mat = S.make_material(albedo=(0.6, 0.6, 0.6, 1), metallic=0.0, roughness=0.6, double_sided=True)
    sc = S.SceneDesc(instances=S.make_instance(np.eye(4), mat), spans=np.array([(0, N * N, 0, len(idx) // 3)], dtype=S.MESH_SPAN), vertices=vert, indices=idx,
                     point_lights=S.make_point_light(np.array([20.0, 20.0, 20.0]), (0.5, 2.0, 3.0), 0.0), cameras=[cam])
    skins = np.zeros(N * N, dtype=S.SKIN)
    skins["joints"][:, 1] = 1
    skins["weights"][:, 1] = vert["uv"][:, 1]
    skins["weights"][:, 0] = np.float32(1) - skins["weights"][:, 1]
    return sc.finalize(True), skins


def measure(calls):
    from tauray_amd import _lib
    from tauray_amd import renderer as R
    records = "TRHIP_NO_SHADE_TRIS" not in os.environ
    ctx = R.Context(0)
    sc, skins = scene()
    ss = R.SceneStage(ctx, sc)
    rng = np.random.default_rng(1)
    planes = [rng.random((TARGETS, N * N, 3), dtype=np.float32) * np.float32(0.01) for _ in range(3)]
    ss.set_skin(0, skins)
    ss.set_morph_targets(0, *planes)
    del planes
    joints = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    joints[1, :3, 3] = (0.1, 0.0, 0.2)

    def weights(k):
        w = np.zeros(TARGETS, np.float32)
        w[(np.arange(ACTIVE) * 7 + k) % TARGETS] = 0.5 + 0.01 * k
        return w

    def timed(fn):
        out = []
        for k in range(calls + 3):
            ctx.sync()
            t0 = time.perf_counter()
            fn(k)
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out[3:])), float(min(out[3:]))
    lines = []
    vb = N * N * 48
    moved = 2 * vb + ACTIVE * 3 * N * N * 12
    if not records:
        morph = timed(lambda k: ss.morph(0, weights(k), refit=None))
        skin = timed(lambda k: ss.skin(0, joints, refit=None))
        src, dst = ctx.alloc(moved // 2).zero(), ctx.alloc(moved // 2).zero()
        L = _lib.lib()
        copy = timed(lambda k: _lib.check(L.trhip_copy_peer(ctx.h, dst.data_ptr(), ctx.h, src.data_ptr(), moved // 2, None)))
        floor = moved / HBM_BYTES_PER_S * 1e3
        lines += [f"device: {ctx.info()}",
                  f"mesh: {N * N} vertices, {len(sc.indices) // 3} triangles, {TARGETS} targets x 3 planes ({TARGETS * 3 * N * N * 12 / 2**30:.2f} GiB), {ACTIVE} active; {calls} calls, 3 warm-up",
                  "without per-triangle vertex records (a call = kernel + copy of its list + two synchronisations), wall ms per call, median (min):",
                  f"  trhip_scene_morph (k_morph)   {morph[0]:.4f} ({morph[1]:.4f})   moves {moved / 1e6:.0f} MB: base {vb / 1e6:.0f} + {ACTIVE} x 3 planes {ACTIVE * 3 * N * N * 12 / 1e6:.0f} + destination {vb / 1e6:.0f}",
                  f"  trhip_scene_skin (k_skinning) {skin[0]:.4f} ({skin[1]:.4f})   moves {(2 * vb + N * N * 32) / 1e6:.0f} MB: source + skins + destination",
                  f"  device-to-device copy of {moved // 2 / 1e6:.0f} MB (reads and writes {moved / 1e6:.0f} MB) {copy[0]:.4f} ({copy[1]:.4f})",
                  f"  {moved / 1e6:.0f} MB at 8 TB/s: {floor:.4f} ms; k_morph call / that: {morph[0] / floor:.2f}; k_morph call / copy call: {morph[0] / copy[0]:.2f}; "
                  f"k_morph call - copy call + copy's bytes at 8 TB/s would be {max(morph[0] - copy[0], 0) + floor:.4f} ms", ""]
    else:
        steps = {"morph": [], "skin": [], "refit": [], "frame": []}
        for k in range(calls + 3):
            ctx.sync()
            t = [time.perf_counter()]
            ss.morph(0, weights(k), refit=None); t.append(time.perf_counter())
            ss.skin(0, joints, refit=None); t.append(time.perf_counter())
            ss._accel_after_change(True); ctx.sync(); t.append(time.perf_counter())
            if k >= 3:
                for name, d in zip(("morph", "skin", "refit"), np.diff(t)):
                    steps[name].append(d * 1e3)
                steps["frame"].append((t[-1] - t[0]) * 1e3)
        lines += ["one frame of the mesh with the records (the skin rebuilds them; the morph of a skinned mesh writes the skin's source only), wall ms, median (min):"]
        lines += [f"  {name:6s} {np.median(v):.4f} ({min(v):.4f})" for name, v in steps.items()] + [""]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "morph.txt"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.stdout.write(measure(args.calls))
        return
    text = ""
    for env in ({"TRHIP_NO_SHADE_TRIS": "1"}, {}):      # a fresh process each: the library reads the variable at upload
        e = {k: v for k, v in os.environ.items() if k != "TRHIP_NO_SHADE_TRIS"}
        e.update(env)
        text += subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"--calls={args.calls}"], env=e, check=True, capture_output=True, text=True, timeout=400).stdout
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== tools/morph_probe.py\n" + text)


if __name__ == "__main__":
    main()
