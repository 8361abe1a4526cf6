#!/usr/bin/env python3
"""Writes tests/golden/morph.glb: a small scene with morph targets, made for the loader / morph / animation tests (no such fixture exists
in the reference, whose loader skips morph targets).

  mesh "sheet"  a 9 x 9 grid in the xy plane facing +z, three targets: 0 a dense POSITION bulge; 1 a POSITION ripple of a few vertices stored
                through a sparse accessor over zeros; 2 POSITION + NORMAL + TANGENT deltas, its NORMAL stored sparse over a bufferView.
                mesh.weights are non-zero.  The dense twins of the two sparse accessors are in the file as accessors nothing uses; the mesh's
                `extras` name them (sparse accessor -> dense accessor).
  nodes         "left" and "right" both show the sheet; "right" carries node.weights of its own.
  mesh "strip"  a 3 x 9 strip along +y with one target and a two-joint skin whose rest pose is sheared (translations only, so that both
                hosts compute the same joint matrices to the bit); node "strip" shows it.
  clip "morph"  a LINEAR weights channel on "left", a STEP one on "right", a CUBICSPLINE one on "strip".
  a point light and a camera.  Every translation is a dyadic rational: the transforms are exact in both hosts."""
import json
import os
import struct

import numpy as np

GRID = 9
MESH_WEIGHTS = [0.5, 0.25, 0.0]
RIGHT_WEIGHTS = [0.0, 1.0, 0.75]
STRIP_WEIGHTS = [0.5]
LINEAR_TIMES, LINEAR_KEYS = [0.0, 0.5, 1.0], [[0.0, 0.0, 0.0], [1.0, 0.5, 0.0], [0.25, 0.0, 1.0]]
STEP_TIMES, STEP_KEYS = [0.0, 0.25, 0.75], [[0.0, 1.0, 0.75], [1.0, 0.0, 0.0], [0.0, 0.0, 1.5]]
# CUBICSPLINE: (in-tangent, value, out-tangent) per key
CUBIC_TIMES, CUBIC_KEYS = [0.0, 0.5, 1.0], [[[0.0], [0.0], [2.0]], [[-1.0], [1.0], [1.0]], [[0.5], [-0.5], [0.0]]]


def sheet():
    pos, nrm, tan, uv, idx = [], [], [], [], []
    for y in range(GRID):
        for x in range(GRID):
            u, v = x / (GRID - 1), y / (GRID - 1)
            pos.append((u - 0.5, v - 0.5, 0.0)); nrm.append((0.0, 0.0, 1.0)); tan.append((1.0, 0.0, 0.0, 1.0)); uv.append((u, v))
    for y in range(GRID - 1):
        for x in range(GRID - 1):
            a = y * GRID + x
            idx += [a, a + 1, a + GRID, a + 1, a + GRID + 1, a + GRID]
    p = np.array(pos, np.float32)
    r2 = p[:, 0] ** 2 + p[:, 1] ** 2
    t0 = np.zeros_like(p); t0[:, 2] = 0.5 * np.exp(-6.0 * r2)                                   # bulge
    t1 = np.zeros_like(p)                                                                     # ripple: every seventh vertex
    t1_idx = np.arange(3, GRID * GRID, 7, dtype=np.uint32)
    t1[t1_idx] = np.stack([0.0625 * np.cos(t1_idx), 0.0625 * np.sin(t1_idx), 0.125 + 0.0 * t1_idx], axis=1)
    t2 = np.zeros_like(p); t2[:, 2] = 0.25 * np.sin(4.0 * p[:, 0])                               # wave along x ...
    t2n = np.zeros_like(p); t2n[:, 0] = -np.cos(4.0 * p[:, 0])                                   # ... with its normal tilt
    t2n_idx = np.arange(0, GRID * GRID, 2, dtype=np.uint32)
    t2n_base = t2n.copy(); t2n_base[t2n_idx] = 0.0                                              # the bufferView holds the odd vertices only
    t2t = np.zeros_like(p); t2t[:, 2] = np.cos(4.0 * p[:, 0])
    return dict(pos=p, nrm=nrm, tan=tan, uv=uv, idx=idx, t0=t0, t1=t1.astype(np.float32), t1_idx=t1_idx, t2=t2, t2n=t2n.astype(np.float32),
                t2n_idx=t2n_idx, t2n_base=t2n_base.astype(np.float32), t2t=t2t.astype(np.float32))


def strip():
    pos, nrm, uv, joints, weights, idx = [], [], [], [], [], []
    nx, ny = 3, 9
    for y in range(ny):
        f = y / (ny - 1)
        for x in range(nx):
            pos.append(((x - 1) * 0.25, 2.0 * f - 1.0, 0.0)); nrm.append((0.0, 0.0, 1.0)); uv.append((x / (nx - 1), f))
            joints.append((0, 1, 0, 0)); weights.append((1.0 - f, f, 0.0, 0.0))
    for y in range(ny - 1):
        for x in range(nx - 1):
            a = y * nx + x
            idx += [a, a + 1, a + nx, a + 1, a + nx + 1, a + nx]
    p = np.array(pos, np.float32)
    t = np.zeros_like(p); t[:, 2] = 0.5 * (1.0 - p[:, 1] ** 2); t[:, 0] = 0.25 * p[:, 0]
    ibm = [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1.0, 0, 1], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, -1.0, 0, 1]]     # column-major translate(0, -y, 0)
    return dict(pos=p, nrm=nrm, uv=uv, joints=joints, weights=weights, idx=idx, t=t.astype(np.float32), ibm=ibm)


def build(path=None):
    blobs, views, accessors = [], [], []

    def view(arr, dtype, target=None):
        raw = np.asarray(arr, dtype=dtype).tobytes()
        off = sum(len(b) for b in blobs)
        blobs.append(raw + b"\0" * ((-len(raw)) % 4))
        v = {"buffer": 0, "byteOffset": off, "byteLength": len(raw)}
        if target:
            v["target"] = target
        views.append(v)
        return len(views) - 1

    def add(arr, dtype, atype, target=None, minmax=False):
        a = np.asarray(arr, dtype=dtype)
        comp = {np.dtype("<f4"): 5126, np.dtype("<u2"): 5123, np.dtype("u1"): 5121, np.dtype("<u4"): 5125}[a.dtype]
        acc = {"bufferView": view(a, dtype, target), "componentType": comp, "count": len(a) if a.ndim > 1 else a.size, "type": atype}
        if minmax:
            acc["min"], acc["max"] = a.min(axis=0).tolist(), a.max(axis=0).tolist()
        accessors.append(acc)
        return len(accessors) - 1

    def add_sparse(count, indices, values, base=None):
        acc = {"componentType": 5126, "count": count, "type": "VEC3",
               "sparse": {"count": len(indices), "indices": {"bufferView": view(indices, "<u2"), "componentType": 5123},
                          "values": {"bufferView": view(values, "<f4")}}}
        if base is not None:
            acc["bufferView"] = view(base, "<f4", 34962)
        accessors.append(acc)
        return len(accessors) - 1

    s, b = sheet(), strip()
    n = GRID * GRID
    a_pos, a_nrm, a_tan = add(s["pos"], "<f4", "VEC3", 34962, True), add(s["nrm"], "<f4", "VEC3", 34962), add(s["tan"], "<f4", "VEC4", 34962)
    a_uv, a_idx = add(s["uv"], "<f4", "VEC2", 34962), add(s["idx"], "<u2", "SCALAR", 34963)
    a_t0 = add(s["t0"], "<f4", "VEC3", 34962)
    a_t1 = add_sparse(n, s["t1_idx"], s["t1"][s["t1_idx"]])
    a_t1_dense = add(s["t1"], "<f4", "VEC3")
    a_t2 = add(s["t2"], "<f4", "VEC3", 34962)
    a_t2n = add_sparse(n, s["t2n_idx"], s["t2n"][s["t2n_idx"]], s["t2n_base"])
    a_t2n_dense = add(s["t2n"], "<f4", "VEC3")
    a_t2t = add(s["t2t"], "<f4", "VEC3", 34962)
    b_pos, b_nrm, b_uv = add(b["pos"], "<f4", "VEC3", 34962, True), add(b["nrm"], "<f4", "VEC3", 34962), add(b["uv"], "<f4", "VEC2", 34962)
    b_jnt, b_wgt, b_idx = add(b["joints"], "u1", "VEC4", 34962), add(b["weights"], "<f4", "VEC4", 34962), add(b["idx"], "<u2", "SCALAR", 34963)
    b_t, b_ibm = add(b["t"], "<f4", "VEC3", 34962), add(b["ibm"], "<f4", "MAT4")
    lin_t, lin_v = add(LINEAR_TIMES, "<f4", "SCALAR"), add(np.array(LINEAR_KEYS).reshape(-1), "<f4", "SCALAR")
    stp_t, stp_v = add(STEP_TIMES, "<f4", "SCALAR"), add(np.array(STEP_KEYS).reshape(-1), "<f4", "SCALAR")
    cub_t, cub_v = add(CUBIC_TIMES, "<f4", "SCALAR"), add(np.array(CUBIC_KEYS).reshape(-1), "<f4", "SCALAR")

    doc = {
        "asset": {"version": "2.0", "generator": "tools/make_morph_glb.py"},
        "extensionsUsed": ["KHR_lights_punctual"],
        "extensions": {"KHR_lights_punctual": {"lights": [{"type": "point", "color": [1.0, 0.95, 0.9], "intensity": 300.0}]}},
        "scene": 0,
        "scenes": [{"nodes": [0, 1, 2, 3, 6, 7]}],
        "nodes": [
            {"name": "left", "mesh": 0, "translation": [-1.25, 0.0, 0.0]},
            {"name": "right", "mesh": 0, "translation": [1.25, 0.0, 0.0], "weights": RIGHT_WEIGHTS},
            {"name": "strip", "mesh": 1, "skin": 0},
            {"name": "skeleton", "children": [4]},
            {"name": "joint0", "translation": [0.0, -1.0, 0.0], "children": [5]},
            {"name": "joint1", "translation": [0.25, 2.0, 0.125]},
            {"name": "lamp", "translation": [0.5, 2.0, 3.0], "extensions": {"KHR_lights_punctual": {"light": 0}}},
            {"name": "camera", "camera": 0, "translation": [0.0, 0.0, 4.0]},
        ],
        "cameras": [{"type": "perspective", "perspective": {"yfov": 0.7, "znear": 0.1, "zfar": 100.0, "aspectRatio": 1.5}}],
        "skins": [{"joints": [4, 5], "skeleton": 3, "inverseBindMatrices": b_ibm}],
        "materials": [
            {"name": "sheet", "pbrMetallicRoughness": {"baseColorFactor": [0.3, 0.6, 0.8, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5}, "doubleSided": True},
            {"name": "strip", "pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.4, 0.2, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.7}, "doubleSided": True},
        ],
        "meshes": [
            {"name": "sheet", "weights": MESH_WEIGHTS, "extras": {"dense_twins": {str(a_t1): a_t1_dense, str(a_t2n): a_t2n_dense}},
             "primitives": [{"attributes": {"POSITION": a_pos, "NORMAL": a_nrm, "TANGENT": a_tan, "TEXCOORD_0": a_uv}, "indices": a_idx, "material": 0,
                             "targets": [{"POSITION": a_t0}, {"POSITION": a_t1}, {"POSITION": a_t2, "NORMAL": a_t2n, "TANGENT": a_t2t}]}]},
            {"name": "strip", "weights": STRIP_WEIGHTS,
             "primitives": [{"attributes": {"POSITION": b_pos, "NORMAL": b_nrm, "TEXCOORD_0": b_uv, "JOINTS_0": b_jnt, "WEIGHTS_0": b_wgt}, "indices": b_idx,
                             "material": 1, "targets": [{"POSITION": b_t}]}]},
        ],
        "animations": [{"name": "morph",
                        "samplers": [{"input": lin_t, "output": lin_v, "interpolation": "LINEAR"}, {"input": stp_t, "output": stp_v, "interpolation": "STEP"},
                                     {"input": cub_t, "output": cub_v, "interpolation": "CUBICSPLINE"}],
                        "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}, {"sampler": 1, "target": {"node": 1, "path": "weights"}},
                                     {"sampler": 2, "target": {"node": 2, "path": "weights"}}]}],
        "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": sum(len(x) for x in blobs)}],
    }
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    binary = b"".join(blobs)
    total = 12 + 8 + len(js) + 8 + len(binary)
    out = struct.pack("<III", 0x46546C67, 2, total) + struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(binary), 0x004E4942) + binary
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "morph.glb")
    with open(path, "wb") as f:
        f.write(out)
    print("wrote", os.path.normpath(path), len(out), "bytes")


if __name__ == "__main__":
    build()
