"""Two-level acceleration structures (trhip_scene_set_accel_strategy): per-mesh BLASes shared by the instances of one span under a TLAS,
and the static instances merged into one world-space BLAS next to per-mesh BLASes for the dynamic ones.  The default structure
(all-merged) is what the rest of the suite tests; here the two-level ones are held against it and against the oracle."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, PER_MESH, STATIC_MERGED = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_entry_points_declared_exported_and_bound(tmp_path):
    from tauray_amd import _lib
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    for name in ("trhip_scene_set_accel_strategy", "trhip_scene_set_dynamic_instances", "trhip_scene_get_accel_layout"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    for m, v in (("TRHIP_AS_ALL_MERGED", 0), ("TRHIP_AS_PER_MESH", 1), ("TRHIP_AS_STATIC_MERGED_DYNAMIC_PER_MESH", 2)):
        assert re.search(r"#define %s %d\b" % (m, v), header), m
    assert (_lib.AS_ALL_MERGED, _lib.AS_PER_MESH, _lib.AS_STATIC_MERGED_DYNAMIC_PER_MESH) == (0, 1, 2)
    src = tmp_path / "sz.c"
    src.write_text('#include "trhip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu\\n", sizeof(trhip_accel_layout), '
                   'offsetof(trhip_accel_layout, node_bytes), sizeof(trhip_accel_info)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, info = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_lib.AccelLayoutC) == 40
    assert off == _lib.AccelLayoutC.node_bytes.offset
    assert info == C.sizeof(_lib.AccelInfoC) == 48
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tauray_amd", "libtrhip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        for name in ("trhip_scene_set_accel_strategy", "trhip_scene_set_dynamic_instances", "trhip_scene_get_accel_layout"):
            assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"{name} is not exported"


def _world_triangles(sc):
    from tauray_amd.scene import from_glm
    out = []
    for i in range(len(sc.instances)):
        sp = sc.spans[i]
        v = sc.vertices["pos"][sp["vertex_offset"]:sp["vertex_offset"] + sp["vertex_count"]].astype(np.float64)
        ix = sc.indices[sp["index_offset"]:sp["index_offset"] + 3 * sp["triangle_count"]]
        m = np.asarray(from_glm(sc.instances["model"][i]), dtype=np.float64)
        out.append(((np.c_[v, np.ones(len(v))] @ m.T)[:, :3])[ix])
    return np.concatenate(out)


def test_shared_teapot_scene_is_the_same_world():
    from tauray_amd import scenes
    a = scenes.sponza_teapots(width=64, height=36)
    b = scenes.sponza_teapots(width=64, height=36, share_teapot_mesh=True)
    assert scenes.scene_hash(scenes.sponza_teapots()) == "1487debe8d5aa1a3"      # the default scene is what it was
    assert len(a.instances) == len(b.instances)
    teapots = b.spans[-50:]
    assert len(np.unique(teapots)) == 1 and teapots[0]["triangle_count"] == 14280
    assert len(np.unique(a.spans[-50:])) == 50
    assert np.array_equal(a.instances, b.instances)
    assert np.array_equal(_world_triangles(a), _world_triangles(b))
    assert len(b.vertices) < len(a.vertices) and len(b.indices) < len(a.indices)


def test_cli_rejects_an_unknown_strategy():
    exe = os.path.join(ROOT, "tauray_amd", "tauray_hip")
    if not os.path.exists(exe):
        pytest.fail("tauray_amd/tauray_hip is not built (__graft_entry__.build())")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")      # nothing to open: the option is checked before any device is touched
    r = subprocess.run([exe, os.path.join(GOLDEN, "test.glb"), "--as-strategy=bogus", "--headless=/dev/null"], capture_output=True, text=True,
                       env=env, timeout=60)
    assert r.returncode != 0
    msg = r.stderr + r.stdout
    for v in ("all-merged", "per-material", "per-model", "static-merged-dynamic-per-model"):
        assert v in msg, msg


# ---------------------------------------------------------------------------------------------------------------------------------
# on the GPU

@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


def _dup(size):
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    return DistributionParams(tuple(size), DISTRIBUTION_DUPLICATE, 0, 1, True)


def _frame(R, ctx, ss, scene, size, frames=1, lanes=None, **kw):
    from test_gpu_parity import _render_hip
    if lanes is None:
        return _render_hip(R, ctx, ss, scene, size, frames=frames, **kw)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, **kw), _dup(size))
    pt.set_lanes(lanes)
    color = ctx.alloc(size[0] * size[1] * 16).zero()
    for _ in range(frames):
        pt.run(color)
    img = color.download((1, size[1], size[0], 4))
    assert pt.counters()["stack_overflows"] == 0
    pt.close()
    return img


def _rays(n, seed, lo=-1.9, hi=1.9, tmax=np.inf):
    rng = np.random.default_rng(seed)
    org = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t1 = np.full((n, 1), tmax, np.float32) if np.isinf(tmax) else rng.uniform(0.05, tmax, size=(n, 1)).astype(np.float32)
    rays = np.concatenate([org, np.full((n, 1), 1e-4, np.float32), d, t1], axis=1)
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    return rays, seeds


def _same_hits(a, b):
    hit = a["instance_id"] >= 0
    return (np.array_equal(a["instance_id"], b["instance_id"]) and np.array_equal(a["primitive_id"], b["primitive_id"])
            and np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32))
            and np.array_equal(a["bary_u"][hit].view(np.uint32), b["bary_u"][hit].view(np.uint32))
            and np.array_equal(a["bary_v"][hit].view(np.uint32), b["bary_v"][hit].view(np.uint32)))


def _identity_scene(sc):
    """The scene with every instance's triangles pre-transformed in numpy (one span per instance) and identity model matrices."""
    from tauray_amd import scene as S
    from tauray_amd.scene import from_glm
    verts, idx, spans, insts = [], [], [], sc.instances.copy()
    vo = io = 0
    for i in range(len(sc.instances)):
        sp = sc.spans[i]
        v = sc.vertices[sp["vertex_offset"]:sp["vertex_offset"] + sp["vertex_count"]].copy()
        m = np.asarray(from_glm(sc.instances["model"][i]), dtype=np.float32)
        p = v["pos"].astype(np.float32)
        w = np.empty_like(p)
        for r in range(3):      # (model * vec4(pos, 1)).xyz in the device's order
            w[:, r] = ((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3]
        w[w == 0] = 0.0          # -0.0 as +0.0
        v["pos"] = w
        verts.append(v)
        idx.append(sc.indices[sp["index_offset"]:sp["index_offset"] + 3 * sp["triangle_count"]])
        spans.append((vo, len(v), io, int(sp["triangle_count"])))
        vo += len(v); io += 3 * int(sp["triangle_count"])
        insts["model"][i] = np.asarray(S.make_instance(np.eye(4), S.make_material())["model"][0])
    out = copy.copy(sc)
    out.vertices, out.indices, out.instances = np.concatenate(verts), np.concatenate(idx).astype(np.uint32), insts
    out.spans = np.array(spans, dtype=S.MESH_SPAN)
    return out


@pytest.fixture(scope="module")
def glb(R):
    from tauray_amd.gltf import load_glb
    return load_glb(os.path.join(GOLDEN, "test.glb"), 128, 128)


def _many_instances(n=4096):
    """test_gpu_parity.test_many_instances_of_one_mesh's scene: n instances of one tetrahedron span."""
    from tauray_amd import scene as S
    rng = np.random.default_rng(9)
    tet = np.zeros(4, dtype=S.VERTEX)
    tet["pos"] = [(0, 0, 0.15), (0.14, 0, -0.07), (-0.07, 0.12, -0.07), (-0.07, -0.12, -0.07)]
    tet["normal"] = tet["pos"] / np.linalg.norm(tet["pos"], axis=1, keepdims=True)
    tet["tangent"] = (1, 0, 0, 1)
    idx = np.array([0, 1, 2, 0, 2, 3, 0, 3, 1, 1, 3, 2], dtype=np.uint32)
    insts = []
    for i in range(n):
        g = np.array([i % 16, (i // 16) % 16, i // 256], dtype=np.float64)
        t = S.trs_matrix((g - (7.5, 7.5, 7.5)) * 0.45 + rng.uniform(-0.05, 0.05, 3), rng.normal(size=4), rng.uniform(0.6, 1.4, 3))
        emis = (3.0, 2.0, 1.0) if i % 97 == 0 else (0, 0, 0)
        insts.append(S.make_instance(t, S.make_material(albedo=tuple(rng.uniform(0.2, 0.9, 3)) + (1.0,), metallic=float(i % 3 == 0),
                                                         roughness=float(rng.uniform(0.1, 1.0)), emission=emis, double_sided=True)))
    cam = S.Camera(fov=50, aspect=1.0)
    cam.transform = S.trs_matrix((0.3, 0.2, 9.0))
    return S.SceneDesc(instances=np.concatenate(insts), spans=np.array([(0, 4, 0, 4)] * n, dtype=S.MESH_SPAN), vertices=tet, indices=idx,
                       point_lights=S.make_point_light((300, 300, 300), (0, 6, 8), 0.3), cameras=[cam]).finalize(True)


@pytest.mark.gpu
def test_identity_instances_are_bit_exact(R, ctx, glb):
    """Identity model matrices: the ray in every instance is the world ray, the BLAS records are the world triangles - hits, shadow
    visibilities and a 4-bounce frame are the bits of the all-merged structure.  STATIC_MERGED without marks is one merged BLAS."""
    ident = _identity_scene(glb)
    rays, seeds = _rays(200_000, 21)
    srays, _ = _rays(100_000, 22, tmax=3.0)
    ref = R.SceneStage(ctx, ident)
    want = (ref.trace_closest(rays, seeds, include_lights=True), ref.trace_closest(rays, None), ref.trace_shadow(srays),
            _frame(R, ctx, ref, ident, (128, 128), max_bounces=4))
    assert (want[0]["instance_id"] >= 0).mean() > 0.5
    ss = R.SceneStage(ctx, ident, as_strategy=PER_MESH)
    lay = ss.layout()
    assert lay["strategy"] == PER_MESH and lay["blas_count"] == len(ident.instances) and lay["tlas_leaf_count"] == len(ident.instances)
    assert _same_hits(ss.trace_closest(rays, seeds, include_lights=True), want[0])
    assert _same_hits(ss.trace_closest(rays, None), want[1])
    assert np.array_equal(ss.trace_shadow(srays).view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(_frame(R, ctx, ss, ident, (128, 128), max_bounces=4), want[3])
    # STATIC_MERGED_DYNAMIC_PER_MESH without dynamic marks on test.glb as uploaded: the all-merged tree's records under one identity leaf
    a, b = R.SceneStage(ctx, glb), R.SceneStage(ctx, glb, as_strategy=STATIC_MERGED)
    assert b.layout()["blas_count"] == 1 and b.layout()["tlas_leaf_count"] == 1
    assert _same_hits(a.trace_closest(rays, seeds, include_lights=True), b.trace_closest(rays, seeds, include_lights=True))
    assert np.array_equal(a.trace_shadow(srays).view(np.uint32), b.trace_shadow(srays).view(np.uint32))
    assert np.array_equal(_frame(R, ctx, a, glb, (128, 128), max_bounces=4), _frame(R, ctx, b, glb, (128, 128), max_bounces=4))


def _agreement(a, b, origin_scale):
    """(instance, primitive) agreement of two hit arrays; every mismatch must be a near-tie."""
    ia = np.stack([a["instance_id"], a["primitive_id"]], 1)
    ib = np.stack([b["instance_id"], b["primitive_id"]], 1)
    same = (ia == ib).all(1)
    hit = same & (a["instance_id"] >= 0)
    # t error against the ray's scale: the object-space ray is the world ray rounded at the magnitude of its origin, so a hit at a small
    # distance from a far origin moves by ulps of the origin, not of t
    scale = np.maximum(np.abs(b["t"][hit]).astype(np.float64), origin_scale[hit])
    terr = np.abs(a["t"][hit].astype(np.float64) - b["t"][hit]) / np.maximum(scale, 1e-30)
    bad = ~same
    ta, tb = a["t"][bad].astype(np.float64), b["t"][bad].astype(np.float64)
    near_t = (np.abs(ta - tb) <= 1e-4 * np.maximum(np.abs(tb), 1e-30)) & (ta > 0) & (tb > 0)

    def edge(h):
        u, v = h["bary_u"].astype(np.float64), h["bary_v"].astype(np.float64)
        return (np.minimum(np.minimum(u, v), 1.0 - u - v) <= 1e-4) & (h["instance_id"] >= 0)
    near_edge = edge(a[bad]) | edge(b[bad])
    return float(same.mean()), terr, near_t | near_edge, int(bad.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["test.glb", "many_instances"])
def test_two_level_agrees_with_the_world_space_result(R, ctx, glb, which):
    """200 k random rays, transforms that are not the identity, half of the instances marked dynamic.  Measured on MI355X (both two-level
    strategies): test.glb - every (instance, primitive) and every shadow visibility equal, t error of max(t, |origin|) p99.9 5.8e-7, max
    4.9e-6; 4096 tetrahedra - 2 of 200 000 rays hit another triangle (near-ties), shadow visibility all equal, t error p99.9 1.9e-6, max
    6.9e-5 (grazing hits).  Bounds: >= 99.9 % agreement, near-ties only, t error p99.9 / max <= 1e-6 / 1e-5 (test.glb) and 4e-6 / 1.5e-4
    (tetrahedra).  The t error is taken against max(t, |origin|): the object-space ray is the world ray rounded at the magnitude of its
    origin, so a hit close to a far origin moves by ulps of the origin - relative to t alone test.glb's largest is 1.2e-3, at t ~ 1e-3."""
    sc = glb if which == "test.glb" else _many_instances()
    lo, hi = (-1.9, 1.9) if which == "test.glb" else (-4.0, 4.0)
    rays, seeds = _rays(200_000, 31, lo, hi)
    srays, _ = _rays(200_000, 32, lo, hi, tmax=3.0)
    ref = R.SceneStage(ctx, sc)
    want_c, want_n, want_s = ref.trace_closest(rays, seeds), ref.trace_closest(rays, None), ref.trace_shadow(srays)
    dynamic = np.zeros(len(sc.instances), np.uint8)
    dynamic[::2] = 1
    for strategy in (PER_MESH, STATIC_MERGED):
        ss = R.SceneStage(ctx, sc, as_strategy=strategy, dynamic=dynamic)
        for got, want in ((ss.trace_closest(rays, seeds), want_c), (ss.trace_closest(rays, None), want_n)):
            frac, terr, near, n_bad = _agreement(got, want, np.abs(rays[:, :3]).max(1).astype(np.float64))
            ties = bool(near.all())
            p999, tmax = float(np.quantile(terr, 0.999)), float(terr.max())
            print(f"{which} strategy {strategy}: agree {frac:.6f}, {n_bad} mismatches, t error of max(t, |origin|): p99.9 {p999:.3e}, max {tmax:.3e}")
            assert frac >= 0.999 and ties, f"strategy {strategy}: {frac:.5f} agree, {n_bad} mismatches, near-ties only: {ties}"
            # grazing hits turn the rounding of the object-space ray into a larger shift of t: the tail is bounded apart
            b999, bmax = (1e-6, 1e-5) if which == "test.glb" else (4e-6, 1.5e-4)
            assert p999 <= b999 and tmax <= bmax, f"strategy {strategy}: t error p99.9 {p999:.3e}, max {tmax:.3e}"
        vs = ss.trace_shadow(srays)
        agree = float(((vs == 0) == (want_s == 0)).mean())
        print(f"{which} strategy {strategy}: shadow visibility agrees for {agree:.6f}")
        assert agree >= 0.999


def _alpha_instances(n=24):
    """n instances of one 128-triangle grid, every third opaque (instance 0 - the instance a shared BLAS is built from - among them),
    every third with a constant alpha of its own, every third with an alpha texture: layers the rays cross, at random poses."""
    from tauray_amd import scene as S
    rng = np.random.default_rng(17)
    k = 8
    g = np.linspace(-0.5, 0.5, k + 1, dtype=np.float32)
    xx, yy = np.meshgrid(g, g)
    verts = np.zeros((k + 1) ** 2, dtype=S.VERTEX)
    verts["pos"] = np.stack([xx.ravel(), yy.ravel(), np.zeros(xx.size, np.float32)], 1)
    verts["normal"] = (0, 0, 1)
    verts["tangent"] = (1, 0, 0, 1)
    verts["uv"] = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], 1)
    idx = []
    for j in range(k):
        for i in range(k):
            a = j * (k + 1) + i
            idx += [a, a + 1, a + k + 2, a, a + k + 2, a + k + 1]
    tex = np.zeros((16, 16, 4), np.uint8)
    tex[..., :3] = 200
    tex[..., 3] = rng.integers(0, 256, size=(16, 16))
    insts = []
    for i in range(n):
        kind = i % 3
        if kind == 0:
            m = S.make_material(albedo=(0.8, 0.7, 0.6, 1.0), metallic=0.0, roughness=0.5, double_sided=True)
        elif kind == 1:
            m = S.make_material(albedo=(0.5, 0.8, 0.6, 0.3 + 0.02 * i), metallic=0.0, roughness=0.5, double_sided=True)
        else:
            m = S.make_material(albedo=(0.9, 0.9, 0.9, 0.9), metallic=0.0, roughness=0.5, albedo_tex=0, double_sided=True)
        t = S.trs_matrix((rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -1.0 + 0.09 * i), rng.normal(size=4), rng.uniform(0.8, 1.6, 3))
        insts.append(S.make_instance(t, m))
    cam = S.Camera(fov=50, aspect=1.0)
    cam.transform = S.trs_matrix((0.0, 0.0, 4.0))
    sc = S.SceneDesc(instances=np.concatenate(insts), spans=np.array([(0, len(verts), 0, 2 * k * k)] * n, dtype=S.MESH_SPAN), vertices=verts,
                     indices=np.array(idx, dtype=np.uint32), textures=[tex], cameras=[cam],
                     point_lights=S.make_point_light((30, 30, 30), (0, 2, 3), 0.2)).finalize(True)
    assert sc.potentially_transparent().tolist() == [i % 3 != 0 for i in range(n)]
    return sc


@pytest.mark.gpu
def test_alpha_per_instance_of_a_shared_mesh(R, ctx):
    """Instances of one mesh with different materials - opaque, a constant alpha, an alpha texture - share one BLAS: the instance id,
    the non-opaque bit and the any-hit record have to come from the TLAS leaf, not from the records (built from instance 0, which is
    opaque).  Seeded closest hits (stochastic alpha), fixed-cutoff hits and shadow visibility against all-merged, 200 k rays.  Measured
    on MI355X (per-mesh, seeded): 2 of 200 000 rays differ - a t near-tie (0.30105305 / 0.3010532) and one any-hit decision on an
    alpha-textured candidate that the rounded object-space ray saw on the other side of a texel; t error max 1.2e-5 of max(t, |origin|);
    occlusion equal for every shadow ray, |visibility difference| p99.9 1.0e-6 / max 1.0e-5 (products in another order, texels filtered at
    rounded coordinates).  Bounds: >= 99.9 % agreement, every mismatch a near-tie or an any-hit decision (<= 5), t error <= 2.5e-5,
    occlusion >= 99.9 %, visibility p99.9 <= 2e-6 and max <= 2e-5.  With the leaf's words taken from the BLAS's instance 0 instead, 35 %
    of the rays differ."""
    sc = _alpha_instances()
    rays, seeds = _rays(200_000, 51, -1.2, 1.2)
    srays, _ = _rays(200_000, 52, -1.2, 1.2, tmax=3.0)
    ref = R.SceneStage(ctx, sc)
    want_c, want_n, want_s = ref.trace_closest(rays, seeds), ref.trace_closest(rays, None), ref.trace_shadow(srays)
    kinds = np.where(want_c["instance_id"] >= 0, want_c["instance_id"] % 3, -1)
    assert (kinds == 1).sum() > 1000 and (kinds == 2).sum() > 1000 and (kinds == 0).sum() > 1000
    assert ((want_s > 0) & (want_s < 1)).sum() > 1000
    dynamic = (np.arange(len(sc.instances)) % 2).astype(np.uint8)
    for strategy in (PER_MESH, STATIC_MERGED):
        ss = R.SceneStage(ctx, sc, as_strategy=strategy, dynamic=dynamic)
        assert ss.layout()["blas_count"] == (1 if strategy == PER_MESH else 2)
        for got, want in ((ss.trace_closest(rays, seeds), want_c), (ss.trace_closest(rays, None), want_n)):
            frac, terr, near, n_bad = _agreement(got, want, np.abs(rays[:, :3]).max(1).astype(np.float64))
            ties = bool(near.all())
            tmax = float(terr.max()) if terr.size else 0.0
            bad = np.flatnonzero((got["instance_id"] != want["instance_id"]) | (got["primitive_id"] != want["primitive_id"]))
            # a mismatch that is not a near-tie of t or of an edge has to be an any-hit decision: the nearer of the two hits lies on
            # a non-opaque instance, whose candidate alpha (a texel, or the hash cutoff) went the other way for the rounded ray
            ga, wa = got[bad], want[bad]
            near_inst = np.where((ga["t"] < wa["t"]) & (ga["instance_id"] >= 0) | (wa["instance_id"] < 0), ga["instance_id"], wa["instance_id"])
            alpha_decided = (near_inst >= 0) & (near_inst % 3 != 0)
            print(f"alpha instances strategy {strategy}: agree {frac:.6f}, {n_bad} mismatches ({int(alpha_decided.sum())} on a non-opaque "
                  f"nearer hit), t error max {tmax:.3e}; mismatches: {list(zip(ga['instance_id'], ga['t'], wa['instance_id'], wa['t']))[:6]}")
            assert frac >= 0.999 and (near | alpha_decided).all(), f"strategy {strategy}: {frac:.5f} agree, {n_bad} mismatches"
            assert int(alpha_decided.sum()) <= 5, f"strategy {strategy}: {int(alpha_decided.sum())} any-hit decisions differ"
            assert tmax <= 2.5e-5, f"strategy {strategy}: t error {tmax:.3e}"
        vs = ss.trace_shadow(srays)
        dv = np.abs(vs.astype(np.float64) - want_s)
        occl = float(((vs == 0) == (want_s == 0)).mean())
        q = np.quantile(dv, [0.99, 0.999, 0.9999])
        print(f"alpha instances strategy {strategy}: occlusion equal for {occl:.6f}; |visibility difference| p99 {q[0]:.3e} p99.9 {q[1]:.3e} "
              f"p99.99 {q[2]:.3e} max {dv.max():.3e}")
        assert occl >= 0.999 and q[1] <= 2e-6 and dv.max() <= 2e-5, f"strategy {strategy}: occlusion {occl:.6f}, p99.9 {q[1]:.3e}, max {dv.max():.3e}"


def _edge_scenes():
    """The scenes at which a per-lane loop starts in an unusual state: no triangle at all, a root that is a leaf, a leaf that can never be
    hit next to one that can (test_gpu_parity.test_edge_scenes' scenes), and one non-opaque instance (the grid and alpha texture of
    _alpha_instances), at the identity so that the two-level structure promises the world-space bits."""
    from tauray_amd import scene as S
    cam = S.Camera(fov=60, aspect=1.0)
    cam.transform = S.trs_matrix((0, 0, 3))
    tri = np.zeros(3, dtype=S.VERTEX)
    tri["pos"] = [(-1, -1, 0), (1, -1, 0), (0, 1, 0)]
    tri["normal"] = (0, 0, 1)
    tri["tangent"] = (1, 0, 0, 1)
    mat = S.make_material(albedo=(0.8, 0.8, 0.8, 1), metallic=0.0, roughness=0.5, emission=(0.5, 0.2, 0.1))
    light = S.make_point_light((5, 5, 5), (0, 0, 2), 0.2)

    def scene_with(verts, idx, material=mat, **kw):
        n = len(idx) // 3
        inst = S.make_instance(np.eye(4), material) if n else np.zeros(0, dtype=S.INSTANCE)
        return S.SceneDesc(instances=inst, spans=np.array([(0, len(verts), 0, n)] if n else [], dtype=S.MESH_SPAN), vertices=verts,
                           indices=np.asarray(idx, dtype=np.uint32), point_lights=light, cameras=[cam], **kw).finalize(True)

    deg = np.zeros(6, dtype=S.VERTEX)
    deg[:3] = tri
    deg["pos"][3:] = (0.25, 0.25, 0.5)       # zero-area triangle in front of the real one
    deg["normal"][3:] = (0, 0, 1)
    grid = _alpha_instances(1)
    glass = S.make_material(albedo=(0.9, 0.9, 0.9, 0.9), metallic=0.0, roughness=0.5, albedo_tex=0, double_sided=True)
    alpha = scene_with(grid.vertices, grid.indices, glass, textures=grid.textures)
    assert alpha.potentially_transparent().tolist() == [True]
    return [("empty", scene_with(np.zeros(0, dtype=S.VERTEX), [])), ("single triangle", scene_with(tri, [0, 1, 2])),
            ("degenerate pair", scene_with(deg, [0, 1, 2, 3, 4, 5])), ("non-opaque instance", alpha)]


def _edge_rays():
    """256 rays around the unit square of the plane z = 0, where the edge scenes have their triangles: half of them aimed at it (most
    hit), half anywhere (most miss), the first four special."""
    rng = np.random.default_rng(77)
    n = 256
    org = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    org[:, 2] = rng.uniform(0.5, 3.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    target = np.concatenate([rng.uniform(-0.7, 0.7, size=(n, 2)), np.zeros((n, 1))], axis=1).astype(np.float32)
    d = np.where((np.arange(n) % 2 == 0)[:, None], target - org, rng.normal(size=(n, 3))).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], axis=1)
    rays[0, :3] = (np.nan, 0.0, 2.0)                                       # a NaN origin
    rays[1] = (0.0, -0.25, 2.0, 1e-4, 0.0, 0.0, 0.0, np.inf)               # a zero direction
    rays[2] = (0.04, -0.31, 2.0, 1e-4, 0.0, 0.0, -1.0, 1.0)                 # tmax shorter than the hit at t = 2 ...
    rays[3] = (0.04, -0.31, 2.0, 1e-4, 0.0, 0.0, -1.0, np.inf)              # ... and the same ray with room for it
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    return rays, seeds


@pytest.mark.gpu
def test_per_lane_loops_on_edge_scenes(R, ctx, oracle):
    """The per-lane loops of csrc/trace.h (one loop per query kind for both structure kinds) in the states their start can get wrong:
    the empty scene, a root that is a leaf, a degenerate leaf, a non-opaque instance - under the all-merged and the per-mesh
    structure.  Frames go through the wave loops of trace_quad.h; the ray queries and the feature stage are what runs these loops
    alone, so they are held against the oracle bit for bit (identity instances: the two-level structure traces the world ray)."""
    rays, seeds = _edge_rays()
    for what, sc in _edge_scenes():
        osc = oracle.OracleScene(sc)
        want_c, want_n, want_s = osc.trace_closest(rays, seeds), osc.trace_closest(rays, None), osc.trace_shadow(rays)
        want_f = {fid: osc.render_feature(fid, 16, 16) for fid in (5, 9)}
        # not vacuous (decided by the oracle alone): hits and misses in every scene but the empty one, the special rays do what they are for
        hit = want_n["instance_id"] >= 0
        assert not hit[:3].any(), f"{what}: a NaN origin, a zero direction and a short tmax hit nothing"
        if what == "empty":
            assert not hit.any() and (want_s == 1).all()
        else:
            assert hit[3] and hit.sum() >= 32 and (~hit).sum() >= 32, f"{what}: {hit.sum()} hits of {len(hit)}"
            assert (want_s == 0).any() or what == "non-opaque instance"
            assert np.isfinite(want_f[5][..., 0]).any() and np.isnan(want_f[5][..., 0]).any(), f"{what}: the 16 x 16 view wants hits and misses"
        if what == "non-opaque instance":
            assert ((want_s > 0) & (want_s < 1)).sum() >= 16 and not _same_hits(want_c, want_n), "the any-hit decisions have to matter"
        for strategy in (ALL, PER_MESH):
            ss = R.SceneStage(ctx, sc, as_strategy=strategy)
            assert _same_hits(ss.trace_closest(rays, seeds), want_c), f"{what}, strategy {strategy}: seeded closest hits"
            assert _same_hits(ss.trace_closest(rays, None), want_n), f"{what}, strategy {strategy}: closest hits"
            assert np.array_equal(ss.trace_shadow(rays).view(np.uint32), want_s.view(np.uint32)), f"{what}, strategy {strategy}: shadow rays"
            for fid in (5, 9):       # distance, instance id
                fs = R.FeatureStage(ctx, ss, fid, _dup((16, 16)))
                buf = ctx.alloc(16 * 16 * 16).zero()
                fs.run(buf)
                assert np.array_equal(buf.download((16, 16, 4)), want_f[fid], equal_nan=True), f"{what}, strategy {strategy}: feature {fid}"


@pytest.mark.gpu
def test_shape_independence_and_rigid_updates(R, ctx, glb):
    """Within a strategy, hits and frames do not depend on the tree: static build, fast build, update + refit, and a fresh build after
    the same update agree bit for bit - for rigid moves of dynamic instances (no BLAS touched), a moved static instance and a
    skinned instance."""
    from tauray_amd import _lib
    from tauray_amd.scene import SKIN
    rays, seeds = _rays(100_000, 41)
    n = len(glb.instances)
    dynamic = np.zeros(n, np.uint8)
    dynamic[[1, 3]] = 1
    static_inst = int(np.flatnonzero(dynamic == 0)[-1])
    moved = glb.instances.copy()
    for i in (1, 3):
        moved["model"][i][3][:3] += np.float32(0.0625) * (i + 1)
    moved_static = moved.copy()
    moved_static["model"][static_inst][3][:3] += np.float32(0.03125)

    def probe(ss, scene):
        return ss.trace_closest(rays, seeds, include_lights=True), _frame(R, ctx, ss, scene, (96, 96), max_bounces=3)

    def same(a, b):
        return _same_hits(a[0], b[0]) and np.array_equal(a[1], b[1])

    for strategy in (PER_MESH, STATIC_MERGED):
        a = R.SceneStage(ctx, glb, as_strategy=strategy, dynamic=dynamic)
        base = probe(a, glb)
        fast = R.SceneStage(ctx, glb, as_strategy=strategy, dynamic=dynamic)
        _lib.check(_lib.lib().trhip_scene_set_build_mode(fast.ctx.h, 1))
        info = _lib.AccelInfoC()
        _lib.check(_lib.lib().trhip_scene_build_accel(fast.ctx.h, C.byref(info)))
        assert same(probe(fast, glb), base), f"strategy {strategy}: fast build"
        for inst, touches in ((moved, 0), (moved_static, 1 if strategy == STATIC_MERGED else 0)):
            a.update_instances(inst, refit=True)
            lay = a.layout()
            assert lay["blas_updated"] == touches, f"strategy {strategy}: {lay}"
            sc2 = copy.copy(glb)
            sc2.instances = inst
            fresh = R.SceneStage(ctx, sc2, as_strategy=strategy, dynamic=dynamic)
            got, want = probe(a, sc2), probe(fresh, sc2)
            assert same(got, want), f"strategy {strategy}: refit after a move != fresh build"
            assert not _same_hits(got[0], base[0])
        # skinning: the BLAS of that mesh alone is refit
        inst = 1
        vc = int(glb.spans[inst]["vertex_count"])
        skins = np.zeros(vc, dtype=SKIN)
        skins["weights"][:, 0] = 1.0
        for ss in (a, fresh):
            ss.set_skin(inst, skins)
        bend = np.eye(4, dtype=np.float32)[None].repeat(1, 0)
        bend[0, :3, 3] = (0.05, 0.1, -0.05)
        a.skin(inst, bend, refit=True)
        assert a.layout()["blas_updated"] == 1
        fresh.skin(inst, bend, refit=False)
        assert same(probe(a, sc2), probe(fresh, sc2)), f"strategy {strategy}: skinned refit != rebuild"


@pytest.mark.gpu
def test_tri_lights_are_byte_equal_across_strategies(R, ctx):
    sc = _many_instances()
    got = [R.SceneStage(ctx, sc, as_strategy=s, dynamic=(np.arange(len(sc.instances)) % 3 == 0)).tri_lights() for s in (ALL, PER_MESH, STATIC_MERGED)]
    assert len(got[0]) == 4 * len(range(0, len(sc.instances), 97))
    for g in got[1:]:
        assert np.array_equal(g.view(np.uint8), got[0].view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [PER_MESH, STATIC_MERGED])
def test_two_level_frames_match_the_oracle(R, ctx, oracle, glb, strategy):
    """_compare (both shading arithmetics) against the oracle's frames, as test_many_instances_of_one_mesh does for all-merged; features
    9 (instance id), 5 (distance) and 1 (normal) against the oracle's.  Measured on MI355X: instance id equal for 99.994 % (per-mesh) /
    100 % of the 4096-instance pixels and for all of test.glb's; distance within 1e-4 on every pixel of the same instance."""
    from test_gpu_parity import _compare_both
    for sc, what in ((_many_instances(), "4096 instances"), (glb, "test.glb")):
        dyn = np.zeros(len(sc.instances), np.uint8)
        dyn[1::2] = 1
        ss = R.SceneStage(ctx, sc, as_strategy=strategy, dynamic=dyn)
        osc = oracle.OracleScene(sc)
        w, h = 128, 128
        ref = osc.render_pt(oracle.options_for_scene(sc, max_bounces=3), w, h)
        _compare_both(R, ctx, ss, sc, (w, h), ref, f"{what} strategy {strategy}", max_bounces=3)
        feats = {}
        for fid in (9, 5, 1):
            fs = R.FeatureStage(ctx, ss, fid, _dup((w, h)))
            buf = ctx.alloc(w * h * 16).zero()
            fs.run(buf)
            feats[fid] = (buf.download((h, w, 4)), osc.render_feature(fid, w, h))
        # the bounds of test_two_level_agrees_with_the_world_space_result: the instance hit by >= 99.9 % of the pixels' rays, the
        # distance and normal of those pixels within the rounding of the object-space ray
        same = (feats[9][0] == feats[9][1]).all(-1)
        print(f"{what} strategy {strategy}: instance id equal for {same.mean():.5f} of the pixels")
        assert same.mean() >= 0.999, f"{what} strategy {strategy}: feature 9 equal for {same.mean():.5f}"
        for fid in (5, 1):
            got, want = feats[fid]
            close = np.isclose(got, want, rtol=1e-4, atol=1e-5, equal_nan=True).all(-1)
            err = np.abs(got - want)[same].max()
            print(f"{what} strategy {strategy}: feature {fid} close for {close[same].mean():.5f} of the same-instance pixels, max error {err:.3e}")
            # distance within 1e-4 everywhere; the interpolated normal of a grazing hit moves with the hit point along the surface
            # (measured: 99.4 / 99.7 % of the 4096-instance pixels within 1e-4, largest error 1.2e-3; test.glb 99.94 %, largest 7.4e-5)
            if fid == 5:
                assert close[same].all(), f"{what} strategy {strategy}: feature {fid}"
            else:
                assert close[same].mean() >= 0.99 and err <= 5e-3, f"{what} strategy {strategy}: feature {fid}"


@pytest.mark.gpu
def test_memory_of_the_shared_teapot_scene(R, ctx):
    from tauray_amd import scenes
    sc = scenes.sponza_teapots(width=64, height=36, share_teapot_mesh=True)
    n = len(sc.instances)
    teapot = np.zeros(n, np.uint8)
    teapot[-50:] = 1
    a = R.SceneStage(ctx, sc)
    base = a.layout()
    assert base["strategy"] == ALL and base["blas_count"] == 1
    a_bytes = base["node_bytes"] + base["record_bytes"]
    del a
    for strategy, dyn, blases in ((PER_MESH, None, n - 49), (STATIC_MERGED, teapot, 2)):
        ss = R.SceneStage(ctx, sc, as_strategy=strategy, dynamic=dyn)
        lay = ss.layout()
        assert lay["blas_count"] == blases, lay
        ratio = (lay["node_bytes"] + lay["record_bytes"]) / a_bytes
        assert ratio <= 0.40, f"strategy {strategy}: {ratio:.3f} of all-merged's bytes"


@pytest.mark.gpu
def test_full_size_shared_teapots_static_merged(R, ctx):
    """1920 x 1080, 4 bounces, static instances merged, the teapots dynamic: no stack overflow, the same bits for 1 and 4 lanes and for 1
    and 2 frames in flight, and after
    64 accumulated frames unbiased against the all-merged structure's frame.  Measured on MI355X: RMS 1.88e-3 (mean radiance 0.193), mean
    radiance equal to 1.1e-6, 0.30 % of the pixels off by more than 1e-2 - paths that took another near-tie decision (the object-space ray
    of a teapot rounds differently) and then diverged; the RMS is theirs, which is why it is bounded at 2.5e-3 and not at 1e-3."""
    from tauray_amd import scenes
    size = (1920, 1080)
    sc = scenes.sponza_teapots(width=size[0], height=size[1], share_teapot_mesh=True)
    teapot = np.zeros(len(sc.instances), np.uint8)
    teapot[-50:] = 1
    ss = R.SceneStage(ctx, sc, as_strategy=STATIC_MERGED, dynamic=teapot)
    one = _frame(R, ctx, ss, sc, size, lanes=1, max_bounces=4)
    four = _frame(R, ctx, ss, sc, size, lanes=4, max_bounces=4)
    assert np.array_equal(one, four)
    # 1 and 2 frames in flight: frame i of the slotted renderer is frame i of the one-frame-at-a-time renderer
    opt = R.options_for_scene(sc, max_bounces=4)
    serial = R.RtRenderer(ctx, sc, opt, size, use_torch=False, as_strategy=STATIC_MERGED, dynamic=teapot)
    want = []
    for _ in range(3):
        serial.render()
        want.append(serial.download("color"))
    serial.close()
    slotted = R.RtRenderer(ctx, sc, opt, size, use_torch=False, frames_in_flight=2, as_strategy=STATIC_MERGED, dynamic=teapot)
    for _ in range(3):
        slotted.render()
    slotted.sync()
    for i in (1, 2):
        assert np.array_equal(slotted.slots[i % 2].color.download((1, size[1], size[0], 4)), want[i]), f"frame {i}"
    assert slotted.counters()["stack_overflows"] == 0
    slotted.close()
    acc = _frame(R, ctx, ss, sc, size, frames=64, max_bounces=4)
    ref = _frame(R, ctx, R.SceneStage(ctx, sc), sc, size, frames=64, max_bounces=4)
    rms = float(np.sqrt(np.mean((acc[..., :3] - ref[..., :3]) ** 2)))
    bias = abs(float(acc[..., :3].mean()) - float(ref[..., :3].mean())) / float(ref[..., :3].mean())
    rel = np.abs(acc[..., :3] - ref[..., :3]) / (np.abs(ref[..., :3]) + 1e-2)
    off = float((rel.max(-1) > 1e-2).mean())
    print(f"64 frames: rms {rms:.3e}, mean {float(ref[..., :3].mean()):.4f}, bias {bias:.3e}, pixels off by > 1e-2: {off:.4%}")
    assert bias <= 1e-4 and off <= 0.01 and rms <= 2.5e-3, (rms, bias, off)


@pytest.mark.gpu
def test_cpp_host_per_model_strategy(tmp_path):
    """`tauray_hip test.glb --as-strategy=per-model` writes the frame of the all-merged run within _compare's default bounds."""
    from test_gpu_parity import _compare
    exe = os.path.join(ROOT, "tauray_amd", "tauray_hip")
    W = H = 128
    imgs = {}
    for strategy in ("all-merged", "per-model", "static-merged-dynamic-per-model"):
        prefix = str(tmp_path / strategy)
        subprocess.check_call([exe, os.path.join(GOLDEN, "test.glb"), f"--width={W}", f"--height={H}", "--max-ray-depth=4", "--filetype=raw",
                               f"--as-strategy={strategy}", f"--headless={prefix}"], timeout=120)
        imgs[strategy] = np.fromfile(prefix + ".raw", dtype=np.float32).reshape(H, W, 4)
    assert imgs["all-merged"][..., :3].mean() > 0.01
    _compare(imgs["per-model"], imgs["all-merged"], "per-model vs all-merged")
    assert np.array_equal(imgs["static-merged-dynamic-per-model"], imgs["all-merged"])     # nothing is dynamic: one merged BLAS
