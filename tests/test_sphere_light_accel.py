"""Sphere lights through a light tree (trhip_scene_set_light_accel): the lights with radius != 0 get a 4-wide tree of their own, walked
after the triangles.  The loop over every light stays the definition (the oracle's, oracle/oracle.cc): hits must equal it bit for bit in
every mode and under every acceleration-structure strategy, also where the fp32 sphere test reports hits well outside the sphere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, LOOP, TREE = 0, 1, 2
STRATEGIES = (0, 1, 2)
NAMES = ("trhip_scene_set_light_accel", "trhip_scene_get_light_accel", "trhip_pt_get_light_counters")


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_entry_points_declared_exported_and_bound(tmp_path):
    from tauray_amd import _lib, renderer
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    for m, v in (("TRHIP_LIGHT_ACCEL_AUTO", 0), ("TRHIP_LIGHT_ACCEL_LOOP", 1), ("TRHIP_LIGHT_ACCEL_TREE", 2)):
        assert re.search(r"#define %s %d\b" % (m, v), header), m
    assert (_lib.LIGHT_ACCEL_AUTO, _lib.LIGHT_ACCEL_LOOP, _lib.LIGHT_ACCEL_TREE) == (0, 1, 2)
    src = tmp_path / "sz.c"
    src.write_text('#include "trhip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(trhip_light_accel_info), offsetof(trhip_light_accel_info, tree_bytes), offsetof(trhip_light_accel_info, last_was_refit), '
                   'sizeof(trhip_light_counters), sizeof(trhip_counters)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_bytes, off_refit, counters, old = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_lib.LightAccelInfoC) == 40
    assert off_bytes == _lib.LightAccelInfoC.tree_bytes.offset and off_refit == _lib.LightAccelInfoC.last_was_refit.offset
    assert counters == C.sizeof(_lib.LightCountersC) == 24
    assert old == C.sizeof(_lib.CountersC) == 56          # trhip_counters is unchanged
    for cls, attr in ((renderer.SceneStage, "set_light_accel"), (renderer.SceneStage, "light_accel"), (renderer.SceneStage, "update_lights"),
                      (renderer.PathTracerStage, "light_counters")):
        assert callable(getattr(cls, attr)), attr
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tauray_amd", "libtrhip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"{name} is not exported"


def test_sponza_lights_is_deterministic_with_its_light_classes():
    from tauray_amd import scenes
    a, b = scenes.sponza_lights(256, seed=3, width=64, height=36), scenes.sponza_lights(256, seed=3, width=64, height=36)
    assert scenes.scene_hash(a) == scenes.scene_hash(b)
    assert scenes.scene_hash(a) != scenes.scene_hash(scenes.sponza_lights(256, seed=4, width=64, height=36))
    base = scenes.sponza_class(3, 260_000, 0, 64, 36)
    assert np.array_equal(a.vertices, base.vertices) and np.array_equal(a.instances, base.instances)
    pl = a.point_lights
    assert len(pl) == 256
    r, pos = pl["radius"], pl["pos"].astype(np.float64)
    assert 10 <= (r == 0).sum() <= 60                               # lights without a sphere
    nz = r[r > 0]
    assert nz.min() >= 1e-3 * 0.999 and nz.max() <= 0.2 * 1.001 and nz.min() < 5e-3 and nz.max() > 0.1
    spot = pl["spot_radius"] >= 0
    assert 40 <= spot.sum() <= 80 and not spot[:a.spotlight_base].any() and spot[a.spotlight_base:].all()
    far = np.linalg.norm(pos, axis=1) > 90
    assert far.sum() == 4 and (r[far] > 0).all() and (r[far] <= 1e-2).all()
    inside = ~far
    assert (np.abs(pos[inside, 0]) < 15).all() and (pos[inside, 1] > 0).all() and (pos[inside, 1] < 12).all() and (np.abs(pos[inside, 2]) < 7).all()
    assert len(scenes.sponza_lights(0, width=64, height=36).point_lights) == 0


def _lights_only(point_lights):
    from tauray_amd import scene as S
    cam = S.Camera(fov=50, aspect=1.0)
    return S.SceneDesc(instances=np.zeros(0, dtype=S.INSTANCE), spans=np.zeros(0, dtype=S.MESH_SPAN), vertices=np.zeros(0, dtype=S.VERTEX),
                       indices=np.zeros(0, np.uint32), point_lights=point_lights, cameras=[cam]).finalize(True)


def test_fp32_sphere_test_reports_hits_outside_the_box():
    """Why a light tree with boxes pos +- r would miss hits: a 1 cm light 100 units away is "hit" by rays passing centimetres outside it."""
    from oracle import binding as B
    from tauray_amd import scene as S
    p = np.array([61.3, -52.1, 58.9])
    p = p / np.linalg.norm(p) * 100.0
    osc = B.OracleScene(_lights_only(S.make_point_light((1, 1, 1), tuple(p), 0.01)))
    rng = np.random.default_rng(3)
    n = 100_000
    u = rng.normal(size=(n, 3))
    u -= (u @ p)[:, None] * p / (p @ p)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    off = rng.uniform(0.0, 0.08, n)
    org = np.array([0.3, -0.2, 0.1])
    d = p + u * off[:, None] - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.tile(org, (n, 1)), np.zeros((n, 1)), d, np.full((n, 1), np.inf)], 1).astype(np.float32)
    hit = osc.trace_closest(rays, include_lights=True)["primitive_id"] == 0
    # the ray's distance from the centre, and how far its closest point lies outside the box pos +- r
    o64, d64 = rays[:, :3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    t = ((p - o64) * d64).sum(1) / (d64 * d64).sum(1)
    closest = o64 + t[:, None] * d64
    outside_box = np.max(np.abs(closest - p), axis=1) - 0.01
    assert hit[outside_box < 0.005].mean() > 0.5
    assert (hit & (outside_box > 0.02)).sum() > 0, "no hit 2 cm outside the box"
    assert (hit & (outside_box > 0.05)).sum() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# on the GPU

@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


@pytest.fixture(scope="module")
def oracle():
    from oracle import binding
    return binding


@pytest.fixture(scope="module")
def glb(R):
    from tauray_amd.gltf import load_glb
    return load_glb(os.path.join(GOLDEN, "test.glb"), 64, 64)


@pytest.fixture(scope="module")
def glb_world(glb):
    """test.glb with its triangles pre-transformed and identity model matrices: the two-level strategies then trace the world ray itself
    and their triangle hits are bit-exact to the oracle (test_accel_strategies.py), so the light hits can be held against it too."""
    from test_accel_strategies import _identity_scene
    return _identity_scene(glb)


def _light_rig(L, seed, extent=3.0):
    """L point / spot lights around test.glb: radii log-uniform in [1e-3, 0.2], one in ten 0, groups of equal lights (same position and
    radius at spread-out indices) and up to four tiny lights 100 .. 1000 units away."""
    from tauray_amd import scene as S
    rng = np.random.default_rng([seed, L])
    out = []
    for k in range(L):
        pos = rng.uniform(-extent, extent, 3)
        radius = 0.0 if rng.uniform() < 0.1 else float(np.exp(rng.uniform(np.log(1e-3), np.log(0.2))))
        if k < min(4, L // 8):
            d = rng.normal(size=3)
            pos, radius = d / np.linalg.norm(d) * rng.uniform(100, 1000), float(np.exp(rng.uniform(np.log(1e-3), np.log(1e-2))))
        col = tuple(rng.uniform(1, 5, 3))
        out.append(S.make_spotlight(col, tuple(pos), tuple(rng.normal(size=3)), radius, 40.0, 2.0) if k % 5 == 4 else S.make_point_light(col, tuple(pos), radius))
    pl = np.concatenate(out)
    if L >= 7:
        for g in range(min(3, L // 7)):
            src = int(rng.integers(0, L))
            for dst in rng.choice(L, size=2, replace=False):
                pl["pos"][dst], pl["radius"][dst] = pl["pos"][src], max(float(pl["radius"][src]), 0.05)
            pl["radius"][src] = max(float(pl["radius"][src]), 0.05)
    return pl


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _ray_sets(pl, seed, extent=4.0):
    """{name: rays (n, 8)} aimed at the rig `pl`."""
    rng = np.random.default_rng(seed)
    pos, rad = pl["pos"].astype(np.float64), pl["radius"].astype(np.float64)
    cand = np.flatnonzero(rad > 0)
    if len(cand) == 0:
        cand = np.arange(len(pl))

    def pack(o, d, tmin, tmax):
        n = len(o)
        return np.concatenate([o, np.broadcast_to(np.asarray(tmin, np.float64).reshape(-1, 1), (n, 1)), d,
                               np.broadcast_to(np.asarray(tmax, np.float64).reshape(-1, 1), (n, 1))], 1).astype(np.float32)

    sets = {}
    n = 3000
    o = rng.uniform(-extent, extent, (n, 3))
    sets["uniform"] = pack(o, _unit(rng.normal(size=(n, 3))), np.where(rng.uniform(size=n) < 0.5, 0.0, 1e-4),
                           np.where(rng.uniform(size=n) < 0.8, np.inf, rng.uniform(0.5, 8, n)))
    j = rng.choice(cand, n)
    dist = np.exp(rng.uniform(np.log(0.1), np.log(1000.0), n))
    o = pos[j] + _unit(rng.normal(size=(n, 3))) * dist[:, None]
    sets["aimed"] = pack(o, _unit(pos[j] - o + rng.normal(size=(n, 3)) * rad[j, None] * 0.5), 0.0, np.inf)
    # tangent rays: aimed at pos + w (r + s delta D), w perpendicular to the view direction, delta in [1e-5, 1e-2], s = +-1
    j = rng.choice(cand, n)
    D = np.exp(rng.uniform(np.log(0.1), np.log(1000.0), n))
    o = pos[j] + _unit(rng.normal(size=(n, 3))) * D[:, None]
    v = _unit(pos[j] - o)
    w = rng.normal(size=(n, 3))
    w = _unit(w - (w * v).sum(1, keepdims=True) * v)
    delta = np.exp(rng.uniform(np.log(1e-5), np.log(1e-2), n)) * np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
    sets["tangent"] = pack(o, _unit(pos[j] + w * (rad[j] + delta * D)[:, None] - o), 0.0, np.inf)
    m = 1000
    j = rng.choice(cand, m)
    o = pos[j] + _unit(rng.normal(size=(m, 3))) * (rad[j] * rng.uniform(0, 0.9, m))[:, None]
    sets["inside"] = pack(o, _unit(rng.normal(size=(m, 3))), 0.0, np.inf)
    j = rng.choice(cand, m)
    D = rng.uniform(0.5, 50.0, m)
    o = pos[j] + _unit(rng.normal(size=(m, 3))) * D[:, None]
    sets["tmin_cut"] = pack(o, _unit(pos[j] - o), D + rad[j] * rng.uniform(-1.2, 1.2, m), np.inf)
    # equal lights: several records with one position and radius (the lowest index wins)
    key = np.concatenate([pl["pos"], pl["radius"][:, None]], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    dup = np.flatnonzero((cnt[inv.reshape(-1)] > 1) & (rad > 0))
    if len(dup):
        j = rng.choice(dup, m)
        o = pos[j] + _unit(rng.normal(size=(m, 3))) * rng.uniform(0.5, 20, m)[:, None]
        sets["equal_lights"] = pack(o, _unit(pos[j] - o + rng.normal(size=(m, 3)) * rad[j, None] * 0.5), 0.0, np.inf)
    return sets


def _check_hits(got, ref, what):
    bad = ((got["instance_id"] != ref["instance_id"]) | (got["primitive_id"] != ref["primitive_id"])
           | (got["t"].view(np.uint32) != ref["t"].view(np.uint32)))
    hit = ref["primitive_id"] >= 0
    bad |= hit & ((got["bary_u"].view(np.uint32) != ref["bary_u"].view(np.uint32)) | (got["bary_v"].view(np.uint32) != ref["bary_v"].view(np.uint32)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} hits differ, first {np.flatnonzero(bad)[:5]}"


def _queries_match(ss, osc, sets, what, expect_light_hits=True):
    light_hits = 0
    for name, rays in sets.items():
        seeds = np.random.default_rng(len(rays)).integers(0, 2**32, len(rays), dtype=np.uint64).astype(np.uint32)
        for sd in (None, seeds):
            ref = osc.trace_closest(rays, sd, include_lights=True)
            _check_hits(ss.trace_closest(rays, sd, include_lights=True), ref, f"{what} {name} seeds={sd is not None}")
            light_hits += int(((ref["instance_id"] < 0) & (ref["primitive_id"] >= 0)).sum())
    if expect_light_hits:
        assert light_hits > 0, f"{what}: the rays hit no light"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 7, 64, 1000, 4096])
def test_queries_match_the_oracle(R, ctx, oracle, glb_world, L):
    import copy
    sc = copy.copy(glb_world)
    sc.point_lights = _light_rig(L, 5)
    osc = oracle.OracleScene(sc)
    sets = _ray_sets(sc.point_lights, 11 + L)
    n_sphere = int((sc.point_lights["radius"] != 0).sum())
    for strategy in STRATEGIES:
        ss = R.SceneStage(ctx, sc, as_strategy=strategy)
        for mode in (TREE, AUTO):
            ss.set_light_accel(mode)
            info = ss.light_accel()
            tree = mode == TREE or n_sphere >= info["auto_threshold"]
            assert info["requested"] == mode and info["in_effect"] == (TREE if tree and n_sphere else LOOP), info
            if info["in_effect"] == TREE:
                assert info["tree_lights"] == n_sphere and info["node_count"] >= 1 and info["tree_bytes"] >= 16 + 128
            _queries_match(ss, osc, sets, f"L={L} strategy={strategy} mode={mode}")


@pytest.mark.gpu
def test_tree_equals_loop_under_instance_transforms(R, ctx, glb):
    """test.glb as it is (instance transforms: the two-level strategies trace object-space rays, whose triangle hits differ from the
    world-space ones by ulps): under every strategy the tree gives exactly the loop's hits."""
    import copy
    sc = copy.copy(glb)
    sc.point_lights = _light_rig(1000, 9)
    sets = _ray_sets(sc.point_lights, 19)
    for strategy in STRATEGIES:
        ss = R.SceneStage(ctx, sc, as_strategy=strategy)
        for name, rays in sets.items():
            ss.set_light_accel(LOOP)
            ref = ss.trace_closest(rays, include_lights=True)
            ss.set_light_accel(TREE)
            _check_hits(ss.trace_closest(rays, include_lights=True), ref, f"strategy {strategy} {name}")


def _tie_scene():
    """One big triangle in the plane z = 4 (det a power of two, so the triangle test returns t = 4 exactly for rays along +z from integer
    points of z = 0) and spheres of radius 1 at z = 5 above those points (hh = (10 - 2) / 2 = 4 exactly): the triangle must win."""
    from tauray_amd import scene as S
    v = np.zeros(3, dtype=S.VERTEX)
    v["pos"] = [(-64, -64, 4), (64, -64, 4), (0, 64, 4)]
    v["normal"] = (0, 0, -1)
    v["tangent"] = (1, 0, 0, 1)
    inst = S.make_instance(np.eye(4), S.make_material(albedo=(0.5, 0.5, 0.5, 1.0), metallic=0.0, roughness=0.5, double_sided=True))
    xy = [(x, y) for x in range(-8, 9, 2) for y in range(-8, 9, 2)]
    pl = np.concatenate([S.make_point_light((1, 1, 1), (x, y, 5.0), 1.0) for x, y in xy])
    cam = S.Camera(fov=50, aspect=1.0)
    sc = S.SceneDesc(instances=inst, spans=np.array([(0, 3, 0, 1)], dtype=S.MESH_SPAN), vertices=v, indices=np.arange(3, dtype=np.uint32),
                     point_lights=pl, cameras=[cam]).finalize(True)
    o = np.array([(x, y, 0.0) for x, y in xy])
    rays = np.concatenate([o, np.zeros((len(o), 1)), np.tile([0.0, 0.0, 1.0], (len(o), 1)), np.full((len(o), 1), np.inf)], 1).astype(np.float32)
    return sc, rays


@pytest.mark.gpu
def test_triangle_beats_a_light_at_the_same_t_and_light_only_scenes(R, ctx, oracle):
    sc, rays = _tie_scene()
    osc = oracle.OracleScene(sc)
    ref = osc.trace_closest(rays, include_lights=True)
    assert (ref["instance_id"] == 0).all() and (ref["t"] == 4.0).all()        # the triangle, at exactly the light's hh
    lights_only = _lights_only(_light_rig(1000, 8))
    osc2 = oracle.OracleScene(lights_only)
    sets = _ray_sets(lights_only.point_lights, 21)
    for strategy in STRATEGIES:
        ss = R.SceneStage(ctx, sc, as_strategy=strategy)
        ss.set_light_accel(TREE)
        assert ss.light_accel()["in_effect"] == TREE
        _check_hits(ss.trace_closest(rays, include_lights=True), ref, f"ties, strategy {strategy}")
        _queries_match(ss, osc, {"near_ties": _ray_sets(sc.point_lights, 3)["aimed"]}, f"tie scene, strategy {strategy}")
        so = R.SceneStage(ctx, lights_only, as_strategy=strategy)
        so.set_light_accel(TREE)
        _queries_match(so, osc2, sets, f"lights only, strategy {strategy}")


@pytest.mark.gpu
def test_moved_lights_are_found_after_refit_and_rebuild(R, ctx, oracle, glb_world):
    """trhip_scene_update_lights leaves a valid tree: moved lights (refit) and radii switched to or from 0 (rebuild) against an oracle built
    with the moved lights.  A stale tree misses the moved lights."""
    import copy
    sc = copy.copy(glb_world)
    sc.point_lights = _light_rig(1000, 6)
    rng = np.random.default_rng(17)
    for strategy in (0, 1):
        ss = R.SceneStage(ctx, sc, as_strategy=strategy)
        ss.set_light_accel(TREE)
        assert ss.light_accel()["last_was_refit"] == 0
        moved = sc.point_lights.copy()
        moved["pos"] += rng.uniform(-0.6, 0.6, moved["pos"].shape).astype(np.float32)
        ss.update_lights(moved)
        info = ss.light_accel()
        assert info["last_was_refit"] == 1 and info["in_effect"] == TREE, info
        sc2 = copy.copy(sc)
        sc2.point_lights = moved
        _queries_match(ss, oracle.OracleScene(sc2), _ray_sets(moved, 30 + strategy), f"moved, strategy {strategy}")
        again = moved.copy()
        again["pos"] += rng.uniform(-0.6, 0.6, again["pos"].shape).astype(np.float32)
        flip = rng.uniform(size=len(again)) < 0.15
        again["radius"][flip] = np.where(again["radius"][flip] == 0, 0.07, 0.0).astype(np.float32)
        ss.update_lights(again)
        info = ss.light_accel()
        assert info["last_was_refit"] == 0 and info["tree_lights"] == int((again["radius"] != 0).sum()), info
        sc3 = copy.copy(sc)
        sc3.point_lights = again
        _queries_match(ss, oracle.OracleScene(sc3), _ray_sets(again, 40 + strategy), f"moved + radii, strategy {strategy}")


def _frame(R, ctx, ss, scene, size, ieee=None, count=False, **kw):
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, **kw), DistributionParams(tuple(size), DISTRIBUTION_DUPLICATE, 0, 1, True))
    if ieee is not None:
        pt.set_shading_arithmetic(ieee)
    if count:
        pt.set_profiling(count_work=True)
        pt.reset_counters()
    color = ctx.alloc(size[0] * size[1] * 16).zero()
    pt.run(color)
    img = color.download((size[1], size[0], 4))
    c, lc = pt.counters(), pt.light_counters()
    assert c["stack_overflows"] == 0
    pt.close()
    return img, c, lc


@pytest.fixture(scope="module")
def lights1000():
    from tauray_amd import scenes
    return scenes.sponza_lights(1000, seed=2, width=160, height=90)


@pytest.mark.gpu
def test_tree_and_loop_frames_are_bit_identical(R, ctx, lights1000):
    sc = lights1000
    ss = R.SceneStage(ctx, sc)
    for ieee in (True, False):
        for hide in (0, 1):
            kw = dict(max_bounces=4, hide_lights=hide)
            ss.set_light_accel(LOOP)
            a = _frame(R, ctx, ss, sc, (160, 90), ieee=ieee, **kw)[0]
            ss.set_light_accel(TREE)
            b = _frame(R, ctx, ss, sc, (160, 90), ieee=ieee, **kw)[0]
            assert (a[..., :3] > 0).mean() > 0.5
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"ieee={ieee} hide_lights={hide}"


@pytest.mark.gpu
def test_tree_and_loop_frames_are_bit_identical_at_1080p(R, ctx):
    from tauray_amd import scenes
    sc = scenes.sponza_lights(1000, seed=1)
    ss = R.SceneStage(ctx, sc)
    ss.set_light_accel(LOOP)
    a = _frame(R, ctx, ss, sc, (1920, 1080), max_bounces=4)[0]
    ss.set_light_accel(TREE)
    b = _frame(R, ctx, ss, sc, (1920, 1080), max_bounces=4)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_light_counters(R, ctx):
    from tauray_amd import scenes
    sc = scenes.sponza_lights(4096, seed=2, width=128, height=72)
    n_sphere = int((sc.point_lights["radius"] != 0).sum())
    ss = R.SceneStage(ctx, sc)
    ss.set_light_accel(LOOP)
    _, c, lc = _frame(R, ctx, ss, sc, (128, 72), count=True, max_bounces=4, hide_lights=0)
    assert c["closest_rays"] > 0 and lc["node_visits"] == 0 and lc["walk_fallbacks"] == 0
    assert lc["sphere_tests"] == n_sphere * c["closest_rays"], (lc, c["closest_rays"], n_sphere)
    ss.set_light_accel(TREE)
    _, c2, lc2 = _frame(R, ctx, ss, sc, (128, 72), count=True, max_bounces=4, hide_lights=0)
    assert c2["closest_rays"] == c["closest_rays"]
    per_ray = lc2["sphere_tests"] / c2["closest_rays"]
    assert 0 < per_ray < 64, per_ray
    assert 0 < lc2["node_visits"] / c2["closest_rays"] < 256
    _, c3, lc3 = _frame(R, ctx, ss, sc, (128, 72), count=False, max_bounces=4, hide_lights=0)
    assert lc3 == {"sphere_tests": 0, "node_visits": 0, "walk_fallbacks": 0}        # nothing counted without count_work
    assert lc2["walk_fallbacks"] <= lc2["node_visits"] // 100


@pytest.mark.gpu
def test_light_accel_info(R, ctx, glb):
    import copy
    from tauray_amd import scene as S
    ss = R.SceneStage(ctx, glb)
    ss.set_light_accel(TREE)
    info = ss.light_accel()
    n = int((glb.point_lights["radius"] != 0).sum())
    assert info["sphere_lights"] == n
    if n:
        assert info["in_effect"] == TREE and info["tree_lights"] == n and info["node_count"] >= 1
    sc = copy.copy(glb)
    sc.point_lights = S.make_point_light((1, 1, 1), (0, 3, 0), 0.0)      # no sphere light: the loop (over nothing)
    ss2 = R.SceneStage(ctx, sc)
    ss2.set_light_accel(TREE)
    info = ss2.light_accel()
    assert info["in_effect"] == LOOP and info["tree_lights"] == 0 and info["tree_bytes"] == 0 and info["sphere_lights"] == 0
    ss2.set_light_accel(AUTO)
    thr = ss2.light_accel()["auto_threshold"]
    assert thr >= 1
    for L, expect in ((max(1, thr // 2), LOOP), (thr * 2 + 8, TREE)):
        sc.point_lights = _light_rig(L, 12, extent=2.0)
        sc.point_lights["radius"] = np.maximum(sc.point_lights["radius"], 0.01)
        ss3 = R.SceneStage(ctx, sc)
        ss3.set_light_accel(AUTO)
        info = ss3.light_accel()
        assert info["requested"] == AUTO and info["in_effect"] == expect, (L, info)
    ss3.set_light_accel(LOOP)
    assert ss3.light_accel()["in_effect"] == LOOP and ss3.light_accel()["tree_lights"] == 0


@pytest.mark.gpu
def test_environment_switch(R, glb):
    """TRHIP_LIGHT_ACCEL chooses the mode of a device on which none was set (any letter case); another value is an error, not AUTO."""
    import copy
    sc = copy.copy(glb)
    sc.point_lights = _light_rig(3, 4)
    sc.point_lights["radius"] = 0.05
    old = os.environ.get("TRHIP_LIGHT_ACCEL")
    try:
        ctx2 = R.Context(0)
        os.environ["TRHIP_LIGHT_ACCEL"] = "Tree"
        info = R.SceneStage(ctx2, sc).light_accel()
        assert info["requested"] == TREE and info["in_effect"] == TREE, info
        os.environ["TRHIP_LIGHT_ACCEL"] = "treee"
        with pytest.raises(R.TrhipError, match="TRHIP_LIGHT_ACCEL"):
            R.SceneStage(ctx2, sc)
    finally:
        if old is None:
            os.environ.pop("TRHIP_LIGHT_ACCEL", None)
        else:
            os.environ["TRHIP_LIGHT_ACCEL"] = old


@pytest.mark.gpu
def test_unchanged_lights_keep_the_tree(R, ctx, glb):
    """trhip_scene_update_lights with the records the device holds (what an animated scene sends every frame) touches no tree."""
    import copy
    sc = copy.copy(glb)
    sc.point_lights = _light_rig(64, 7)
    ss = R.SceneStage(ctx, sc)
    ss.set_light_accel(TREE)
    moved = sc.point_lights.copy()
    moved["pos"] += np.float32(0.01)
    ss.update_lights(moved)
    assert ss.light_accel()["last_was_refit"] == 1
    before = ss.light_accel()
    ss.update_lights(moved.copy())          # the same records again: no refit, no rebuild
    after = ss.light_accel()
    assert after["last_ms"] == before["last_ms"] and after["last_was_refit"] == 1 and after["in_effect"] == TREE
