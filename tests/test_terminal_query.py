"""The last bounce as a first-hit emitter query (trhip_pt_set_terminal_query).  At bounce max_bounces - 1 a surface hit
can only add the emission of what was hit, so the ray needs one of three answers: it escapes, the nearest accepted hit is an emitter
triangle (with today's record), or something else is in the way (blocked).  The oracle's closest hit stays the definition: the query's class
must be the class of that hit, an emitter's record must equal it bit for bit, and frames must not depend on the mode at all."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, OFF = 0, 1
BLOCKED = -2
NAMES = ("trhip_pt_set_terminal_query", "trhip_pt_get_terminal_counters", "trhip_trace_terminal")


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_entry_points_declared_exported_and_bound(tmp_path):
    from tauray_amd import _lib, renderer
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    for m, v in (("TRHIP_TERMINAL_QUERY_AUTO", 0), ("TRHIP_TERMINAL_QUERY_OFF", 1)):
        assert re.search(r"#define %s %d\b" % (m, v), header), m
    assert (_lib.TERMINAL_QUERY_AUTO, _lib.TERMINAL_QUERY_OFF, _lib.HIT_BLOCKED) == (AUTO, OFF, BLOCKED)
    src = tmp_path / "sz.c"
    src.write_text('#include "trhip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(trhip_terminal_counters), offsetof(trhip_terminal_counters, in_effect), offsetof(trhip_terminal_counters, threshold), '
                   'sizeof(trhip_counters)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_effect, off_thr, old = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_lib.TerminalCountersC) == 32
    assert off_effect == _lib.TerminalCountersC.in_effect.offset and off_thr == _lib.TerminalCountersC.threshold.offset
    assert old == C.sizeof(_lib.CountersC) == 56          # trhip_counters is unchanged
    for cls, attr in ((renderer.SceneStage, "trace_terminal"), (renderer.PathTracerStage, "set_terminal_query"),
                      (renderer.PathTracerStage, "terminal_counters")):
        assert callable(getattr(cls, attr)), attr
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tauray_amd", "libtrhip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"{name} is not exported"


def _holes_texture(seed, size=32):
    """RGBA8 with alpha 0 / 255 in blobs and a colour gradient: an alpha-tested occluder, an emission texture."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / size
    img = np.zeros((size, size, 4), np.uint8)
    img[..., 0] = (255 * x).astype(np.uint8)
    img[..., 1] = (255 * y).astype(np.uint8)
    img[..., 2] = rng.integers(0, 256, (size, size), dtype=np.uint8)
    img[..., 3] = np.where(np.sin(x * 19.0) * np.cos(y * 23.0) > 0.2, 0, 255).astype(np.uint8)
    return img


def _rig(coplanar_emitter_first=True, emission=True, gather=True, extra_emitters=0, seed=1):
    """A room with clutter, a mirror and a glass panel, and the emitters the query is about:
      E1 an opaque emissive quad under the ceiling with a half-transparent and an alpha-textured occluder below it,
      E2 a non-opaque emitter (albedo alpha 0.5) with an emission texture,
      E3 an emissive quad coplanar with a non-emissive quad twice its size (the instance order of the pair is the argument),
    plus `extra_emitters` small emissive quads (to cross the threshold).  Returns the scene and {name: instance ids}."""
    from tauray_amd import scene as S, scenes
    rng = np.random.default_rng(seed)
    b = scenes._Builder()
    ids = {}

    def add(name, verts_idx, mat, model=None):
        ids.setdefault(name, []).append(len(b.inst))
        b.add(verts_idx[0], verts_idx[1], mat, model)

    grey = lambda a=0.6: S.make_material(albedo=(a, a * 0.9, a * 0.8, 1), metallic=0.0, roughness=0.7, double_sided=True)      # noqa: E731
    e = (9.0, 7.0, 4.0) if emission else (0, 0, 0)
    add("room", scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), 6, 6), grey(0.7))                    # floor
    add("room", scenes._quad((-4, 5, -4), (0, 0, 8), (8, 0, 0), 2, 2), grey(0.5))                    # ceiling
    add("room", scenes._quad((-4, 0, -4), (0, 5, 0), (8, 0, 0), 3, 3), grey(0.6))                    # back wall
    add("room", scenes._quad((-4, 0, -4), (0, 0, 8), (0, 5, 0), 3, 3), grey(0.6))                    # left wall (the right side and the front stay open: rays escape)
    for k in range(10):                                                                              # clutter
        p = rng.uniform((-3, 0.2, -3), (3, 3.0, 3))
        eu, ev = rng.normal(size=3) * 0.7, rng.normal(size=3) * 0.7
        add("clutter", scenes._quad(p, eu, ev, 2, 2), grey(float(rng.uniform(0.2, 0.9))))
    add("mirror", scenes._quad((-3.9, 0.5, -1), (0, 0, 2), (0, 2, 0)), S.make_material(albedo=(0.9, 0.9, 0.9, 1), metallic=1.0, roughness=0.0, double_sided=True))
    add("glass", scenes._quad((1.5, 0.3, -1), (0, 2, 0), (1, 0, 1.5)), S.make_material(albedo=(1, 1, 1, 1), metallic=0.0, roughness=0.0, transmittance=1.0, ior=1.4, double_sided=True))
    textures = [_holes_texture(3), _holes_texture(4)]
    add("E1", scenes._quad((-1, 4.9, -1), (2, 0, 0), (0, 0, 2)), S.make_material(albedo=(0, 0, 0, 1), metallic=0.0, roughness=1.0, emission=e, double_sided=True))
    add("occluder", scenes._quad((-1.2, 4.0, -1.2), (1.4, 0, 0), (0, 0, 2.4)), S.make_material(albedo=(0.8, 0.3, 0.3, 0.5), metallic=0.0, roughness=0.6, double_sided=True))
    add("occluder", scenes._quad((0.0, 4.2, -1.2), (1.4, 0, 0), (0, 0, 2.4)), S.make_material(albedo=(0.3, 0.8, 0.3, 1), metallic=0.0, roughness=0.6, double_sided=True, albedo_tex=0))
    add("E2", scenes._quad((-3, 0.8, 2.5), (2, 0, 0), (0, 1.5, 0)), S.make_material(albedo=(0.2, 0.2, 0.2, 0.5), metallic=0.0, roughness=1.0, emission=e, emission_tex=1, double_sided=True))
    big = scenes._quad((1.0, 0.5, -3.5), (2, 0, 0), (0, 2, 0))
    small = scenes._quad((1.5, 1.0, -3.5), (1, 0, 0), (0, 1, 0))
    em3 = S.make_material(albedo=(0, 0, 0, 1), metallic=0.0, roughness=1.0, emission=e, double_sided=True)
    for name in (("E3", "coplanar") if coplanar_emitter_first else ("coplanar", "E3")):
        add(name, small if name == "E3" else big, em3 if name == "E3" else grey(0.4))
    for k in range(extra_emitters):
        add("extra", scenes._quad((-3.5 + 0.4 * (k % 16), 4.95, 2.0 + 0.3 * (k // 16)), (0.2, 0, 0), (0, 0, 0.2)), em3)
    cam = S.Camera(fov=60, aspect=16 / 9)
    cam.transform = S.trs_matrix((0.3, 2.2, 3.9))         # at the open front, looking down -z into the room
    sc = S.SceneDesc(instances=np.concatenate(b.inst), spans=np.array(b.spans, dtype=S.MESH_SPAN), vertices=np.concatenate(b.verts),
                     indices=np.concatenate(b.idx).astype(np.uint32), textures=textures, envmap=np.ones((2, 4, 4), dtype=np.float32),
                     environment_factor=(0.25, 0.3, 0.4, 1.0), directional_lights=S.make_directional_light((3.0, 2.8, 2.5), (0.5, -1.0, 0.4), 0.5),
                     cameras=[cam]).finalize(gather)
    return sc, ids


def test_rig_has_the_cases_it_is_for():
    sc, ids = _rig()
    assert len(sc.instances) == 4 + 10 + 2 + 1 + 2 + 1 + 2 and sc.triangle_count > 150
    em = np.flatnonzero(np.any(sc.instances["mat"]["emission_factor"][:, :3] != 0, axis=1))
    assert sorted(em) == sorted(ids["E1"] + ids["E2"] + ids["E3"]) and int(sc.spans["triangle_count"][em].sum()) == 6
    pt = sc.potentially_transparent()
    assert pt[ids["E2"][0]] and pt[ids["occluder"]].all() and pt[ids["glass"][0]] and not pt[ids["E1"][0]]
    a, b = _rig(True)[1], _rig(False)[1]
    assert a["E3"][0] < a["coplanar"][0] and b["E3"][0] > b["coplanar"][0]
    assert sc.tri_light_count == 6 and _rig(gather=False)[0].tri_light_count == 0
    assert (_rig(gather=False)[0].instances["light_base_id"] == -1).all()


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


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _quad_points(sc, inst, rng, n):
    """n random points on the (planar, axis-aligned-uv) quad of instance `inst`, world space (the rig's models are identities)."""
    sp = sc.spans[inst]
    p = sc.vertices["pos"][sp["vertex_offset"]:sp["vertex_offset"] + sp["vertex_count"]].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    return lo + rng.uniform(0.02, 0.98, (n, 3)) * (hi - lo)


def _ray_sets(sc, ids, seed):
    rng = np.random.default_rng(seed)

    def pack(o, d, tmin, tmax):
        n = len(o)
        return np.concatenate([o, np.broadcast_to(np.asarray(tmin, np.float64).reshape(-1, 1), (n, 1)), d,
                               np.broadcast_to(np.asarray(tmax, np.float64).reshape(-1, 1), (n, 1))], 1).astype(np.float32)

    sets = {}
    n = 4000
    o = rng.uniform((-3.8, 0.1, -3.8), (3.8, 4.8, 3.8), (n, 3))
    sets["random"] = pack(o, _unit(rng.normal(size=(n, 3))), np.where(rng.uniform(size=n) < 0.5, 0.0, 1e-4),
                          np.where(rng.uniform(size=n) < 0.8, np.inf, rng.uniform(0.5, 8, n)))
    emitters = ids["E1"] + ids["E2"] + ids["E3"]
    for name, targets in (("aimed", emitters), ("through_occluders", ids["E1"]), ("coplanar", ids["E3"] + ids["coplanar"]), ("non_opaque_emitter", ids["E2"])):
        tgt = np.concatenate([_quad_points(sc, i, rng, n // len(targets)) for i in targets])
        if name == "through_occluders":       # from below the occluders, so that the ray to E1 crosses them
            o = np.stack([rng.uniform(-1.2, 1.4, len(tgt)), rng.uniform(0.2, 3.5, len(tgt)), rng.uniform(-1.2, 1.2, len(tgt))], 1)
        else:
            o = rng.uniform((-3.8, 0.1, -3.8), (3.8, 4.8, 3.8), (len(tgt), 3))
        sets[name] = pack(o, _unit(tgt - o), 1e-4, np.inf)
    m = 1500
    for name, tmin in (("from_an_emitter_tmin0", 0.0), ("from_an_emitter", 1e-4)):
        o = np.concatenate([_quad_points(sc, i, rng, m // len(emitters)) for i in emitters])
        d = _unit(rng.normal(size=o.shape))
        d[::3] = _unit(np.concatenate([_quad_points(sc, i, rng, m // len(emitters)) for i in emitters]) - o + 1e-9)[::3]      # in the emitter's own plane
        sets[name] = pack(o, d, tmin, np.inf)
    tgt = np.concatenate([_quad_points(sc, i, rng, m // len(emitters)) for i in emitters])
    o = rng.uniform((-3.8, 0.1, -3.8), (3.8, 4.8, 3.8), tgt.shape)
    dist = np.linalg.norm(tgt - o, axis=1)
    sets["tmin_cut"] = pack(o, _unit(tgt - o), dist * rng.uniform(0.9, 1.1, len(o)), np.inf)
    sets["tmax_cut"] = pack(o, _unit(tgt - o), 1e-4, dist * rng.uniform(0.9, 1.1, len(o)))
    return sets


def _check_terminal(got, ref, emitter_instances, what):
    """Nothing is left out: every ray's class is the class of the oracle's closest hit, and a miss or an emitter carries its record."""
    miss = ref["instance_id"] < 0
    emit = np.isin(ref["instance_id"], emitter_instances)
    blocked = ~miss & ~emit
    assert ((got["instance_id"] == BLOCKED) == blocked).all(), \
        f"{what}: class differs for {int(((got['instance_id'] == BLOCKED) != blocked).sum())} of {len(ref)} rays, first {np.flatnonzero((got['instance_id'] == BLOCKED) != blocked)[:5]}"
    keep = ~blocked
    bad = keep & ((got["instance_id"] != ref["instance_id"]) | (got["primitive_id"] != ref["primitive_id"]) | (got["t"].view(np.uint32) != ref["t"].view(np.uint32)))
    bad |= emit & ((got["bary_u"].view(np.uint32) != ref["bary_u"].view(np.uint32)) | (got["bary_v"].view(np.uint32) != ref["bary_v"].view(np.uint32)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} records differ, first {np.flatnonzero(bad)[:5]}"
    return int(miss.sum()), int(emit.sum()), int(blocked.sum())


def _check_closest(got, ref, what):
    bad = ((got["instance_id"] != ref["instance_id"]) | (got["primitive_id"] != ref["primitive_id"]) | (got["t"].view(np.uint32) != ref["t"].view(np.uint32)))
    hit = ref["instance_id"] >= 0
    bad |= hit & ((got["bary_u"].view(np.uint32) != ref["bary_u"].view(np.uint32)) | (got["bary_v"].view(np.uint32) != ref["bary_v"].view(np.uint32)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} hits differ, first {np.flatnonzero(bad)[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("emitter_first", [True, False])
def test_queries_match_the_oracle(R, ctx, oracle, emitter_first):
    sc, ids = _rig(coplanar_emitter_first=emitter_first)
    emitters = ids["E1"] + ids["E2"] + ids["E3"]
    osc = oracle.OracleScene(sc)
    ss = R.SceneStage(ctx, sc)
    totals = np.zeros(3, np.int64)
    per_set = {}
    for name, rays in _ray_sets(sc, ids, 7).items():
        seeds = np.random.default_rng(len(rays)).integers(0, 2**32, len(rays), dtype=np.uint64).astype(np.uint32)
        for sd in (None, seeds):
            ref = osc.trace_closest(rays, sd)
            counts = _check_terminal(ss.trace_terminal(rays, sd), ref, emitters, f"{name} seeds={sd is not None}")
            per_set[name] = np.asarray(counts) + per_set.get(name, 0)
            totals += counts
            # the per-ray fallback: flagged rays are ordinary closest hits, the others keep their class
            fb = (np.arange(len(rays)) % 3 == 0).astype(np.uint32)
            got = ss.trace_terminal(rays, sd, fallback=fb)
            _check_closest(got[fb != 0], ref[fb != 0], f"{name} fallback rays")
            _check_terminal(got[fb == 0], ref[fb == 0], emitters, f"{name} next to fallback rays")
    assert (totals > 500).all(), totals                               # the sets hold misses, emitter hits and blocked rays
    assert per_set["through_occluders"][1] > 100 and per_set["through_occluders"][2] > 100      # the occluders let some rays through
    assert per_set["non_opaque_emitter"][1] > 100 and per_set["coplanar"][1] > 50 and per_set["coplanar"][2] > 50
    assert per_set["from_an_emitter_tmin0"][1] > 20 and per_set["tmin_cut"][1] > 50


@pytest.mark.gpu
def test_query_refuses_what_it_cannot_answer(R, ctx):
    sc, _ = _rig(extra_emitters=8)        # 6 + 16 emitter triangles
    ss = R.SceneStage(ctx, sc)
    rays = np.array([[0, 1, 0, 0, 0, 1, 0, np.inf]], np.float32)
    with pytest.raises(R.TrhipError, match="emitter triangles"):
        ss.trace_terminal(rays)
    ss2 = R.SceneStage(ctx, _rig()[0], as_strategy=1)
    with pytest.raises(R.TrhipError, match="all-merged"):
        ss2.trace_terminal(rays)


def _frame(R, ctx, ss, scene, size, mode, ieee=None, count=True, shard=None, **kw):
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, **kw), DistributionParams(tuple(size), DISTRIBUTION_DUPLICATE, 0, 1, True))
    pt.set_terminal_query(mode)
    if ieee is not None:
        pt.set_shading_arithmetic(ieee)
    if shard is not None:
        pt.set_shard(**shard)
    if count:
        pt.set_profiling(count_work=True)
        pt.reset_counters()
    color = ctx.alloc(size[0] * size[1] * 16).zero()
    pt.run(color)
    img = color.download((size[1], size[0], 4))
    c, tc = pt.counters(), pt.terminal_counters()
    assert c["stack_overflows"] == 0
    pt.close()
    return img, c, tc


def _same_frames(R, ctx, ss, sc, size, what, expect_on=True, interior=False, arithmetics=(True, False), **kw):
    """AUTO and OFF give the same bits and the same ray and surface counts; returns AUTO's counters."""
    out = None
    for ieee in arithmetics:
        a, ca, ta = _frame(R, ctx, ss, sc, size, OFF, ieee=ieee, **kw)
        b, cb, tb = _frame(R, ctx, ss, sc, size, AUTO, ieee=ieee, **kw)
        assert (a[..., :3] > 0).mean() > 0.1, what            # not a black frame (one bounce shows the emitters and the environment only)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what} ieee={ieee}: {int((a.view(np.uint32) != b.view(np.uint32)).any(-1).sum())} pixels differ"
        for k in ("closest_rays", "shadow_rays", "surface_hits"):
            assert ca[k] == cb[k], (what, ieee, k, ca[k], cb[k])
        assert ta["in_effect"] == 0 and ta["blocked_rays"] == 0 and ta["fallback_rays"] == 0, (what, ta)
        assert tb["in_effect"] == (1 if expect_on else 0), (what, tb)
        if expect_on:
            assert tb["blocked_rays"] > 0, (what, tb)       # the mode is not silently off
            assert tb["blocked_rays"] + tb["fallback_rays"] <= cb["closest_rays"]
            if interior:
                assert cb["node_visits"] < ca["node_visits"], (what, ca["node_visits"], cb["node_visits"])
        else:
            assert tb["blocked_rays"] == 0 and tb["fallback_rays"] == 0, (what, tb)
            # (node visits of two runs of the same launches differ by a few: which rays a wave hands to its quad tail depends on timing)
        # frames without work counting run the fused launches: the same bits again
        c2 = _frame(R, ctx, ss, sc, size, AUTO, ieee=ieee, count=False, **kw)[0]
        assert np.array_equal(a.view(np.uint32), c2.view(np.uint32)), f"{what} ieee={ieee}, fused launches"
        out = (cb, tb)
    return out


OPTION_SETS = [dict(max_bounces=4), dict(max_bounces=2), dict(max_bounces=4, sampler=1),
               dict(max_bounces=4, russian_roulette_delta=2.0, regularization_gamma=0.5, indirect_clamping=4.0)]


@pytest.mark.gpu
def test_frames_do_not_depend_on_the_mode_rig(R, ctx):
    sc, _ = _rig()
    ss = R.SceneStage(ctx, sc)
    for kw in OPTION_SETS:
        _same_frames(R, ctx, ss, sc, (160, 90), f"rig {kw}", interior=True, **kw)
    _same_frames(R, ctx, ss, sc, (160, 90), "rig, one bounce", expect_on=False, max_bounces=1)       # the only bounce feeds the first-hit targets
    # shards of the viewports and samples
    _same_frames(R, ctx, ss, sc, (160, 90), "rig, sample shard", interior=True, max_bounces=4, shard=dict(sample_base=1, sample_stride=2))
    # tri-light NEE off: the emission still arrives through mat.emission, and the emitters are still emitters
    sc2, _ = _rig(gather=False)
    ss2 = R.SceneStage(ctx, sc2)
    cb, tb = _same_frames(R, ctx, ss2, sc2, (160, 90), "rig, no tri lights", interior=True, max_bounces=4)
    assert tb["emitter_triangles"] == 6


@pytest.mark.gpu
def test_more_emitters_than_the_threshold_switch_the_mode_off(R, ctx):
    sc, _ = _rig(extra_emitters=8)
    ss = R.SceneStage(ctx, sc)
    cb, tb = _same_frames(R, ctx, ss, sc, (160, 90), "rig + 8 emissive quads", expect_on=False, max_bounces=4)
    assert tb["emitter_triangles"] == 22 and tb["threshold"] < 22
    # ... and so do a two-level structure and a sphere light
    ss2 = R.SceneStage(ctx, _rig()[0], as_strategy=1)
    _same_frames(R, ctx, ss2, _rig()[0], (160, 90), "rig, two-level", expect_on=False, arithmetics=(False,), max_bounces=4)
    from tauray_amd import scene as S
    sc3 = copy.copy(_rig()[0])
    sc3.point_lights = S.make_point_light((5, 5, 5), (0, 3, 0), 0.2)
    _same_frames(R, ctx, R.SceneStage(ctx, sc3), sc3, (160, 90), "rig + sphere light", expect_on=False, arithmetics=(False,), max_bounces=4)
    sc3.point_lights = S.make_point_light((5, 5, 5), (0, 3, 0), 0.0)      # a light without a sphere is no obstacle
    _same_frames(R, ctx, R.SceneStage(ctx, sc3), sc3, (160, 90), "rig + point light", arithmetics=(False,), max_bounces=4)


@pytest.mark.gpu
def test_frames_do_not_depend_on_the_mode_bench_scenes(R, ctx):
    from tauray_amd import scenes
    from tauray_amd.gltf import load_glb
    glb = load_glb(os.path.join(GOLDEN, "test.glb"), 160, 90)
    n_sphere = int((glb.point_lights["radius"] != 0).sum())
    _same_frames(R, ctx, R.SceneStage(ctx, glb), glb, (160, 90), "test.glb", expect_on=n_sphere == 0, max_bounces=4)
    sc = scenes.sponza_class(3, 60_000, 0, 160, 90)
    ss = R.SceneStage(ctx, sc)
    for kw in (dict(max_bounces=4), dict(max_bounces=2)):
        _same_frames(R, ctx, ss, sc, (160, 90), f"sponza_class {kw}", interior=True, **kw)
    sc = scenes.sponza_teapots(1, 320, 180)
    _same_frames(R, ctx, R.SceneStage(ctx, sc), sc, (320, 180), "sponza_teapots", interior=True, max_bounces=4)


@pytest.mark.gpu
def test_emission_switched_on_and_off_by_update_instances(R, ctx):
    """Materials can change: the emitter set follows trhip_scene_update_instances through the rebuild or the refit after it."""
    sc, ids = _rig(gather=False)
    ss = R.SceneStage(ctx, sc)
    base = _same_frames(R, ctx, ss, sc, (160, 90), "before", interior=True, arithmetics=(False,), max_bounces=4)[1]
    assert base["emitter_triangles"] == 6
    dark = sc.instances.copy()
    dark["mat"]["emission_factor"][ids["E1"][0]] = 0
    lit = sc.instances.copy()
    lit["mat"]["emission_factor"][ids["clutter"][0]] = (5, 5, 5, 0)
    for refit in (False, True):
        for inst, n_emit, what in ((dark, 4, "E1 off"), (lit, 14, "clutter on"), (sc.instances, 6, "back")):
            ss.update_instances(inst, refit=refit)
            sc_now = copy.copy(sc)
            sc_now.instances = inst
            tc = _same_frames(R, ctx, ss, sc_now, (160, 90), f"{what} refit={refit}", interior=True, arithmetics=(False,), max_bounces=4)[1]
            assert tc["emitter_triangles"] == n_emit, (what, refit, tc)
    # the frame with E1 dark differs from the frame with it lit: the update reached the image
    ss.update_instances(dark, refit=True)
    a = _frame(R, ctx, ss, sc, (160, 90), AUTO, max_bounces=4)[0]
    ss.update_instances(sc.instances, refit=True)
    b = _frame(R, ctx, ss, sc, (160, 90), AUTO, max_bounces=4)[0]
    assert not np.array_equal(a, b)


@pytest.mark.gpu
def test_environment_switch(R, ctx):
    """TRHIP_TERMINAL_QUERY chooses the mode of a stage on which none was set (any letter case); another value is an error, not AUTO."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    sc, _ = _rig()
    ss = R.SceneStage(ctx, sc)
    old = os.environ.get("TRHIP_TERMINAL_QUERY")
    try:
        for value, on in (("Off", 0), ("AUTO", 1), ("", 1)):
            os.environ["TRHIP_TERMINAL_QUERY"] = value
            pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=4), DistributionParams((64, 36), DISTRIBUTION_DUPLICATE, 0, 1, True))
            assert pt.terminal_counters()["in_effect"] == on, value
            pt.set_terminal_query(OFF)
            assert pt.terminal_counters()["in_effect"] == 0
            pt.close()
        os.environ["TRHIP_TERMINAL_QUERY"] = "on"
        pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=4), DistributionParams((64, 36), DISTRIBUTION_DUPLICATE, 0, 1, True))
        color = ctx.alloc(64 * 36 * 16).zero()
        with pytest.raises(R.TrhipError, match="TRHIP_TERMINAL_QUERY"):
            pt.run(color)
        with pytest.raises(R.TrhipError, match="unknown mode"):
            pt.set_terminal_query(2)
        pt.close()
    finally:
        if old is None:
            os.environ.pop("TRHIP_TERMINAL_QUERY", None)
        else:
            os.environ["TRHIP_TERMINAL_QUERY"] = old
