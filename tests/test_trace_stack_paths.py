"""The deep end of the per-lane traversal stack (csrc/trace.h LaneStack): pushes that cross from the LDS rows into
the spill rows, pops that come back, the re-deal of spilled stacks to the quad tail, and the sphere-light step behind a closest hit.

The scene is a "deck": DECK_QUADS coincident-in-xy quads a hair apart along z, so that a ray along z hits every child box of every node
and holds more than TR_LDS_STACK entries (the depth reached is asserted on a counting frame: test_deck_reaches_the_spill_rows).  With
alpha 0 everywhere an any-hit ray ends nowhere and its visibility is exactly 1 in any order, exactly 0 where the opaque plate stands
behind the deck; with stochastic alpha 0.5 acceptance is a hash of (seed, instance, primitive), so closest hits are order-independent and
must equal the oracle's bit for bit."""
import numpy as np
import pytest

DECK_QUADS = 16384         # 4096 reach a depth of 19 entries, one short of TR_LDS_STACK + 4; every factor of four adds a level of the tree
SHORT_QUADS = 40           # what the short rays of the last wave cross
DECK_DEPTH = 1.0            # the deck fills z in [0, DECK_DEPTH)
PLATE_Z = 1.5
TR_LDS_STACK = 16           # csrc/trace.h
N_RAYS = 256                # four waves
LIGHT = ((0.45, -0.35, -0.5), 0.2)      # sphere light in front of the deck: centre, radius


def _deck_scene(alpha, light=False):
    from tauray_amd import scene as S, scenes
    b = scenes._Builder()
    qv, qi = scenes._quad((-1, -1, 0), (2, 0, 0), (0, 2, 0))
    verts = np.tile(qv, DECK_QUADS)
    verts["pos"][:, 2] = np.repeat(np.arange(DECK_QUADS, dtype=np.float64) * (DECK_DEPTH / DECK_QUADS), len(qv))
    # half-sizes between 1 and 1.25, no two alike: with equal quads every merge the builder weighs costs the same, and its clustering of a
    # deck this size does not converge ("PLOC: clustering did not converge")
    verts["pos"][:, :2] *= np.repeat(1.0 + 0.25 * np.random.default_rng(5).permutation(DECK_QUADS) / DECK_QUADS, len(qv))[:, None]
    idx = (np.tile(np.asarray(qi).reshape(-1), DECK_QUADS) + np.repeat(np.arange(DECK_QUADS) * len(qv), len(np.asarray(qi).reshape(-1)))).astype(np.uint32)
    b.add(verts, idx, S.make_material(albedo=(0.8, 0.7, 0.6, alpha), metallic=0.0, roughness=0.8, double_sided=True))                                # instance 0: the deck
    b.add(*scenes._quad((-1, -1, PLATE_Z), (1, 0, 0), (0, 2, 0)), S.make_material(albedo=(0.5, 0.5, 0.5, 1), metallic=0.0, roughness=0.8, double_sided=True))    # instance 1: the plate, x < 0
    cam = S.Camera(fov=40, aspect=1.0)
    cam.transform = S.trs_matrix((0.0, 0.0, 4.0))          # looking down -z: the plate in front of one half, the deck's back behind the other
    sc = S.SceneDesc(instances=np.concatenate(b.inst), spans=np.array(b.spans, dtype=S.MESH_SPAN), vertices=np.concatenate(b.verts),
                     indices=np.concatenate(b.idx).astype(np.uint32), textures=[], envmap=np.ones((2, 4, 4), dtype=np.float32),
                     environment_factor=(0.5, 0.5, 0.5, 1.0), cameras=[cam])
    if light:
        sc.point_lights = S.make_point_light((5.0, 5.0, 5.0), LIGHT[0], LIGHT[1])
    return sc.finalize(True)


def _rays():
    """256 rays from z = -1 along +z with a small tilt, at least 0.1 from the plate's edge (x = 0) and from the quads' diagonal (x = y).
    Rays 0 .. 191: through the whole deck.  Rays 192 .. 255 (the last wave): twelve such rays among 52 that end behind the first forty
    quads - those live for a few node phases and are gone, which leaves the wave to the quad tail while the twelve hold deep stacks.
    Eight rays of the first wave start on the axis of the sphere light."""
    rng = np.random.default_rng(22)
    xy = np.zeros((N_RAYS, 2))
    for i in range(N_RAYS):
        while True:
            p = rng.uniform(-0.9, 0.9, 2)
            if abs(p[0]) > 0.1 and abs(p[0] - p[1]) > 0.1:
                xy[i] = p
                break
    xy[8:16] = np.asarray(LIGHT[0][:2]) + rng.uniform(-0.05, 0.05, (8, 2))
    d = np.concatenate([rng.uniform(-0.01, 0.01, (N_RAYS, 2)), np.ones((N_RAYS, 1))], 1)
    d[::7, :2] = 0.0                                       # some exactly along the axis: two slabs without a direction
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    long_ray = np.ones(N_RAYS, bool)
    long_ray[192:] = False
    long_ray[192 + 5 * np.arange(12)] = True
    tmax = np.where(long_ray, np.inf, 1.0 + (SHORT_QUADS + 0.5) * DECK_DEPTH / DECK_QUADS)
    rays = np.concatenate([xy, -np.ones((N_RAYS, 1)), np.full((N_RAYS, 1), 1e-4), d, tmax[:, None]], 1).astype(np.float32)
    seeds = rng.integers(0, 2**32, N_RAYS, dtype=np.uint64).astype(np.uint32)
    return rays, seeds, long_ray


def _pcg(s):
    s = (s * np.uint32(747796405) + np.uint32(2891336453)).astype(np.uint32)
    s = (((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)).astype(np.uint32)
    return ((s >> np.uint32(22)) ^ s).astype(np.uint32)


def _accepts(seed, instance, prim, alpha):
    """rt_common.rahit with the traversal-order independent cutoff (csrc/trace.h alpha_cutoff_hash): accepted unless alpha <= cutoff."""
    with np.errstate(over="ignore"):
        k = (np.uint32(instance) * np.uint32(0x9E3779B9) + prim.astype(np.uint32)).astype(np.uint32)
        cutoff = _pcg(np.uint32(seed) ^ _pcg(k)).astype(np.float32) * np.float32(2.3283064365386963e-10)
    return ~(np.float32(alpha) <= cutoff)


def _expected_closest(rays, seeds, alpha):
    """(instance, primitive) per ray, from the geometry alone: the first quad along z whose triangle under the ray accepts, else the plate
    (x < 0), else nothing; tmax cuts the walk."""
    inst, prim = np.full(len(rays), -1), np.full(len(rays), -1)
    z = np.arange(DECK_QUADS) * (DECK_DEPTH / DECK_QUADS)
    for i, r in enumerate(rays.astype(np.float64)):
        par = 0 if r[0] > r[1] else 1                      # _grid_mesh: triangle (a, b, d) has u > v, (a, d, c) has v > u
        t = (z + 1.0) / r[6]
        prims = 2 * np.arange(DECK_QUADS) + par
        ok = _accepts(seeds[i], 0, prims, alpha) & (t < r[7]) if alpha > 0 else np.zeros(DECK_QUADS, bool)
        if ok.any():
            inst[i], prim[i] = 0, prims[np.argmax(ok)]
        elif r[0] < 0 and (PLATE_Z + 1.0) / r[6] < r[7]:
            inst[i] = 1
    return inst, prim


@pytest.fixture(scope="module")
def deck():
    """Scenes, rays and the oracle's answers, computed once: alpha 0 (any-hit and full-length closest walks) and alpha 0.5 (closest, terminal)."""
    from oracle import binding as B
    rays, seeds, long_ray = _rays()
    d = {"rays": rays, "seeds": seeds, "long": long_ray}
    for name, alpha in (("clear", 0.0), ("half", 0.5)):
        sc = _deck_scene(alpha)
        osc = B.OracleScene(sc)
        d[name] = {"scene": sc, "closest": osc.trace_closest(rays, seeds), "closest_cutoff": osc.trace_closest(rays, None), "shadow": osc.trace_shadow(rays),
                   "closest_lights": osc.trace_closest(rays, seeds, include_lights=True)}
    sc = _deck_scene(0.5, light=True)
    d["lit"] = {"scene": sc, "closest_lights": B.OracleScene(sc).trace_closest(rays, seeds, include_lights=True)}
    return d


def test_the_oracle_gives_what_the_deck_is_built_for(deck):
    rays, seeds, long_ray = deck["rays"], deck["seeds"], deck["long"]
    assert deck["clear"]["scene"].triangle_count == 2 * DECK_QUADS + 2 and len(rays) == N_RAYS
    assert long_ray[:192].all() and long_ray[192:].sum() == 12
    behind_plate = long_ray & (rays[:, 0] < 0)
    assert 60 < behind_plate.sum() < 150
    # any-hit, alpha 0: exactly 0 behind the plate, exactly 1 elsewhere
    assert (deck["clear"]["shadow"] == np.where(behind_plate, 0.0, 1.0).astype(np.float32)).all()
    # any-hit, alpha 0.5: the product underflows to exactly 0 over the full deck; forty or forty-one quads leave 2^-40 or 2^-41
    assert (deck["half"]["shadow"][long_ray] == 0).all() and (deck["half"]["shadow"][~long_ray] > 0).all()
    for name, alpha in (("clear", 0.0), ("half", 0.5)):
        inst, prim = _expected_closest(rays, seeds, alpha)
        got = deck[name]["closest"]
        assert (got["instance_id"] == inst).all(), name
        assert (got["primitive_id"][inst == 0] == prim[inst == 0]).all(), name
        # no sphere light in these scenes: asking for lights changes nothing
        assert got.tobytes() == deck[name]["closest_lights"].tobytes()
    assert (deck["clear"]["closest_cutoff"]["instance_id"] == deck["clear"]["closest"]["instance_id"]).all()
    assert (deck["half"]["closest_cutoff"]["primitive_id"][long_ray] == (rays[long_ray, 0] <= rays[long_ray, 1])).all()      # fixed cutoff: the first quad
    depth = deck["half"]["closest"]["primitive_id"] // 2
    assert depth.max() >= 6 and (depth == 0).sum() < N_RAYS * 0.7            # hits at many depths of the deck
    lit = deck["lit"]["closest_lights"]
    on_light = (lit["instance_id"] == -1) & (lit["primitive_id"] == 0)
    assert on_light[8:16].all() and 8 <= on_light.sum() < 64
    assert (lit[~on_light].tobytes() == deck["half"]["closest"][~on_light].tobytes())


# ---------------------------------------------------------------------------------------------------------------------------------
# on the GPU

@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


def _same_hits(got, ref, what):
    bad = (got["instance_id"] != ref["instance_id"]) | (got["primitive_id"] != ref["primitive_id"]) | (got["t"].view(np.uint32) != ref["t"].view(np.uint32))
    hit = ref["instance_id"] >= 0
    bad |= hit & ((got["bary_u"].view(np.uint32) != ref["bary_u"].view(np.uint32)) | (got["bary_v"].view(np.uint32) != ref["bary_v"].view(np.uint32)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} hits differ, first {np.flatnonzero(bad)[:5]}"


@pytest.mark.gpu
def test_deck_reaches_the_spill_rows(R, ctx, deck):
    """Non-vacuity: a 64 x 64 counting frame of the deck holds stacks of at least TR_LDS_STACK + 4 entries.  Measured on an MI355X: 93
    entries with the 16 384 quads of unequal size (76 of them in the spill rows); 4 096 equal quads reached 19."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    sc = deck["clear"]["scene"]
    ss = R.SceneStage(ctx, sc)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=2), DistributionParams((64, 64), DISTRIBUTION_DUPLICATE, 0, 1, True))
    pt.set_profiling(count_work=True)
    pt.reset_counters()
    color = ctx.alloc(64 * 64 * 16).zero()
    pt.run(color)
    c, depth = pt.counters(), pt.max_stack_depth()
    pt.close()
    print(f"deck of {DECK_QUADS} quads: deepest stack {depth} entries, {c['node_visits']} node visits, {c['tri_tests']} triangle tests")
    assert c["stack_overflows"] == 0
    assert depth >= TR_LDS_STACK + 4, depth


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["clear", "half"])
def test_deck_queries_match_the_oracle(R, ctx, deck, name):
    rays, seeds, ref = deck["rays"], deck["seeds"], deck[name]
    ss = R.SceneStage(ctx, ref["scene"])
    # any-hit: exact, whatever the order of the product
    vis = ss.trace_shadow(rays)
    assert (vis.view(np.uint32) == ref["shadow"].view(np.uint32)).all() if name == "clear" else ((vis == 0) == (ref["shadow"] == 0)).all()
    if name == "half":      # the short rays multiply forty factors of exactly 0.5: exact in any order
        assert (vis.view(np.uint32) == ref["shadow"].view(np.uint32)).all()
    # closest hit, stochastic alpha and fixed cutoff, with and without the sphere-light step (no light here: point_light_count == 0)
    _same_hits(ss.trace_closest(rays, seeds), ref["closest"], f"{name} closest")
    _same_hits(ss.trace_closest(rays, None), ref["closest_cutoff"], f"{name} closest, fixed cutoff")
    _same_hits(ss.trace_closest(rays, seeds, include_lights=True), ref["closest_lights"], f"{name} closest, zero lights")
    # the terminal query walks in slot order (push_packed): as a fallback ray it is a closest hit, otherwise hit = blocked (no emitters)
    _same_hits(ss.trace_terminal(rays, seeds, fallback=np.ones(N_RAYS, np.uint32)), ref["closest"], f"{name} terminal fallback")
    term = ss.trace_terminal(rays, seeds)
    miss = ref["closest"]["instance_id"] < 0
    assert ((term["instance_id"] == -2) == ~miss).all() and (term["instance_id"][miss] == -1).all()


@pytest.mark.gpu
def test_one_sphere_light_in_front_of_the_deck(R, ctx, deck):
    rays, seeds, ref = deck["rays"], deck["seeds"], deck["lit"]
    ss = R.SceneStage(ctx, ref["scene"])
    _same_hits(ss.trace_closest(rays, seeds, include_lights=True), ref["closest_lights"], "one light")
    _same_hits(ss.trace_closest(rays, seeds), deck["half"]["closest"], "one light, not asked for")
