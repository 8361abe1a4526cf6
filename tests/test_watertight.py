"""Ray queries against a float64 brute force (tests/ray_reference.py): closed meshes, rays aimed exactly at and within an ulp of shared
edges and vertices.  The rest of the suite holds the GPU's geometry against oracle/oracle.cc, whose triangle test, fp64 fallback and slab
pad are the kernels' own, line for line; here neither is the reference.  The CPU part holds the oracle against the brute force - it is
where the bounds come from - and the GPU part holds the kernels against the brute force alone, under all three acceleration
structures, through all three queries, in nearly empty waves, after a refit and through a frame kernel.

Conditions, without exception on any ray: every aimed ray hits; the primitive is the float64 winner or shares a vertex with it;
|t - T| <= B max(T, |origin|); the point at the reported barycentrics lies within B_P x the placement's scale of origin + T direction;
a shadow ray with tmax = 1.01 T is blocked, with 0.99 T it is not.  On the lattices' exact rays t == T."""
import functools

import numpy as np
import pytest

import ray_reference as RR

ALL, PER_MESH, STATIC_MERGED = 0, 1, 2
HIT_BLOCKED = -2

# Distance bound B per mesh: four times the oracle's largest |t - T| / max(T, |origin|) over the placements and families of that mesh,
# rounded up to one digit.  test_oracle_against_brute_force asserts that the oracle stays below B / 2, so the constant can drift neither
# way unnoticed.  Measured (oracle against brute force, this file's seeds):
#   icosphere   3.857e-7   (`rot`, outside; 3.166e-7 at `unit`, `small` and `large`, below 3e-9 at `far` and `rotfar`)
#   bipyramid   2.024e-6   (`unit`, `small` and `large`, inside: the needles' hit distance is ill-conditioned in the edge functions)
#   lattices    0: t == T on all 2700 exact rays, and on the same rays under the dyadic placement
B = {"icosphere": 2e-6, "bipyramid": 9e-6, "flat": 0.0, "bumpy": 0.0}
# Hit-point bound B_P per mesh, in units of the placement's scale, derived the same way from the oracle's largest
# |P(primitive, u, v) - (origin + T direction)| / scale:
#   icosphere   4.973e-7   (`rot`, outside)
#   bipyramid   3.819e-6   (`rot`, outside)
#   lattices    0: the barycentrics of the exact rays are exact
B_P = {"icosphere": 2e-6, "bipyramid": 2e-5, "flat": 0.0, "bumpy": 0.0}


def two_level_bounds(mesh):
    """(distance, hit point) bounds under a two-level structure, which traces the world ray re-rounded in object space.  1e-5 is the
    project's own measured bound for non-grazing hits (test_accel_strategies.test_two_level_agrees_with_the_world_space_result); for
    the bipyramid's needles it is multiplied by B[bipyramid] / B[icosphere], the conditioning factor of the same kind of rounding as
    measured on the oracle.  The distance bound is max(B, 1e-5) x that factor, the hit-point bound max(B_P, 1e-5 x that factor)."""
    k = B["bipyramid"] / B["icosphere"] if mesh == "bipyramid" else 1.0
    return max(B[mesh], 1e-5) * k, max(B_P[mesh], 1e-5 * k)


ROT = ((0.3, 0.5, -0.2, 0.8), (1.3, 0.7, 1.0))
# name: (translation, rotation, scale, the placement's scale)
PLACEMENTS = {
    "unit": ((0, 0, 0), (0, 0, 0, 1), (1, 1, 1), 1.0),
    "far": ((1000, 1000, 1000), (0, 0, 0, 1), (1, 1, 1), 1.0),
    "small": ((0, 0, 0), (0, 0, 0, 1), (1 / 1024,) * 3, 1 / 1024),
    "large": ((0, 0, 0), (0, 0, 0, 1), (1024,) * 3, 1024.0),
    "rot": ((0.3, -0.2, 0.1),) + ROT + (1.0,),
    "rotfar": ((300, -200, 100),) + ROT + (1.0,),
    "dyadic": ((0.5, -0.25, 1.0), (0, 0, 0, 1), (2, 2, 2), 1.0),        # the lattices' two-level placement: exact in float32
}
SOLIDS = [(m, p) for m in ("icosphere", "bipyramid") for p in ("unit", "far", "small", "large", "rot", "rotfar")]
LATTICES = [(m, p) for m in ("flat", "bumpy") for p in ("unit", "dyadic")]
SEEDS = {"inside": 101, "outside": 202, "tilted": 303}


@functools.lru_cache(maxsize=None)
def _mesh(mesh):
    if mesh == "icosphere":
        v, t = RR.icosphere(3)
        assert v.shape == (642, 3) and t.shape == (1280, 3)
    elif mesh == "bipyramid":
        v, t = RR.bipyramid(256)
        assert v.shape == (258, 3) and t.shape == (512, 3)
    else:
        v, t = RR.lattice(16, np.zeros((17, 17)) if mesh == "flat" else RR.bumpy_heights(16, 7))
        assert v.shape == (289, 3) and t.shape == (512, 3)
    return v, t


def _scene(mesh, placement):
    """One opaque instance of the mesh under the placement, no light, a camera at the placement's translation."""
    from tauray_amd import scene as S
    v, t = _mesh(mesh)
    tr, rot, sc, _ = PLACEMENTS[placement]
    verts = np.zeros(len(v), dtype=S.VERTEX)
    verts["pos"] = v
    verts["normal"] = (0, 0, 1)
    verts["tangent"] = (1, 0, 0, 1)
    inst = S.make_instance(S.trs_matrix(tr, rot, sc), S.make_material(albedo=(0.8, 0.8, 0.8, 1), metallic=0.0, roughness=0.5, double_sided=True))
    cam = S.Camera(fov=90, aspect=1.0)
    cam.transform = S.trs_matrix(tr)
    return S.SceneDesc(instances=inst, spans=np.array([(0, len(v), 0, len(t))], dtype=S.MESH_SPAN), vertices=verts,
                       indices=t.reshape(-1).astype(np.uint32), cameras=[cam]).finalize(True)


@functools.lru_cache(maxsize=None)
def _case(mesh, placement):
    """Scene, world geometry, ray families and their float64 answers - computed once per process and never written to."""
    scene = _scene(mesh, placement)
    P, tri = RR.world_vertices(scene)
    scale = PLACEMENTS[placement][3]
    tmin = 1e-4 * scale
    if mesh in ("flat", "bumpy"):
        fams = {"exact": RR.exact(P, tri, 16, tmin)}
        if mesh == "flat":
            fams["tilted"] = RR.exact(P, tri, 16, tmin, tilt_seed=SEEDS["tilted"])
        assert all(len(r) == 900 for r, _ in fams.values())
    else:
        fams = {"inside": RR.inside(mesh, P, tri, SEEDS["inside"], tmin), "outside": RR.outside(mesh, P, tri, SEEDS["outside"], tmin)}
        assert all(len(r) == RR.N_RAYS for r, _ in fams.values())
    out = {}
    for name, (rays, adj) in fams.items():
        T, I, M = RR.brute_force(rays, P, tri)
        for a in (rays, adj, T, I, M):
            a.setflags(write=False)
        out[name] = dict(rays=rays, adj=adj, T=T, I=I, M=M)
    return dict(mesh=mesh, placement=placement, scene=scene, P=P, tri=tri, scale=scale, families=out)


@pytest.fixture(scope="module")
def cases():
    """_case: rays and float64 answers, computed once per (mesh, placement) and shared by the CPU and the GPU tests of the module."""
    return _case


def _seeds(n):
    return np.random.default_rng(5).integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)


def _shadow_rays(f, factor):
    r = f["rays"].copy()
    r[:, 7] = (factor * f["T"]).astype(np.float32)
    return r


def _reference_is_sound(case):
    """What the float64 answers themselves must satisfy: every ray hits, an aimed ray hits at its target, an exact ray on an edge."""
    for name, f in case["families"].items():
        what = f"{case['mesh']} {case['placement']} {name}"
        assert (f["I"] >= 0).all() and np.isfinite(f["T"]).all(), f"{what}: the brute force misses {int((f['I'] < 0).sum())} rays"
        aimed = f["adj"][:, 0] >= 0
        near = np.zeros(len(aimed), bool)
        for k in range(2):       # a vertex target's triangles all share it; an edge target's two hold the edge's ends between them
            near |= RR.shares_vertex(case["tri"], f["I"], f["adj"][:, k])
        assert near[aimed].all(), f"{what}: {int((~near[aimed]).sum())} aimed rays hit away from their target"
        assert aimed.sum() == (len(aimed) if name != "inside" else 2 * (len(aimed) // 3))
        if name in ("exact", "tilted"):
            assert (f["M"] == 0).all(), f"{what}: float64 margin {np.abs(f['M']).max()}"


def _check_hits(case, name, got, b, b_p, what, exact=False, point_scale=None):
    """The hit, primitive, distance and hit-point conditions of `got` against the family's float64 answers; returns the measured
    (distance error / max(T, |origin|), hit-point error / scale) maxima.  No exception is allowed."""
    f = case["families"][name]
    rays, T, I = f["rays"].astype(np.float64), f["T"], f["I"]
    hit = got["instance_id"] >= 0
    assert hit.all(), f"{what}: {int((~hit).sum())} of {len(hit)} rays miss, first {np.flatnonzero(~hit)[:5]}"
    assert (got["instance_id"] == 0).all()
    near = RR.shares_vertex(case["tri"], got["primitive_id"], I)
    assert near.all(), f"{what}: {int((~near).sum())} primitives away from the float64 winner, first {np.flatnonzero(~near)[:5]}"
    t = got["t"].astype(np.float64)
    terr = np.abs(t - T) / np.maximum(T, np.abs(rays[:, :3]).max(1))
    if exact:
        assert (t == T).all(), f"{what}: t != T on {int((t != T).sum())} exact rays"
    assert (terr <= b).all(), f"{what}: distance error {terr.max():.3e} > {b:.1e} on {int((terr > b).sum())} rays"
    p = RR.hit_points(case["P"], case["tri"], got["primitive_id"], got["bary_u"], got["bary_v"])
    perr = np.linalg.norm(p - (rays[:, :3] + T[:, None] * rays[:, 4:7]), axis=1) / (case["scale"] if point_scale is None else point_scale)
    assert (perr <= b_p).all(), f"{what}: hit point {perr.max():.3e} > {b_p:.1e} on {int((perr > b_p).sum())} rays"
    return float(terr.max()), float(perr.max())


def _check_shadow(case, name, trace_shadow, what):
    f = case["families"][name]
    blocked, free = trace_shadow(_shadow_rays(f, 1.01)), trace_shadow(_shadow_rays(f, 0.99))
    assert (blocked == 0).all(), f"{what}: {int((blocked != 0).sum())} shadow rays leak past their hit"
    assert (free == 1).all(), f"{what}: {int((free != 1).sum())} shadow rays are blocked in front of their hit"


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU: the oracle against the brute force

def test_meshes_are_closed_and_share_vertices():
    for mesh, nv, nt in (("icosphere", 642, 1280), ("bipyramid", 258, 512)):
        v, t = _mesh(mesh)
        edges, owners = RR._edges(t)
        assert len(v) == nv and len(t) == nt and (owners >= 0).all() and len(edges) == 3 * nt // 2      # every edge has two triangles
    valence = np.bincount(_mesh("bipyramid")[1].ravel())
    assert (np.sort(valence)[-2:] == 256).all() and (valence[:-2] == 4).all()
    for mesh in ("flat", "bumpy"):
        v, t = _mesh(mesh)
        assert (v * 16 == np.round(v * 16)).all() and np.abs(v[:, 2]).max() <= 0.5       # dyadic
    assert (_mesh("flat")[0][:, 2] == 0).all() and len(np.unique(_mesh("bumpy")[0][:, 2])) > 8
    # the split of scenes._grid_mesh
    from tauray_amd import scenes
    _, idx = scenes._quad((-1, -1, 0), (2, 0, 0), (0, 2, 0), 16, 16)
    assert np.array_equal(idx.reshape(-1, 3), _mesh("flat")[1])


def test_brute_force_on_known_answers():
    P = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 2), (1, 0, 2), (0, 1, 2)], np.float32)
    tri = np.array([(0, 1, 2), (3, 4, 5)])
    rays = np.array([(0.25, 0.25, 5, 1e-4, 0, 0, -1, np.inf),       # through both: the upper one wins
                     (0.25, 0.25, 5, 1e-4, 0, 0, -1, 2.5),          # tmax in front of the upper one
                     (0.25, 0.25, 1, 1e-4, 0, 0, -1, np.inf),       # from between them
                     (0.5, 0.5, 1, 1e-4, 0, 0, -2, np.inf),         # on the hypotenuse, unnormalised direction
                     (0.75, 0.75, 1, 1e-4, 0, 0, -1, np.inf),       # past it
                     (0.25, 0.25, 1, 1e-4, 1, 0, 0, np.inf)], np.float32)      # parallel
    T, I, M = RR.brute_force(rays, P, tri)
    assert I.tolist() == [1, -1, 0, 0, -1, -1]
    assert T[[0, 2, 3]].tolist() == [3.0, 1.0, 0.5] and M[[0, 2, 3]].tolist() == [0.25, 0.25, 0.0]
    assert RR.shares_vertex(np.array([(0, 1, 2), (2, 3, 4), (5, 6, 7)]), [0, 0, 0, -1], [0, 1, 2, 0]).tolist() == [True, True, False, False]


@pytest.mark.parametrize("mesh,placement", SOLIDS + LATTICES, ids=lambda x: x)
def test_oracle_against_brute_force(oracle, cases, mesh, placement):
    """The measurement B and B_P come from: the oracle meets every condition, with half of the bound to spare."""
    case = cases(mesh, placement)
    _reference_is_sound(case)
    osc = oracle.OracleScene(case["scene"])
    for name, f in case["families"].items():
        what = f"oracle, {mesh} {placement} {name}"
        for seeds in (_seeds(len(f["rays"])), None):
            got = osc.trace_closest(f["rays"], seeds)
            terr, perr = _check_hits(case, name, got, B[mesh] / 2, B_P[mesh] / 2, what, exact=mesh in ("flat", "bumpy"))
        print(f"{what}: distance error {terr:.3e} of max(T, |origin|), hit point {perr:.3e} of the scale, "
              f"median float64 margin {np.median(f['M']):.1e}, {int((f['M'] < 1e-6).sum())} rays within 1e-6 of an edge")
        _check_shadow(case, name, osc.trace_shadow, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# on the GPU: the kernels against the brute force

@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


def _stage(R, ctx, scene, strategy):
    return R.SceneStage(ctx, scene, as_strategy=strategy, dynamic=np.ones(1, np.uint8) if strategy == STATIC_MERGED else None)


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("instance_id", "primitive_id", "bary_u", "bary_v", "t"))


def _check_stage(case, ss, strategy, what):
    """All three queries of one stage against the float64 answers of every family of the case."""
    mesh = case["mesh"]
    lattice = mesh in ("flat", "bumpy")
    for name, f in case["families"].items():
        w = f"{what}, strategy {strategy}, {name}"
        rays, seeds = f["rays"], _seeds(len(f["rays"]))
        if strategy == ALL:
            b, b_p, point_scale = B[mesh], B_P[mesh], None
        else:
            # the object-space ray is the world ray rounded at the magnitude of its origin, and the object-space triangle is the
            # world-space one to half an ulp of its world coordinates: the hit point moves by ulps of max(scale, |origin|)
            b, b_p = two_level_bounds(mesh)
            point_scale = np.maximum(case["scale"], np.abs(rays[:, :3].astype(np.float64)).max(1))
        seeded = ss.trace_closest(rays, seeds)
        for got in (seeded, ss.trace_closest(rays, None)):
            terr, perr = _check_hits(case, name, got, b, b_p, w, exact=lattice and strategy == ALL, point_scale=point_scale)
        print(f"{w}: distance error {terr:.3e} (bound {b:.1e}), hit point {perr:.3e} (bound {b_p:.1e})")
        _check_shadow(case, name, ss.trace_shadow, w)
        if strategy == ALL:
            assert _same_bits(ss.trace_terminal(rays, seeds, fallback=np.ones(len(rays), np.uint32)), seeded), f"{w}: terminal fallback"
            term = ss.trace_terminal(rays, seeds)       # no emitters: whatever a ray meets first in slot order blocks it
            assert (term["instance_id"] == HIT_BLOCKED).all(), \
                f"{w}: {int((term['instance_id'] != HIT_BLOCKED).sum())} terminal rays leak, first {np.flatnonzero(term['instance_id'] != HIT_BLOCKED)[:5]}"


def _no_stack_overflow(R, ctx, ss, scene):
    from test_gpu_parity import _render_hip
    _render_hip(R, ctx, ss, scene, (32, 32), max_bounces=2, specialize=False)       # asserts stack_overflows == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,placement", SOLIDS + LATTICES, ids=lambda x: x)
def test_queries_against_brute_force(R, ctx, cases, mesh, placement):
    """trace_closest (seeded and not), trace_shadow and, all-merged, trace_terminal (as a fallback: the closest hit's bits; otherwise
    blocked, every ray) under the three structures.  The lattices' exact rays all take the fp64 fallback of tri_intersect."""
    case = cases(mesh, placement)
    for strategy in (ALL, PER_MESH, STATIC_MERGED):
        ss = _stage(R, ctx, case["scene"], strategy)
        assert ss.layout()["strategy"] == strategy
        _check_stage(case, ss, strategy, f"{mesh} {placement}")
        _no_stack_overflow(R, ctx, ss, case["scene"])
        del ss


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,placement", SOLIDS, ids=lambda x: x)
def test_nearly_empty_waves_give_the_same_bits(R, ctx, cases, mesh, placement):
    """The first 1, 3 and 65 rays of the inside family on their own: waves that start nearly empty, so the quad-cooperative tail of
    trace_quad.h does the work.  The answers are the bits of the same rays inside the full launch."""
    case = cases(mesh, placement)
    f = case["families"]["inside"]
    rays, seeds, srays = f["rays"], _seeds(len(f["rays"])), _shadow_rays(f, 1.01)
    for strategy in (ALL, PER_MESH):
        ss = _stage(R, ctx, case["scene"], strategy)
        full, full_s = ss.trace_closest(rays, seeds), ss.trace_shadow(srays)
        for n in (1, 3, 65):
            assert _same_bits(ss.trace_closest(rays[:n], seeds[:n]), full[:n]), f"strategy {strategy}: the first {n} rays alone"
            assert np.array_equal(ss.trace_shadow(srays[:n]).view(np.uint32), full_s[:n].view(np.uint32)), f"strategy {strategy}: {n} shadow rays"
        if strategy == ALL:
            for n in (1, 3, 65):
                assert _same_bits(ss.trace_terminal(rays[:n], seeds[:n], fallback=np.ones(n, np.uint32)), full[:n])
                assert (ss.trace_terminal(rays[:n], seeds[:n])["instance_id"] == HIT_BLOCKED).all()
        del ss


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["icosphere", "bipyramid"])
def test_refit_and_fast_rebuild_hold_the_new_placement(R, ctx, cases, mesh):
    """Per-mesh: uploaded at `rotfar`, moved to `rot` by update_instances - with a refit, and with a rebuild (ePreferFastBuild).  The
    families of the new placement hold against the new world vertices."""
    old, new = cases(mesh, "rotfar"), cases(mesh, "rot")
    for refit in (True, False):
        ss = _stage(R, ctx, old["scene"], PER_MESH)
        ss.update_instances(new["scene"].instances, refit=refit)
        _check_stage(new, ss, PER_MESH, f"{mesh} rotfar -> rot, refit={refit}")
        _no_stack_overflow(R, ctx, ss, new["scene"])
        del ss


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [ALL, PER_MESH])
def test_distance_image_from_inside_the_sphere(R, ctx, cases, strategy):
    """Through a frame kernel: the camera at the centre of the unit icosphere, feature "distance" at 128 x 128.  A miss is NaN (the
    default value): every pixel is finite and lies between the sphere's inradius and 1."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    case = cases("icosphere", "unit")
    P, tri = case["P"].astype(np.float64), case["tri"]
    n = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
    inradius = float(np.abs((n * P[tri[:, 0]]).sum(1) / np.linalg.norm(n, axis=1)).min())
    assert 0.98 < inradius < 1.0
    ss = _stage(R, ctx, case["scene"], strategy)
    fs = R.FeatureStage(ctx, ss, R.FEATURE_DISTANCE, DistributionParams((128, 128), DISTRIBUTION_DUPLICATE, 0, 1, True))
    buf = ctx.alloc(128 * 128 * 16).zero()
    fs.run(buf)
    d = buf.download((128, 128, 4))[..., 0]
    assert np.isfinite(d).all(), f"strategy {strategy}: {int((~np.isfinite(d)).sum())} pixels see through the sphere"
    print(f"strategy {strategy}: distance in [{d.min():.9f}, {d.max():.9f}], inradius {inradius:.9f}")
    assert d.min() >= inradius and d.max() <= 1 + 1e-6, f"strategy {strategy}: distance in [{d.min()}, {d.max()}], inradius {inradius}"
    _no_stack_overflow(R, ctx, ss, case["scene"])
