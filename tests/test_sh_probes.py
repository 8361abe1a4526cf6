"""The SH probe-grid baking stage (trhip_sh_*, tauray_amd/csrc/sh_probes.{h,hip}): sh_path_tracer_stage + sh_compact_stage.

CPU part: the ABI, the refusals, the numpy model (tests/sh_probes_model.py) against closed forms and its float32 form against its float64
form, both glTF loaders on tests/golden/light_probe.gltf, the command line's refusals, and the grid parameters the C++ host packs
(tests/sh_probes_check.cc) against the Python host's.

GPU part, every test on a small scene of its own:
 * deterministic: an inward-facing box of 12 triangles, max_bounces = 1, no light sampling, point film, IEEE arithmetic.  The model
   intersects the box analytically.  Bound, on every entry: |stage - float64 model| <= 4 |float32 model - float64 model| + one float32 ulp
   of the entry's magnitude.  The half grid is astype(float16) of the float grid; closest_rays = probes * N, shadow_rays = 0.
 * temporal: mix ratios 1, 1/2, 0.4 against the model, reset_history, the frame counter's rotation.
 * invariance, same bits: batches of one probe / one batch; one lane / automatic; per-mesh / all-merged structure; sample-major /
   probe-major path ids (the second build of the library, libtrhip_sample_major.so, in a child process).
 * the first-bounce clamp on the bounce-0 emission and on the bounce-0 light sample: the grid does not follow an emitter above the clamp.
 * multi-bounce against the camera path: equirectangular renders from the probe positions, projected in numpy; the coefficients agree within
   Z standard errors (the multiple tests/test_estimator_consistency.py uses for its variants) plus the camera side's resolution error.
 * Vulkan-grade arithmetic against IEEE: DESIGN.md section 3's bound for that mode (1e-2 relative + 1e-2 absolute on all but 0.5 % of the
   entries, the mean within 2e-3).
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sh_probes_model as M      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "light_probe.gltf")
CLI = os.path.join(ROOT, "tauray_amd", "tauray_hip")


# =====================================================================================================================================
# CPU part
def test_symbols_resolve_and_struct_sizes():
    from tauray_amd import _lib
    L = _lib.lib()
    for name in ("create", "destroy", "set_transform", "set_frame_counter", "reset_history", "set_lanes", "set_batch_probes", "set_shading_arithmetic",
                 "render", "get_grids", "download", "get_counters", "get_timings", "get_grid_data", "pack_grid_data", "set_profiling", "reset_counters"):
        assert hasattr(L, f"trhip_sh_{name}"), name
    assert C.sizeof(_lib.ShOptionsC) == 4 + 12 + 4 + 4
    assert C.sizeof(_lib.ShGridDataC) == 64 + 64 + 12 + 4 + 12 + 4 + 4
    assert C.sizeof(_lib.ShTimingsC) == 4 + 4 + 64 + 5 * 4
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    for name in ("trhip_sh_options", "trhip_sh_grid_data", "trhip_sh_timings", "TRHIP_SH_GRID_HALF"):
        assert name in header


def _create(resolution=(2, 2, 2), dev=None, **kw):
    from tauray_amd import renderer as R
    from tauray_amd.scene import ShGrid
    return R.ShPathTracerStage(dev, None, ShGrid(resolution=resolution), kw)


@pytest.mark.parametrize("kw, resolution, text", [
    (dict(), (2, 0, 2), "zero resolution"),
    (dict(sh_order=5), (2, 2, 2), "order 5 is outside 0..4"),
    (dict(sh_order=-1), (2, 2, 2), "order -1 is outside 0..4"),
    (dict(samples_per_probe=0), (2, 2, 2), "samples_per_probe must be >= 1"),
    (dict(sampler=1), (2, 2, 2), "only sampler = 0"),
    (dict(sampler=3), (2, 2, 2), "sampler 3"),
    (dict(), (2, 2, 2), "null trhip_device (no HIP device: there is no CPU fallback)"),
])
def test_create_refusals(kw, resolution, text):
    from tauray_amd._lib import TrhipError
    with pytest.raises(TrhipError) as e:
        _create(resolution, None, **kw)
    assert text in str(e.value) and str(e.value).startswith("trhip_sh_create:")


def test_reference_defaults_of_the_host_options():
    from tauray_amd import renderer as R
    o = R.sh_options()
    assert (o["samples_per_probe"], o["film"], o["film_radius"], o["temporal_ratio"], o["indirect_clamping"], o["regularization_gamma"], o["sh_order"]) == \
        (1, R.FILM_BLACKMAN_HARRIS, 1.0, 0.02, 100.0, 1.0, 2)
    with pytest.raises(AttributeError):
        R.sh_options(samples_per_pixel=4)
    assert [R.sh_coef_count(o) for o in range(5)] == [1, 4, 9, 16, 25]


# ---- the model against closed forms
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_model_constant_radiance_gives_coefficient_zero(dt):
    """4 pi Y00^2 = 1: under constant radiance e coefficient 0 is e to float rounding, and the other coefficients are quadrature error."""
    e = np.array([0.7, 1.9, 0.05])
    for n, order in ((64, 0), (257, 2), (1000, 4)):
        g = M.grid_data(np.eye(4), (1, 1, 1), (1, 1, 1), n, 5, 1, 0.0, dt)
        ldir = M.local_dirs(np.arange(n), n, g["rotation_x"], g["rotation_y"], dt)
        coefs = M.project(np.broadcast_to(e.astype(dt), (n, 3)), np.zeros(n, dtype=dt), ldir, g, order, dt)
        eps = np.finfo(dt).eps
        y00 = 0.2820947917738781
        assert np.abs(coefs[0, :3].astype(np.float64) * y00 - e).max() <= 16 * eps * e.max()
        assert (coefs[:, 3] == 0).all()


def test_model_basis_on_the_axes():
    """sh_basis at +-x, +-y, +-z against the closed values of the real spherical harmonics."""
    k1, k2a, k2b, k2c = 0.4886025119029199, 1.0925484305920792, 0.3153915652525201, 0.5462742152960396
    for dt in (np.float32, np.float64):
        b = M.sh_basis(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=dt), 4, dt).astype(np.float64)
        want = np.zeros((6, 25))
        want[:, 0] = 0.2820947917738781
        want[:, 1], want[:, 2], want[:, 3] = [0, k1, 0, 0, -k1, 0], [0, 0, k1, 0, 0, -k1], [k1, 0, 0, -k1, 0, 0]
        want[:, 6] = [-k2b, -k2b, 2 * k2b, -k2b, -k2b, 2 * k2b]
        want[:, 8] = [k2c, -k2c, 0, k2c, -k2c, 0]
        want[:, 9], want[:, 15] = [0, -0.5900435899266435, 0, 0, 0.5900435899266435, 0], [0.5900435899266435, 0, 0, -0.5900435899266435, 0, 0]
        want[:, 11], want[:, 13] = [0, -0.4570457994644658, 0, 0, 0.4570457994644658, 0], [-0.4570457994644658, 0, 0, 0.4570457994644658, 0, 0]
        want[:, 12] = [0, 0, 2 * 0.3731763325901155, 0, 0, -2 * 0.3731763325901155]
        want[:, 20] = 0.1057855469152043 * np.array([3, 3, 8, 3, 3, 8])
        want[:, 22] = 0.4730873478787801 * np.array([-1, 1, 0, -1, 1, 0])
        want[:, 24] = 0.6258357354491763
        want[2, 24] = want[5, 24] = 0
        assert np.abs(b - want).max() <= 4 * np.finfo(dt).eps
        for order in range(5):
            assert M.sh_basis(np.zeros((1, 3), dtype=dt), order, dt).shape == (1, (order + 1) ** 2)


@pytest.mark.parametrize("n, frame", [(1, 0), (63, 1), (200, 7)])
def test_model_directions_lie_on_the_sphere_at_the_lattice_heights(n, frame):
    for dt in (np.float32, np.float64):
        g = M.grid_data(np.eye(4), (1, 1, 1), (1, 1, 1), n, frame, 1, 0.0, dt)
        d = M.local_dirs(np.arange(n), n, g["rotation_x"], g["rotation_y"], dt).astype(np.float64)
        eps = np.finfo(dt).eps
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 4 * eps
        assert np.abs(d[:, 2] - (2 * (np.arange(n) + float(g["rotation_y"])) / n - 1)).max() <= 4 * eps
        assert 0 <= g["rotation_x"] <= 1 and 0 <= g["rotation_y"] <= 1
    a, b = (M.grid_data(np.eye(4), (1, 1, 1), (1, 1, 1), n, f, 1, 0.0)["rotation_x"] for f in (frame, frame + 1))
    assert a != b


def test_model_orientation_is_the_rotation_of_the_transform():
    t = _transform()
    for dt in (np.float32, np.float64):
        r = M.matrix_orientation(t, dt).astype(np.float64)
        want = t[:3, :3] / np.linalg.norm(t[:3, :3], axis=0, keepdims=True)
        assert np.abs(r - want).max() <= 8 * np.finfo(dt).eps
    g = M.grid_data(t, SCALING, (3, 2, 1), 4, 0, 1, 0.0, np.float64)
    assert np.allclose(g["cell_scale"], 0.5 * np.array([3, 2, 1]) / np.array(SCALING, dtype=np.float32).astype(np.float64))
    assert [M.grid_data(t, SCALING, (1, 1, 1), 4, 0, h, 0.4)["mix_ratio"] for h in (1, 2, 3, 4)] == [1.0, 0.5, np.float32(0.4), np.float32(0.4)]


def test_float32_model_against_float64_model():
    box = _box_model()
    for res, n, order, film in (((3, 2, 1), 65, 4, 0), ((1, 1, 1), 200, 2, 1), ((1, 1, 1), 64, 3, 2)):
        a = M.bake(box.radiance, _transform(), SCALING, res, order, n, frame_counter=3, film=film, film_radius=0.4, dt=np.float32)
        b = M.bake(box.radiance, _transform(), SCALING, res, order, n, frame_counter=3, film=film, film_radius=0.4, dt=np.float64)
        scale = np.abs(b).max()
        err = np.abs(a.astype(np.float64) - b).max()
        print(f"\n{res} N={n} order {order} film {film}: float32 model - float64 model {err:.3e} at magnitude {scale:.3e}")
        # a term is a handful of roundings and the tree adds log2-deep: far inside 64 eps of the largest entry unless a ray changes face
        assert err <= 64 * np.finfo(np.float32).eps * scale


def test_both_loaders_read_the_light_probe_fixture(tmp_path):
    from tauray_amd.gltf import load_glb
    scene = load_glb(FIXTURE, 64, 64)
    assert len(scene.sh_grids) == 1
    g = scene.sh_grids[0]
    assert g.resolution == (3, 2, 4) and g.radius == 0.25
    want = np.array([[0, -1.5, 0, 1.0], [2.0, 0, 0, -0.5], [0, 0, 0.5, 0.25], [0, 0, 0, 1]])      # the parent's translation, rotation 90 degrees about z, |scale|
    assert np.allclose(g.transform, want, atol=1e-6), g.transform
    assert np.allclose(g.scaling, (2.0, 1.5, 0.5), atol=1e-6)
    out = subprocess.run([_check_binary(tmp_path), "gltf", FIXTURE], capture_output=True, text=True, check=True).stdout.split()
    vals = [float(v) for v in out]
    assert vals[:4] == [3, 2, 4, 0.25]
    assert np.allclose(np.array(vals[4:20]).reshape(4, 4).T, np.asarray(g.transform, dtype=np.float32), atol=1e-6)      # printed column-major
    assert np.allclose(vals[20:23], np.asarray(g.scaling, dtype=np.float32), atol=1e-6)


def _check_binary(tmp_path):
    exe = str(tmp_path / "sh_probes_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DTAURAY_HIP_WITH_ZLIB", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sh_probes_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


def test_cpp_host_packs_the_grid_parameters_of_the_python_host(tmp_path):
    """tests/sh_probes_check.cc prints what tr::sh_grid_parameters (include/tauray_hip.hh) packs for three consecutive renders: transform,
    normal transform, cell_scale, rotations, mix_ratio.  The model is the Python side (the stage itself needs a device; the GPU part compares
    the library's own packing with the model)."""
    t = _transform()
    args = [f"{v!r}" for v in np.asarray(t, dtype=np.float32).T.reshape(16).tolist()] + [repr(float(np.float32(s))) for s in SCALING]
    out = subprocess.run([_check_binary(tmp_path), "params", "3", "2", "5", "65", "7", "0.4"] + args, capture_output=True, text=True, check=True).stdout
    rows = [np.array([float.fromhex(v) for v in line.split()]) for line in out.strip().splitlines()]
    assert len(rows) == 3
    from tauray_amd import renderer as R
    from tauray_amd.scene import ShGrid
    grid = ShGrid(resolution=(3, 2, 5), transform=t, scaling=SCALING)
    for k, row in enumerate(rows):
        g = M.grid_data(t, SCALING, (3, 2, 5), 65, 7 + k, k + 1, 0.4, np.float32)
        want = np.concatenate([g["transform"].T.reshape(16), g["normal_transform"].T.reshape(9), g["cell_scale"], [g["rotation_x"], g["rotation_y"], g["mix_ratio"]]])
        assert (row.astype(np.float32) == want.astype(np.float32)).all(), (k, row, want)
        h = R.sh_grid_parameters(grid, 65, 7 + k, k + 1, 0.4)      # the Python host
        python = np.concatenate([h["transform"].T.reshape(16), h["normal_transform"][:3, :3].T.reshape(9), h["cell_scale"], [h["rotation_x"], h["rotation_y"], h["mix_ratio"]]])
        assert (python.astype(np.float32) == row.astype(np.float32)).all(), (k, row, python)
        assert h["grid_size"] == (3, 2, 5)


@pytest.mark.parametrize("args, text", [
    (["--renderer=sh-probes", os.path.join(GOLDEN, "animated.glb")], "has no light-probe grid"),
    (["--renderer=sh-probes", "--denoiser=bmfr", FIXTURE], "--renderer=sh-probes bakes probe grids: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=sh-probes", "--taa=4", FIXTURE], "--renderer=sh-probes bakes probe grids: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=sh-probes", "--temporal-reprojection=0.5", FIXTURE], "--renderer=sh-probes bakes probe grids: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=sh-probes", "--devices=0,1", FIXTURE], "--renderer=sh-probes runs on one device"),
    (["--renderer=sh-probes", "--sh-order=5", FIXTURE], "--sh-order"),
    (["--renderer=sh-probes", "--samples-per-probe=0", FIXTURE], "--samples-per-probe"),
])
def test_cli_refusals(args, text):
    r = subprocess.run([CLI, "--headless=/tmp/unused_sh_probes", "--frames=1"] + args, capture_output=True, text=True)
    assert r.returncode != 0
    assert text in r.stderr, r.stderr


# =====================================================================================================================================
# the scenes of the GPU part (and of the model tests above)
SCALING = (0.9, 0.6, 0.4)
BOX_LO, BOX_HI = (-2.0, -1.5, -1.0), (2.0, 1.5, 1.25)
CLAMP = 2.0
# per face (-x, +x, -y, +y, -z, +z): emission, albedo, metallic; +x is metallic 1, -y's emission is above the clamp
FACE_EMISSION = [(0.5, 0.25, 0.125), (1.0, 0.75, 0.5), (5.0, 4.0, 3.0), (0.0, 0.0, 0.0), (0.3, 0.9, 0.1), (0.8, 0.1, 1.4)]
FACE_ALBEDO = [(0.8, 0.7, 0.6), (0.9, 0.5, 0.3), (0.4, 0.4, 0.9), (0.6, 0.6, 0.6), (0.2, 0.7, 0.3), (1.0, 0.9, 0.8)]
FACE_METALLIC = [0.0, 1.0, 0.25, 0.5, 0.75, 0.125]


def _transform():
    """Rotated about a skew axis and scaled non-uniformly; its box lies inside the scene's."""
    from tauray_amd.scene import trs_matrix
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    a = math.radians(37.0)
    q = tuple(axis * math.sin(a / 2)) + (math.cos(a / 2),)
    return trs_matrix((0.2, -0.1, 0.05), q, SCALING)


def _box_model(clamp=CLAMP):
    return M.BoxScene(BOX_LO, BOX_HI, FACE_EMISSION, FACE_ALBEDO, FACE_METALLIC, clamp)


def _box_scene(emission=FACE_EMISSION, albedo=FACE_ALBEDO, metallic=FACE_METALLIC, cameras=()):
    """Six instances with the identity transform, one per face, two inward-facing triangles each."""
    from tauray_amd import scene as S
    lo, hi = np.array(BOX_LO), np.array(BOX_HI)
    insts, verts, spans, idx = [], [], [], []
    for f in range(6):
        axis, side = f // 2, f % 2
        u, w = (axis + 1) % 3, (axis + 2) % 3
        p0 = lo.copy()
        p0[axis] = hi[axis] if side else lo[axis]
        eu, ew = np.zeros(3), np.zeros(3)
        eu[u], ew[w] = hi[u] - lo[u], hi[w] - lo[w]
        if not side:
            eu, ew = ew, eu      # ew x eu, the triangles' normal, points along -axis on the hi side and +axis on the lo side: inward
        n = np.cross(ew, eu)
        v = np.zeros(4, dtype=S.VERTEX)
        v["pos"] = [p0, p0 + ew, p0 + ew + eu, p0 + eu]
        v["normal"] = n / np.linalg.norm(n)
        v["tangent"] = tuple(ew / np.linalg.norm(ew)) + (1.0,)
        v["uv"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
        assert (n[axis] < 0) == bool(side)
        spans.append((4 * f, 4, 6 * f, 2))
        insts.append(S.make_instance(np.eye(4), S.make_material(albedo=tuple(albedo[f]) + (1.0,), metallic=metallic[f], roughness=0.6,
                                                                emission=emission[f], double_sided=True)))
        verts.append(v)
        idx += [0, 1, 2, 0, 2, 3]
    return S.SceneDesc(instances=np.concatenate(insts), spans=np.array(spans, dtype=S.MESH_SPAN), vertices=np.concatenate(verts),
                       indices=np.array(idx, dtype=np.uint32), cameras=list(cameras), name="sh_box").finalize(True)


def _grid(resolution):
    from tauray_amd.scene import ShGrid
    return ShGrid(resolution=tuple(resolution), radius=0.0, transform=_transform(), scaling=SCALING)


DETERMINISTIC = dict(max_bounces=1, nee_point=0.0, nee_directional=0.0, nee_envmap=0.0, nee_triangles=0.0, film=0, indirect_clamping=CLAMP,
                     regularization_gamma=0.0, temporal_ratio=0.0)


# =====================================================================================================================================
# GPU part
@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


@pytest.fixture(scope="module")
def box_stage(R, ctx):
    return R.SceneStage(ctx, _box_scene())


def _stage(R, ctx, ss, resolution, n, order, ieee=True, **kw):
    st = R.ShPathTracerStage(ctx, ss, _grid(resolution), dict(DETERMINISTIC, samples_per_probe=n, sh_order=order, **kw))
    st.set_shading_arithmetic(ieee)
    return st


_MODEL_CACHE = {}


def _models(resolution, n, order, frame, history=1, ratio=0.0, previous=(None, None)):
    key = (tuple(resolution), n, order, frame, history, ratio, id(previous[0]))
    if key not in _MODEL_CACHE:
        box = _box_model()
        _MODEL_CACHE[key] = tuple(M.bake(box.radiance, _transform(), SCALING, resolution, order, n, frame_counter=frame, history_length=history,
                                         temporal_ratio=ratio, previous=previous[i], dt=dt) for i, dt in enumerate((np.float32, np.float64)))
    return _MODEL_CACHE[key]


def _check_against_models(got, m32, m64, what):
    """On every entry: |stage - float64 model| <= 4 |float32 model - float64 model| + one float32 ulp of the entry's magnitude."""
    own = np.abs(m32.astype(np.float64) - m64)
    dev = np.abs(got.astype(np.float64) - m64)
    ulp = np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64)
    slack = dev - (4 * own + ulp)
    worst = np.unravel_index(np.argmax(slack), slack.shape)
    same = float((got == m32).mean())
    print(f"\n{what}: stage - float64 model max {dev.max():.3e}, float32 model - float64 model max {own.max():.3e}, "
          f"{same:.1%} of the entries are the float32 model's bits; rgb {float((got[..., :3] == m32[..., :3]).mean()):.1%}; "
          f"worst entry {worst}: stage off by {dev[worst]:.3e}, float32 model by {own[worst]:.3e}, ulp {ulp[worst]:.3e}")
    assert np.isfinite(got).all()
    assert (slack <= 0).all(), f"{what}: {int((slack > 0).sum())} of {slack.size} entries outside the bound; worst {worst}: {dev[worst]:.3e} > 4 * {own[worst]:.3e} + {ulp[worst]:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("resolution, n, order", [((1, 1, 1), 1, 0), ((1, 1, 1), 63, 1), ((3, 2, 1), 64, 2), ((3, 2, 1), 65, 4), ((2, 3, 5), 200, 3)])
def test_deterministic_box_against_the_model(R, ctx, box_stage, resolution, n, order):
    st = _stage(R, ctx, box_stage, resolution, n, order)
    st.set_frame_counter(3)
    gd = st.grid_data()
    st.run()
    got, half = st.download("grid"), st.download("half")
    counters = st.counters()
    timings = st.timings()
    st.close()
    g = M.grid_data(_transform(), SCALING, resolution, n, 3, 1, 0.0)
    assert (gd["normal_transform"][:3, :3] == g["normal_transform"]).all() and (gd["cell_scale"] == g["cell_scale"]).all()
    assert (gd["rotation_x"], gd["rotation_y"], gd["mix_ratio"]) == (g["rotation_x"], g["rotation_y"], 1.0)
    m32, m64 = _models(resolution, n, order, 3)
    assert got.shape == m32.shape == (resolution[2], resolution[1] * (order + 1) ** 2, resolution[0], 4)
    _check_against_models(got, m32, m64, f"{resolution} N={n} order {order}")
    assert (half.view(np.uint16) == got.astype(np.float16).view(np.uint16)).all()
    probes = resolution[0] * resolution[1] * resolution[2]
    assert counters["closest_rays"] == probes * n and counters["shadow_rays"] == 0 and counters["stack_overflows"] == 0
    assert timings["name"] == "SH path tracing" and timings["frames"] == 1 and timings["total_ms"] > 0


@pytest.mark.gpu
def test_temporal_blend_reset_and_frame_counter(R, ctx, box_stage):
    res, n, order = (3, 2, 1), 65, 2
    st = _stage(R, ctx, box_stage, res, n, order, temporal_ratio=0.4)
    st.set_frame_counter(10)
    prev = (None, None)
    for k, ratio in enumerate((1.0, 0.5, np.float32(0.4))):
        assert st.grid_data()["mix_ratio"] == ratio
        st.run()
        got = st.download("grid")
        m = _models(res, n, order, 10 + k, k + 1, 0.4, prev)
        _check_against_models(got, m[0], m[1], f"render {k + 1}, mix ratio {ratio}")
        prev = m
    st.reset_history()
    assert st.grid_data()["mix_ratio"] == 1.0
    st.set_frame_counter(3)
    st.run()
    again = st.download("grid")
    m32, m64 = _models(res, n, order, 3)
    _check_against_models(again, m32, m64, "after reset_history, frame 3")
    first = _models(res, n, order, 10)[0]
    assert (again != first).any()      # another frame counter, another rotation of the lattice
    st.close()


def _bake_once(R, ctx, ss, resolution, n, order, lanes=None, batch=None, **kw):
    st = _stage(R, ctx, ss, resolution, n, order, **kw)
    if lanes is not None:
        st.set_lanes(lanes)
    if batch is not None:
        st.set_batch_probes(batch)
    st.set_frame_counter(2)
    st.run()
    out = st.download("grid"), st.download("half"), st.counters()
    st.close()
    return out


@pytest.mark.gpu
def test_grids_do_not_depend_on_the_batches(R, ctx, box_stage):
    multi = dict(max_bounces=3, nee_triangles=1.0, film=1, film_radius=0.5)
    a = _bake_once(R, ctx, box_stage, (2, 3, 5), 65, 4, batch=1, **multi)
    b = _bake_once(R, ctx, box_stage, (2, 3, 5), 65, 4, **multi)
    c = _bake_once(R, ctx, box_stage, (2, 3, 5), 65, 4, batch=7, **multi)
    assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1].view(np.uint16) == b[1].view(np.uint16)).all()
    assert (c[0].view(np.uint32) == b[0].view(np.uint32)).all()
    assert a[2]["closest_rays"] == b[2]["closest_rays"] and a[2]["shadow_rays"] == b[2]["shadow_rays"] > 0


@pytest.mark.gpu
def test_grids_do_not_depend_on_the_lanes(R, ctx, box_stage):
    """4 x 4 x 4 probes of 4096 samples are 262 144 paths: the automatic schedule runs four lanes."""
    multi = dict(max_bounces=2, nee_triangles=1.0)
    a = _bake_once(R, ctx, box_stage, (4, 4, 4), 4096, 1, lanes=1, **multi)
    b = _bake_once(R, ctx, box_stage, (4, 4, 4), 4096, 1, **multi)
    assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all()
    assert a[2]["closest_rays"] == b[2]["closest_rays"] and a[2]["shadow_rays"] == b[2]["shadow_rays"]


@pytest.mark.gpu
def test_grids_do_not_depend_on_the_acceleration_structure(R, ctx):
    from tauray_amd import _lib
    multi = dict(max_bounces=3, nee_triangles=1.0)
    out = []
    for strategy in (_lib.AS_ALL_MERGED, _lib.AS_PER_MESH):
        ss = R.SceneStage(ctx, _box_scene(), as_strategy=strategy)
        out.append(_bake_once(R, ctx, ss, (3, 2, 1), 200, 2, **multi))
    R.SceneStage(ctx, _box_scene())      # the module's scene again (all-merged)
    assert (out[0][0].view(np.uint32) == out[1][0].view(np.uint32)).all()


@pytest.mark.gpu
def test_first_bounce_clamp_bounds_emission_and_light_samples(R, ctx):
    """INDIRECT_CLAMP_FIRST_BOUNCE, both halves.  One face emits far above the clamp, the walls are diffuse, max_bounces = 2 with light
    sampling: a sample's light is the bounce-0 emission (rays that hit the emitter), the bounce-0 light sample (rays that hit a wall) and
    the bounce-1 emission, and each is cut to the clamp's luminance in the emitter's colour.  So the grid does not depend on how bright the
    emitter is: twice the emission (a power of two: the same r9g9b9e5 mantissas) gives the same grid up to rounding and the handful of
    bounce-1 hits whose MIS weight brings them under the clamp.  Without either first-bounce clamp the grid doubles with the emission."""
    grids = []
    for scale in (1.0, 2.0):
        emission = [(0.0, 0.0, 0.0)] * 6
        emission[3] = (8192.0 * scale, 4096.0 * scale, 2048.0 * scale)
        ss = R.SceneStage(ctx, _box_scene(emission, [(0.75, 0.5, 0.25)] * 6, [0.0] * 6))
        st = R.ShPathTracerStage(ctx, ss, _grid((2, 1, 2)), dict(DETERMINISTIC, max_bounces=2, nee_triangles=1.0, indirect_clamping=0.5,
                                                                  samples_per_probe=2048, sh_order=1))
        st.set_shading_arithmetic(True)
        st.run()
        grids.append(st.download("grid").astype(np.float64))
        assert st.counters()["shadow_rays"] > 0
        st.close()
    R.SceneStage(ctx, _box_scene())      # the module's scene again
    a, b = grids
    top = np.abs(a[..., :3]).max()
    diff = np.abs(a - b)[..., :3].max()
    print(f"\nemission x 1 against x 2 under the clamp: largest entry {top:.4f}, largest difference {diff:.3e}")
    # every sample's three contributions have luminance <= 0.5 before the lobe weights: coefficient 0 stays O(clamp), far below the emission
    assert 0.05 < top < 16.0
    assert diff <= 2e-3 * top
    assert (a[..., 3] == b[..., 3]).all()      # the distance channel does not see the emission


def _hash_in_child(lib, resolution, n, order, options):
    """sha256 of the float grid and of the half grid, baked by a fresh process that loads `lib` (another build of the library)."""
    code = (
        "import hashlib, sys\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); sys.path.insert(0, {ROOT!r})\n"
        "import test_sh_probes as T\n"
        "from tauray_amd import renderer as R\n"
        "ctx = R.Context(0); ss = R.SceneStage(ctx, T._box_scene())\n"
        f"g = T._bake_once(R, ctx, ss, {tuple(resolution)!r}, {n}, {order}, **{options!r})\n"
        "print('HASH', hashlib.sha256(g[0].tobytes()).hexdigest(), hashlib.sha256(g[1].tobytes()).hexdigest())\n")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TRHIP_LIB=lib), capture_output=True, text=True, check=True).stdout
    return [line.split()[1:] for line in out.splitlines() if line.startswith("HASH")][0]


@pytest.mark.gpu
def test_grids_do_not_depend_on_the_path_id_order(R, ctx, box_stage):
    """The library's build is probe-major (TR_SH_SAMPLE_MAJOR = 0); the Makefile also links libtrhip_sample_major.so, the same objects with
    sh_probes.hip compiled sample-major.  A child process bakes with it: the same bits, in several batches (the ids of a batch are what
    differs) and in one."""
    import hashlib
    lib = os.path.join(ROOT, "tauray_amd", "libtrhip_sample_major.so")
    assert os.path.exists(lib), "tauray_amd/csrc/Makefile builds it next to libtrhip.so"
    from tauray_amd import _lib
    assert os.path.realpath(_lib.LIB_PATH) != os.path.realpath(lib)
    multi = dict(max_bounces=3, nee_triangles=1.0, film=2, film_radius=0.5)
    for batch in (None, 7):
        options = dict(multi, batch=batch)
        here = _bake_once(R, ctx, box_stage, (2, 3, 5), 65, 4, **options)
        want = [hashlib.sha256(here[0].tobytes()).hexdigest(), hashlib.sha256(here[1].tobytes()).hexdigest()]
        assert _hash_in_child(lib, (2, 3, 5), 65, 4, options) == want, f"batch {batch}"


@pytest.mark.gpu
def test_render_and_transform_refusals(R):
    """The refusals that need a stage, and a stage needs a device: rendering without a scene and without an acceleration structure, a
    transform that is not finite, more probes per batch than a batch holds."""
    from tauray_amd import _lib
    from tauray_amd._lib import TrhipError
    fresh = R.Context(0)
    st = R.ShPathTracerStage(fresh, None, _grid((1, 1, 1)), dict(DETERMINISTIC))
    with pytest.raises(TrhipError, match="no scene"):
        st.run()
    ss = R.SceneStage(fresh, _box_scene())
    st.run()
    inst = np.ascontiguousarray(ss.scene.instances)
    _lib.check(_lib.lib().trhip_scene_update_instances(fresh.h, inst.ctypes.data, len(inst)))      # invalidates the structure
    with pytest.raises(TrhipError, match="no acceleration structure: call trhip_scene_build_accel first"):
        st.run()
    bad = _transform()
    bad[1, 2] = np.inf
    with pytest.raises(TrhipError, match="the transform is not finite"):
        st.set_transform(bad, SCALING)
    with pytest.raises(TrhipError, match="more than the"):
        R.ShPathTracerStage(fresh, None, _grid((1, 1, 1)), dict(DETERMINISTIC, samples_per_probe=1 << 20)).set_batch_probes(2)
    st.close()
    fresh.close()


@pytest.mark.gpu
def test_vulkan_grade_arithmetic_against_ieee(R, ctx, box_stage):
    """at the default arithmetic an entry is within 1e-2 relative + 1e-2 absolute of the IEEE one on all but 0.5 % of the
    entries, and the mean within 2e-3."""
    for res, n, order in (((3, 2, 1), 65, 4), ((2, 3, 5), 200, 3)):
        ieee = _bake_once(R, ctx, box_stage, res, n, order, ieee=True)[0].astype(np.float64)
        fast = _bake_once(R, ctx, box_stage, res, n, order, ieee=False)[0].astype(np.float64)
        out = np.abs(fast - ieee) > 1e-2 * np.abs(ieee) + 1e-2
        mean = abs(fast.mean() - ieee.mean()) / abs(ieee.mean())
        print(f"\n{res} N={n} order {order}: {out.mean():.3%} of the entries outside 1e-2 + 1e-2, largest difference {np.abs(fast - ieee).max():.3e}, mean off by {mean:.3e}")
        assert out.mean() <= 0.005 and mean <= 2e-3


@pytest.mark.gpu
def test_cli_bakes_the_grids_of_the_python_host(R, ctx, tmp_path):
    """tauray_hip --renderer=sh-probes on the reference's test scene (one 4 x 4 x 4 grid): two frames, the second blended into the first, are
    the bits of the Python host with the same options."""
    from tauray_amd.gltf import load_glb
    glb = os.path.join(GOLDEN, "test.glb")
    prefix = str(tmp_path / "probe")
    subprocess.run([CLI, glb, "--renderer=sh-probes", "--samples-per-probe=65", "--sh-order=3", "--dshgi-temporal-ratio=0.25", "--max-ray-depth=3", "--frames=2",
                    "--filetype=raw", "--headless=" + prefix], check=True, capture_output=True, text=True)
    scene = load_glb(glb, 1280, 720)
    assert len(scene.sh_grids) == 1
    ss = R.SceneStage(ctx, scene)
    w = R.options_for_scene(scene)
    st = R.ShPathTracerStage(ctx, ss, scene.sh_grids[0], dict(
        max_bounces=3, samples_per_probe=65, sh_order=3, temporal_ratio=0.25, film=R.FILM_POINT, film_radius=0.5, indirect_clamping=0.0,
        regularization_gamma=0.0, nee_point=w.nee_point, nee_directional=w.nee_directional, nee_envmap=w.nee_envmap, nee_triangles=w.nee_triangles))
    for f in range(2):
        st.run()
        want = st.download("grid")
        got = np.fromfile(f"{prefix}_grid0{f}.raw", dtype=np.float32).reshape(want.shape)
        assert np.isfinite(want).all() and np.abs(want[..., :3]).max() > 0
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), f"frame {f}"
    st.close()
    R.SceneStage(ctx, _box_scene())      # the module's scene again


# ---- multi-bounce, against the camera path
Z_SE = 4.0      # tests/test_estimator_consistency.py: _assert_same_mean(z_image = 4.0)


def _probe_positions(resolution):
    g = M.grid_data(_transform(), SCALING, resolution, 1, 0, 1, 0.0, np.float64)
    pos = []
    for z in range(resolution[2]):
        for y in range(resolution[1]):
            for x in range(resolution[0]):
                pos.append(M.probe_rays(g, (x, y, z), 1, dt=np.float64)[0][0])
    return np.array(pos)


def _camera_projection(R, ctx, ss, scene, size, spp, seeds, order, options):
    """Per seed and camera: sum over the pixels of modulate_color(albedo, metallic, diffuse, reflection) * sh_basis(grid-space direction of the
    pixel centre) * cos(latitude) * pixel area -> [seeds, cameras, C, 3]."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    w, h = size
    n_cam = len(scene.cameras)
    lon = ((np.arange(w) + 0.5) / w * 2 - 1) * math.pi
    lat = ((h - (np.arange(h) + 0.5)) / h * 2 - 1) * (math.pi / 2)
    lon, lat = np.meshgrid(lon, lat, indexing="xy")
    world = np.stack([np.sin(lon) * np.cos(lat), np.sin(lat), -np.cos(lon) * np.cos(lat)], axis=-1)      # the cameras have identity rotation
    rot = _transform()[:3, :3] / np.linalg.norm(_transform()[:3, :3], axis=0, keepdims=True)
    basis = M.sh_basis(world @ rot, order, np.float64)      # grid space: R^T d
    weight = np.cos(lat) * (2 * math.pi / w) * (math.pi / h)
    out = np.zeros((len(seeds), n_cam, (order + 1) ** 2, 3))
    names = ("diffuse", "reflection", "albedo", "material")
    targets = {k: ctx.alloc(n_cam * w * h * 16).zero() for k in names}
    for si, seed in enumerate(seeds):
        pt = R.PathTracerStage(ctx, ss, R.make_options(samples_per_pixel=spp, samples_per_pass=1, projection=2, hide_lights=1, film=R.FILM_BOX,
                                                       film_radius=0.5, rng_seed=seed, **options),
                               DistributionParams((w, h), DISTRIBUTION_DUPLICATE, 0, 1, True))
        pt.run_targets(targets, viewports=n_cam)
        img = {k: targets[k].download((n_cam, h, w, 4)).astype(np.float64) for k in names}
        pt.close()
        value = M.modulate_color(img["albedo"][..., :3], img["material"][..., 0], img["diffuse"][..., :3], img["reflection"][..., :3], np.float64)
        out[si] = np.einsum("chwk,hwl,hw->clk", value, basis, weight)
    for t in targets.values():
        t.free()
    return out


@pytest.mark.gpu
def test_multi_bounce_against_the_camera_path(R, ctx):
    """Diffuse walls of one albedo, one emissive face, light sampling on, four bounces, no clamp, no regularisation; 2 x 2 x 2 probes."""
    from tauray_amd import scene as S
    res, order, n = (2, 2, 2), 2, 16384
    albedo = [(0.7, 0.6, 0.5)] * 6
    emission = [(0, 0, 0)] * 6
    emission[3] = (4.0, 3.0, 2.0)
    cams = []
    for p in _probe_positions(res):
        c = S.Camera(projection=S.PROJ_EQUIRECTANGULAR)
        m = np.eye(4)
        m[:3, 3] = p
        c.transform = m
        cams.append(c)
    scene = _box_scene(emission, albedo, [0.0] * 6, cams)
    ss = R.SceneStage(ctx, scene)
    path = dict(max_bounces=4, indirect_clamping=0.0, regularization_gamma=0.0, nee_point=0.0, nee_directional=0.0, nee_envmap=0.0, nee_triangles=1.0)
    seeds = (11, 12, 13, 14, 15, 16)
    probe = np.zeros((len(seeds), 8, (order + 1) ** 2, 3))
    for si, seed in enumerate(seeds):
        st = R.ShPathTracerStage(ctx, ss, _grid(res), dict(path, samples_per_probe=n, sh_order=order, film=0, temporal_ratio=0.0, rng_seed=seed))
        st.set_frame_counter(seed)
        st.run()
        g = st.download("grid").astype(np.float64).reshape(res[2], (order + 1) ** 2, res[1], res[0], 4)      # [z][l][y][x]
        st.close()
        probe[si] = g.transpose(0, 2, 3, 1, 4).reshape(8, (order + 1) ** 2, 4)[..., :3]
    # equal total samples at both resolutions: 128 x 64 x 8 spp = 256 x 128 x 2 spp
    fine = _camera_projection(R, ctx, ss, scene, (256, 128), 2, seeds, order, path)
    coarse = _camera_projection(R, ctx, ss, scene, (128, 64), 8, seeds, order, path)
    R.SceneStage(ctx, _box_scene())      # the module's scene again
    k = len(seeds)
    resolution_error = np.abs(fine.mean(0) - coarse.mean(0))
    se = np.sqrt(probe.var(0, ddof=1) / k + fine.var(0, ddof=1) / k)
    diff = np.abs(probe.mean(0) - fine.mean(0))
    z = diff / np.maximum(se, 1e-30)
    print(f"\ncoefficient 0 of probe 0: probes {probe.mean(0)[0, 0]}, cameras {fine.mean(0)[0, 0]}; largest difference {diff.max():.3e} "
          f"({z.max():.2f} standard errors before the resolution error, which is at most {resolution_error.max():.3e}); "
          f"largest excess {(diff - Z_SE * se - resolution_error).max():.3e}")
    assert np.abs(fine.mean(0)[:, 0]).min() > 0.1      # the cameras see light
    assert (diff <= Z_SE * se + resolution_error).all()
