"""The DDISH-GI renderer: direct light plus indirect light looked up in the baked SH probe grids (tauray_amd/csrc/dshgi.hip, trhip_dshgi_*,
DESIGN.md section 20).

CPU part: the C ABI's symbols, struct sizes and refusals, the numpy model's closed forms (tests/dshgi_model.py, written from the rule in
csrc/dshgi.h), float32 model against float64 model, the rule that picks an instance's grid against trhip_dshgi_pick_grid and in both
hosts, the command line's refusals.

GPU part, images of 13 x 7 (one ragged tile) and 37 x 19 (several tiles, ragged on both edges), two viewports each:
 * closed form: a constant-radiance grid and a constant table; every hit pixel equals brdf_indirect of the downloaded surface record.
 * model: random half grids, a rotated and non-uniformly scaled grid that leaves part of the box outside, a random table.  Bound, on every
   pixel: |stage - float64 model| <= 4 |float32 model - float64 model| + one float32 ulp of the value's magnitude (section 19's bound).
 * the surface record against trhip_feature_render bit for bit; miss pixels; out = direct + indirect bit for bit, aliased and without direct;
   the same bits for both acceleration-structure layouts and for two runs; two grids and the pick; the generated table against the model's
   and against the reference's file; the whole renderer in both hosts; the image mean against the path tracer's.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dshgi_model as M      # noqa: E402
from test_sh_probes import BOX_HI, BOX_LO, SCALING, _box_scene, _transform      # noqa: E402  the SH tests' inward-facing box, one material per face

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "light_probe.gltf")
TABLE_FIXTURE = os.path.join(GOLDEN, "brdf_integration.exr")
CLI = os.path.join(ROOT, "tauray_amd", "tauray_hip")
Y00 = 0.2820947917738781
SIZES = ((13, 7), (37, 19))


# =====================================================================================================================================
# CPU part
def test_symbols_resolve_and_struct_sizes():
    from tauray_amd import _lib
    L = _lib.lib()
    for name in ("create", "destroy", "set_grids", "set_instance_grids", "set_brdf_integration", "render", "get_timings", "download", "pick_grid"):
        assert hasattr(L, f"trhip_dshgi_{name}"), name
    assert hasattr(L, "trhip_brdf_integration_generate")
    assert C.sizeof(_lib.DshgiOptionsC) == 12
    assert C.sizeof(_lib.DshgiGridC) == 8 + 12 + 64 + 12
    assert C.sizeof(_lib.DshgiTimingsC) == 4 + 4 + 64
    assert np.dtype(_lib.DSHGI_SURFACE_DTYPE).itemsize == 16 * 4 + 4 * 4 + 2 * 4
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    for name in ("trhip_dshgi_options", "trhip_dshgi_grid", "trhip_dshgi_surface", "trhip_dshgi_timings", "TRHIP_DSHGI_INDIRECT", "TRHIP_DSHGI_SURFACE"):
        assert name in header


@pytest.mark.parametrize("kw, size, layers, text", [
    (dict(), (8, 8), 1, "null trhip_device (no HIP device: there is no CPU fallback)"),
    (dict(order=5), (8, 8), 1, "order 5 is outside 0..4"),
    (dict(order=-1), (8, 8), 1, "order -1 is outside 0..4"),
    (dict(), (0, 8), 1, "zero width, height or layer count"),
    (dict(), (8, 0), 1, "zero width, height or layer count"),
    (dict(), (8, 8), 0, "zero width, height or layer count"),
])
def test_create_refusals(kw, size, layers, text):
    from tauray_amd import renderer as R
    from tauray_amd._lib import TrhipError
    with pytest.raises(TrhipError) as e:
        R.DshgiStage(None, None, size, layers, **kw)
    assert text in str(e.value) and str(e.value).startswith("trhip_dshgi_create:")


def test_generator_refuses_a_null_device():
    from tauray_amd import _lib
    assert _lib.lib().trhip_brdf_integration_generate(None, 16, 16, None, None) != 0
    assert "trhip_brdf_integration_generate: null trhip_device" in _lib.lib().trhip_last_error().decode()


def _constant_grid(resolution, order, value, w=6.0):
    """Only coef[0] is not zero: rgb = value, .w = w (a visibility of w * Y00 = 1.69, above sqrt(3) - 0.4)."""
    rx, ry, rz = resolution
    c = (order + 1) ** 2
    g = np.zeros((rz, ry * c, rx, 4), dtype=np.float16)
    g[:, :ry, :, :3] = value
    g[:, :ry, :, 3] = w
    return g


def _random_surface(rng, n, lo=BOX_LO, hi=BOX_HI):
    from tauray_amd import _lib
    s = np.zeros(n, dtype=np.dtype(_lib.DSHGI_SURFACE_DTYPE))
    s["pos"] = rng.uniform(lo, hi, (n, 3))
    for name in ("smooth_normal", "mapped_normal", "view"):
        v = rng.normal(size=(n, 3))
        s[name] = v / np.linalg.norm(v, axis=1, keepdims=True)
    s["albedo"] = rng.uniform(0.1, 1.0, (n, 4))
    s["metallic"], s["roughness"] = rng.uniform(0, 1, n), rng.uniform(0.01, 1, n)
    s["f0"], s["transmittance"] = 0.04, rng.uniform(0, 0.5, n)
    s["grid"], s["instance_id"] = 0, 0
    return s


@pytest.mark.parametrize("visibility", [False, True])
@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_model_constant_radiance_grid_gives_that_radiance(order, visibility):
    """coef[0] = L / Y00 and nothing else: both lobes have coefficient 0 equal to Y00, so incoming_diffuse = incoming_reflection = L whatever the
    order, normal and roughness - wherever a corner has weight.  Under probe visibility a point that is projected exactly onto a probe has
    none (in a (1, 1, 1) grid every point): the probe is 0 there."""
    rng = np.random.default_rng(order)
    value = np.array([1.5, 0.75, 0.25])      # exact halfs
    for dt in (np.float32, np.float64):
        for res in ((1, 1, 1), (2, 3, 5)):
            grid = M.Grid(_constant_grid(res, order, value), res, _transform(), order)
            s = _random_surface(rng, 64)
            pfw, nfw = M.affine_inverse(grid.transform, dt), M.normal_from_world(grid.transform, dt)
            sp = M._point(pfw, s["pos"].astype(dt))
            sn = M._normalize(M._mul3(nfw, s["smooth_normal"].astype(dt)))
            d = M._normalize(M._mul3(nfw, s["mapped_normal"].astype(dt)))
            cosine, ggx = M.cosine_lobe(d, order, dt), M.ggx_lobe(d, np.sqrt(s["roughness"].astype(dt)), order, dt)
            inc_d, inc_r = M.incoming_light(grid, sp, sn, cosine, ggx, visibility, dt)
            want = np.broadcast_to(value * Y00, inc_d.shape)
            if visibility:      # a point projected onto a probe (outside the grid on every axis it has several probes on) has no corner with weight
                lit = M.visibility_cell(grid, sp, sn, dt)[3] > 0
                assert lit.any() == (res != (1, 1, 1))
                want = want * lit[:, None]
            assert np.isfinite(inc_d).all() and np.isfinite(inc_r).all()
            # eight products and seven sums of the weights, one product with the lobe: far inside 32 eps
            assert np.abs(inc_d - want).max() <= 32 * np.finfo(dt).eps * 1.5, (dt, res)
            assert np.abs(inc_r - want).max() <= 32 * np.finfo(dt).eps * 1.5, (dt, res)


def test_model_trilinear_weights():
    rng = np.random.default_rng(7)
    for res in ((1, 1, 1), (3, 2, 1), (2, 3, 5), (1, 4, 1)):
        grid = M.Grid(_constant_grid(res, 0, 1.0), res, np.eye(4), 0)
        pos = rng.uniform(-1.5, 1.5, (500, 3)).astype(np.float32)
        pos[:8] = [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]      # the box's corners
        for dt in (np.float32, np.float64):
            lo, hi, w = M.trilinear_cell(grid, pos.astype(dt), dt)
            assert np.abs(w.sum(-1) - 1).max() <= 8 * np.finfo(dt).eps
            assert (lo >= 0).all() and (hi < np.array(res)).all() and (hi - lo <= 1).all() and (hi >= lo).all()
            for a in range(3):
                if res[a] == 1:
                    assert (lo[:, a] == 0).all() and (hi[:, a] == 0).all()


def test_model_visibility_corner_cases():
    """A point exactly on a probe: that corner's sample_dir is 0 / 0, both factors clamp to 0, its weight is 0.  All weights 0: a zero probe."""
    for dt in (np.float32, np.float64):
        res = (2, 3, 5)
        grid = M.Grid(_constant_grid(res, 1, 1.0), res, np.eye(4), 1)
        normal = np.array([[1.0, 0.0, 0.0]], dtype=dt)
        pos = np.array([[0.5, -1.0, 0.0]], dtype=dt)      # voxel = (1, -0.5 -> 0, 2): exactly on probe (1, 0, 2)
        lo, hi, w, inv = M.visibility_cell(grid, pos, normal, dt)
        assert tuple(lo[0]) == (1, 0, 2) and np.isfinite(w).all() and np.isfinite(inv).all()
        # corner 0 is the probe itself: 0 / 0, both factors clamp to 0; every other corner has a zero fraction on some axis
        assert (w[0] == 0).all() and inv[0] == 0
        pos = np.array([[0.5, -1.0, 0.1]], dtype=dt)      # voxel.z = 2.25: between two probes of the column through (1, 0)
        lo, hi, w, inv = M.visibility_cell(grid, pos, normal, dt)
        assert w[0, 0] > 0 and w[0, 4] > 0 and (w[0, [1, 2, 3, 5, 6, 7]] == 0).all() and inv[0] > 0
        one = M.Grid(_constant_grid((1, 1, 1), 1, 1.0), (1, 1, 1), np.eye(4), 1)
        lo, hi, w, inv = M.visibility_cell(one, np.array([[0.3, -0.2, 0.9]], dtype=dt), normal, dt)
        assert (w == 0).all() and inv[0] == 0
        lobes = np.ones((1, 4), dtype=dt)
        d, r = M.incoming_light(one, np.array([[0.3, -0.2, 0.9]], dtype=dt), normal, lobes, lobes, True, dt)
        assert (d == 0).all() and (r == 0).all()


def _random_grid(rng, resolution, order):
    """Seeded random contents rounded to half; the distance channel in [0, sqrt 3] on coefficient 0 and small on the rest."""
    rx, ry, rz = resolution
    c = (order + 1) ** 2
    g = rng.normal(0.0, 0.5, (rz, ry * c, rx, 4))
    g[:, :ry, :, :3] = rng.uniform(0.5, 2.0, (rz, ry, rx, 3)) / Y00 * 0.5
    g[..., 3] = rng.uniform(0.0, math.sqrt(3.0), g.shape[:-1])
    return g.astype(np.float16)


def _random_table(rng, w=5, h=3):
    return rng.uniform(0.0, 1.0, (h, w, 2)).astype(np.float32)


@pytest.mark.parametrize("visibility", [False, True])
def test_float32_model_agrees_with_float64_model(visibility):
    rng = np.random.default_rng(11)
    for res, order in (((1, 1, 1), 0), ((3, 2, 1), 2), ((2, 3, 5), 4)):
        grid = M.Grid(_random_grid(rng, res, order), res, _transform(), order)
        s = _random_surface(rng, 400)
        table = _random_table(rng)
        a, b = (M.indirect(s, [grid], table, visibility, dt) for dt in (np.float32, np.float64))
        scale = np.abs(b).max() + 1.0
        err = np.abs(a.astype(np.float64) - b).max()
        print(f"\n{res} order {order} visibility {visibility}: float32 model - float64 model {err:.3e} at magnitude {scale:.3e}")
        assert np.isfinite(a).all() and np.isfinite(b).all()
        # 8 C texel terms of magnitude <= 4 each and C lobe terms, every one a handful of roundings; the weights, the lobes and the table
        # fetch are continuous in the position, so a cell picked differently moves nothing.  2^-12 of the largest value is 256 eps.
        assert err <= 2.0 ** -12 * scale


def _random_pick_case(rng):
    from tauray_amd.scene import trs_matrix
    n = int(rng.integers(1, 5))
    grids = []
    for _ in range(n):
        axis_aligned = rng.random() < 0.5
        scale = tuple(2.0 ** rng.integers(-1, 3, 3)) if axis_aligned else tuple(rng.uniform(0.5, 3.0, 3))
        q = (0.0, 0.0, 0.0, 1.0)
        if not axis_aligned:
            v = rng.normal(size=4)
            q = tuple(v / np.linalg.norm(v))
        t = trs_matrix(tuple(rng.integers(-2, 3, 3).astype(float)) if axis_aligned else tuple(rng.uniform(-2, 2, 3)), q, scale)
        grids.append(dict(transform=t, scaling=scale, resolution=tuple(int(r) for r in rng.integers(1, 6, 3)), radius=float(rng.choice([0.0, 0.25, 0.5, 1.0]))))
    g = grids[int(rng.integers(0, n))]
    kind = int(rng.integers(0, 4))
    local = rng.uniform(-1, 1, 3)
    if kind == 1:      # exactly on a face of the box
        local[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0]))
    elif kind == 2:    # exactly on the guard shell, or just inside it
        local[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0])) * (1.0 + g["radius"] * float(rng.choice([1.0, 0.5])))
    elif kind == 3:    # anywhere
        local = rng.uniform(-3, 3, 3)
    pos = (np.asarray(g["transform"]) @ np.append(local, 1.0))[:3]
    return grids, pos.astype(np.float32)


def test_pick_rule_against_the_model():
    from tauray_amd import renderer as R
    from tauray_amd.scene import ShGrid
    rng = np.random.default_rng(2024)
    seen = set()
    for case in range(200):
        grids, pos = _random_pick_case(rng)
        want = M.pick_grid([g["transform"] for g in grids], [g["scaling"] for g in grids], [g["resolution"] for g in grids], [g["radius"] for g in grids], pos)
        got = R.dshgi_pick_grid([ShGrid(resolution=g["resolution"], radius=g["radius"], transform=g["transform"], scaling=g["scaling"]) for g in grids], pos)
        assert got == want, (case, grids, pos)
        seen.add(got)
    assert len(seen) >= 3
    assert R.dshgi_pick_grid([], (0, 0, 0)) == -1


def test_pick_rule_ties_and_fallback():
    """`<=` on the distance: of two grids at the same distance the later wins.  `>` on the density: of two equally dense grids around the
    point the earlier wins.  Outside every guard shell the largest volume wins."""
    from tauray_amd import renderer as R
    from tauray_amd.scene import ShGrid, trs_matrix
    g = lambda t, s, res, rad: ShGrid(resolution=res, radius=rad, transform=trs_matrix(t, (0, 0, 0, 1), s), scaling=s)      # noqa: E731
    same = [g((0, 0, 0), (1, 1, 1), (2, 2, 2), 0.0), g((0, 0, 0), (1, 1, 1), (2, 2, 2), 0.0)]
    assert R.dshgi_pick_grid(same, (0.5, 0, 0)) == 0
    shell = [g((-2, 0, 0), (1, 1, 1), (2, 2, 2), 1.0), g((2, 0, 0), (1, 1, 1), (2, 2, 2), 1.0)]
    assert R.dshgi_pick_grid(shell, (0, 0, 0)) == 1      # both at distance 1, on both guard shells
    assert R.dshgi_pick_grid(shell, (-0.5, 0, 0)) == 0
    dense = [g((0, 0, 0), (2, 2, 2), (2, 2, 2), 0.0), g((0, 0, 0), (1, 1, 1), (2, 2, 2), 0.0)]
    assert R.dshgi_pick_grid(dense, (0.5, 0, 0)) == 1 and R.dshgi_pick_grid(dense, (1.5, 0, 0)) == 0
    assert R.dshgi_pick_grid(dense, (10, 0, 0)) == 0      # outside both: the larger
    for grids, p in ((same, (0.5, 0, 0)), (shell, (0, 0, 0)), (dense, (10, 0, 0))):
        want = M.pick_grid([x.transform for x in grids], [x.scaling for x in grids], [x.resolution for x in grids], [x.radius for x in grids], np.float32(p))
        assert R.dshgi_pick_grid(grids, p) == want


def _check_binary(tmp_path):
    exe = str(tmp_path / "dshgi_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dshgi_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


def _two_grid_gltf(tmp_path):
    """light_probe.gltf with a second, denser grid inside the first."""
    import json
    doc = json.load(open(FIXTURE))
    doc["nodes"].append({"name": "dense volume", "translation": [1.0, -0.5, 0.25], "scale": [0.5, 0.5, 0.25],
                         "extensions": {"TR_data": {"light_probe": {"type": "GRID", "resolution_x": 4, "resolution_y": 4, "resolution_z": 2, "radius": 0.5}}}})
    doc["scenes"][0]["nodes"].append(len(doc["nodes"]) - 1)
    path = str(tmp_path / "two_grids.gltf")
    json.dump(doc, open(path, "w"))
    return path


PICK_POSITIONS = [(1.0, -0.5, 0.25), (1.2, -0.4, 0.3), (2.4, -0.5, 0.25), (1.0, 1.6, 0.25), (9.0, 9.0, 9.0), (1.0, -0.5, 0.5), (1.0, -0.5, 0.8125)]


def test_both_hosts_pick_the_same_grids(tmp_path):
    """tests/dshgi_check.cc loads a glTF with the C++ loader and prints tr::dshgi_pick_grid for the positions given; the Python host does
    the same with its loader; the model decides.  Built with the host sanitizers."""
    from tauray_amd import renderer as R
    from tauray_amd.gltf import load_glb
    exe = _check_binary(tmp_path)
    for path, count in ((FIXTURE, 1), (_two_grid_gltf(tmp_path), 2)):
        grids = load_glb(path, 64, 64).sh_grids
        assert len(grids) == count
        args = [c for p in PICK_POSITIONS for c in (repr(float(v)) for v in p)]
        out = subprocess.run([exe, "pick", path] + args, capture_output=True, text=True, check=True).stdout.split()
        cpp = [int(v) for v in out]
        py = [R.dshgi_pick_grid(grids, p) for p in PICK_POSITIONS]
        model = [M.pick_grid([g.transform for g in grids], [g.scaling for g in grids], [g.resolution for g in grids], [g.radius for g in grids], np.float32(p))
                 for p in PICK_POSITIONS]
        assert cpp == py == model, (path, cpp, py, model)
        if count == 2:
            assert set(py) == {0, 1}


@pytest.mark.parametrize("args, text", [
    (["--renderer=dshgi", os.path.join(GOLDEN, "animated.glb")], "has no light-probe grid"),
    (["--renderer=dshgi", "--devices=0,1", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi runs on one device"),
    (["--renderer=dshgi", "--process-count=2", "--process-rank=0", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi runs on one device"),
    (["--renderer=dshgi", "--denoiser=bmfr", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=dshgi", "--taa=4", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=dshgi", "--temporal-reprojection=0.5", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=dshgi", "--spatial-reprojection=0", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi: a denoiser, --taa and reprojection do not apply"),
    (["--renderer=dshgi", "--display=looking-glass", os.path.join(GOLDEN, "test.glb")], "--renderer=dshgi: no --display=looking-glass"),
    (["--renderer=dshgi", "--sh-order=5", os.path.join(GOLDEN, "test.glb")], "--sh-order"),
])
def test_cli_refusals(args, text):
    r = subprocess.run([CLI, "--headless=/tmp/unused_dshgi", "--frames=1"] + args, capture_output=True, text=True)
    assert r.returncode != 0
    assert text in r.stderr, r.stderr


# =====================================================================================================================================
# GPU part
@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, eye
    return m


def _cameras(size):
    """Viewport 0 looks around inside the box; viewport 1 stands outside and sees past it."""
    from tauray_amd.scene import Camera
    aspect = size[0] / size[1]
    return [Camera(transform=_look_at((0.3, -0.2, 0.1), (2.0, 1.5, -1.0)), fov=100.0, aspect=aspect),
            Camera(transform=_look_at((7.0, 5.0, 3.0), (1.0, 1.0, 0.5)), fov=50.0, aspect=aspect)]


_STAGES = {}


def _scene_stage(R, ctx, size, strategy=None):
    """The box with the two cameras of `size` on the module's device (a device holds one scene: the last one asked for)."""
    key = (size, strategy)
    if _STAGES.get("current") != key:
        kw = {} if strategy is None else dict(as_strategy=strategy)
        _STAGES["stage"] = R.SceneStage(ctx, _box_scene(cameras=_cameras(size)), **kw)
        _STAGES["current"] = key
    return _STAGES["stage"]


def _grid_of(resolution, transform=None):
    from tauray_amd.scene import ShGrid
    return ShGrid(resolution=tuple(resolution), radius=0.0, transform=_transform() if transform is None else transform, scaling=SCALING)


def _run(R, ctx, ss, size, grids, halfs, table, order, visibility, direct=None, alias=False, instance_grids=None):
    """One frame of both viewports; returns (out, indirect, surface)."""
    st = R.DshgiStage(ctx, ss, size, 2, order, visibility, True)
    images = [ctx.alloc(h.nbytes).upload(h) for h in halfs]
    st.set_grids(grids, images)
    st.set_instance_grids(np.zeros(len(ss.scene.instances), dtype=np.int32) if instance_grids is None else instance_grids)
    tb = ctx.alloc(table.nbytes).upload(table)
    st.set_brdf_integration(tb, table.shape[1], table.shape[0])
    n = size[0] * size[1] * 2
    out = ctx.alloc(n * 16).zero()
    src = None
    if direct is not None:
        src = out.upload(direct) if alias else ctx.alloc(n * 16).upload(direct)
    st.run([0, 1], src, out)
    ctx.sync()
    res = out.download((2, size[1], size[0], 4)), st.download("indirect"), st.download("surface")
    t = st.timings()
    assert t["name"] == "dshgi indirect" and t["frames"] == 1 and t["total_ms"] > 0
    st.close()
    return res


def _check_against_models(got, m32, m64, what):
    """On every value: |stage - float64 model| <= 4 |float32 model - float64 model| + one float32 ulp of the value's magnitude."""
    own = np.abs(m32.astype(np.float64) - m64)
    dev = np.abs(got.astype(np.float64) - m64)
    ulp = np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64)
    slack = dev - (4 * own + ulp)
    worst = np.unravel_index(np.argmax(slack), slack.shape)
    print(f"\n{what}: stage - float64 model max {dev.max():.3e}, float32 model - float64 model max {own.max():.3e}, "
          f"{float((got == m32).mean()):.1%} of the values are the float32 model's bits; worst {worst}: stage off by {dev[worst]:.3e}, "
          f"float32 model by {own[worst]:.3e}, ulp {ulp[worst]:.3e}")
    assert np.isfinite(got).all()
    assert (slack <= 0).all(), f"{what}: {int((slack > 0).sum())} of {slack.size} values outside the bound; worst {worst}: {dev[worst]:.3e} > 4 * {own[worst]:.3e} + {ulp[worst]:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("visibility", [False, True])
@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_closed_form_constant_radiance(R, ctx, order, visibility):
    """The grid is uploaded, nothing is baked: coef[0] = L / Y00, the table a constant (a, b).  Every hit pixel is
    modulate_color(mat, kd * L, L * mix(fresnel * a + b, 1, metallic)) of the record the kernel shaded it with."""
    value = np.array([1.5, 0.75, 0.25])
    a, b = 0.625, 0.125
    for size, res in zip(SIZES, ((1, 1, 1), (2, 3, 5))):
        ss = _scene_stage(R, ctx, size)
        table = np.tile(np.array([a, b], dtype=np.float32), (2, 2, 1))
        out, ind, s = _run(R, ctx, ss, size, [_grid_of(res)], [_constant_grid(res, order, value)], table, order, visibility)
        hit = s["instance_id"] >= 0
        assert hit.any() and (~hit).any() and hit[0].all()      # viewport 0 is inside the box, viewport 1 sees past it
        f64 = np.float64
        L = np.broadcast_to(value * Y00, s.shape + (3,))
        if visibility:      # no corner has weight where the point is projected exactly onto a probe (the model's closed-form test)
            mg = M.Grid(_constant_grid(res, order, value), res, np.asarray(_transform(), dtype=np.float32), order)
            pfw, nfw = M.affine_inverse(mg.transform), M.normal_from_world(mg.transform)
            lit = M.visibility_cell(mg, M._point(pfw, s["pos"]), M._normalize(M._mul3(nfw, s["smooth_normal"])))[3] > 0
            assert (lit & hit).any() == (res != (1, 1, 1))
            L = L * lit[..., None]
        cos_v = np.maximum(-(s["mapped_normal"].astype(f64) * s["view"].astype(f64)).sum(-1), 0)
        rough, f0, metallic = s["roughness"].astype(f64), s["f0"].astype(f64), s["metallic"].astype(f64)
        fresnel = f0 + (np.maximum(1 - rough, f0) - f0) * (1 - cos_v) ** 5
        kd = (1 - fresnel) * (1 - metallic) * (1 - s["transmittance"].astype(f64))
        diffuse = kd[..., None] * L
        reflection = L * ((fresnel * a + b) * (1 - metallic) + metallic)[..., None]
        albedo, m = s["albedo"][..., :3].astype(f64), metallic[..., None]
        want = diffuse * albedo * (1 - m) + reflection * (0.02 * (1 - m) + albedo * m) / (0.02 * (1 - m) + m)
        got = ind[..., :3].astype(f64)
        err = np.abs(got - want)[hit].max()
        print(f"\n{size} grid {res} order {order} visibility {visibility}: largest difference {err:.3e} of {np.abs(want[hit]).max():.3e}")
        # the lookup is 32 eps of L (the model's closed-form test), brdf_indirect and modulate_color a dozen roundings more
        assert err <= 64 * np.finfo(np.float32).eps * np.abs(want[hit]).max()
        assert (ind[~hit] == 0).all() and (ind[..., 3] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("visibility", [False, True])
@pytest.mark.parametrize("res, order, size", [((1, 1, 1), 0, SIZES[0]), ((3, 2, 1), 2, SIZES[1]), ((2, 3, 5), 4, SIZES[0]), ((2, 3, 5), 2, SIZES[1])])
def test_against_the_model(R, ctx, res, order, size, visibility):
    rng = np.random.default_rng(100 * order + res[0])
    ss = _scene_stage(R, ctx, size)
    half, table = _random_grid(rng, res, order), _random_table(rng)
    grid = _grid_of(res)
    out, ind, s = _run(R, ctx, ss, size, [grid], [half], table, order, visibility)
    model_grid = M.Grid(half, res, np.asarray(grid.transform, dtype=np.float32), order)
    m32, m64 = (M.indirect(s, [model_grid], table, visibility, dt) for dt in (np.float32, np.float64))
    hit = s["instance_id"] >= 0
    pfw = M.affine_inverse(model_grid.transform, np.float64)
    local = M._point(pfw, s["pos"][hit].astype(np.float64))
    # the walls lie outside the grid on some axes and inside on others: the clamps are exercised, and so is the interpolation
    assert (np.abs(local) > 1).any(0).all() and (np.abs(local) < 1).any(0).all()
    if visibility and res == (1, 1, 1):
        assert (m64 == 0).all() and (ind == 0).all()      # every point is projected onto the one probe: no corner has weight
    else:
        assert np.abs(m64[hit]).max() > 0.05
    _check_against_models(ind[..., :3], m32, m64, f"{size} grid {res} order {order} visibility {visibility}")


@pytest.mark.gpu
def test_surface_record_misses_and_composition(R, ctx):
    """The record is trhip_feature_render's world-pos, world-normal, albedo and instance id bit for bit; a miss adds exactly 0 and leaves
    the direct colour's bits and alpha; out = direct + indirect bit for bit, also aliased; without direct, out is the indirect term."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    rng = np.random.default_rng(5)
    for size in SIZES:
        ss = _scene_stage(R, ctx, size)
        res, order = (2, 3, 5), 2
        half, table = _random_grid(rng, res, order), _random_table(rng)
        direct = rng.uniform(0.0, 4.0, (2, size[1], size[0], 4)).astype(np.float32)
        direct[0, 0, 0] = [np.float32(1e-30), 0.0, -0.0, 0.25]
        out, ind, s = _run(R, ctx, ss, size, [_grid_of(res)], [half], table, order, False, direct=direct)
        u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)      # noqa: E731
        hit = s["instance_id"] >= 0
        assert hit.any() and (~hit[1]).any()
        assert (u32(out[..., :3]) == u32(direct[..., :3] + ind[..., :3])).all()
        assert (u32(out[..., 3]) == u32(direct[..., 3])).all()
        assert (ind[~hit] == 0).all() and (u32(out[~hit]) == u32(direct[~hit])).all()
        aliased = _run(R, ctx, ss, size, [_grid_of(res)], [half], table, order, False, direct=direct, alias=True)
        assert (u32(aliased[0]) == u32(out)).all()
        alone = _run(R, ctx, ss, size, [_grid_of(res)], [half], table, order, False)
        assert (u32(alone[0]) == u32(ind)).all() and (u32(alone[1]) == u32(ind)).all()
        # two runs: the same bits (the three runs above)
        assert (u32(aliased[1]) == u32(ind)).all()
        n = size[0] * size[1]
        target = ctx.alloc(n * 16)
        for v in range(2):
            for feature, field_name in ((R.FEATURE_WORLD_POS, "pos"), (R.FEATURE_WORLD_NORMAL, "mapped_normal"), (R.FEATURE_ALBEDO, "albedo"), (R.FEATURE_INSTANCE_ID, None)):
                R.FeatureStage(ctx, ss, feature, DistributionParams(size, DISTRIBUTION_DUPLICATE, 0, 1, True), 0, 1e-4).run(target, v)
                ctx.sync()
                f = target.download((size[1], size[0], 4))
                h = hit[v]
                assert (np.isnan(f[..., 0]) == ~h).all()
                if field_name is None:
                    assert (f[..., 0][h] == s["instance_id"][v][h]).all()
                else:
                    k = s[field_name].shape[-1]
                    assert (u32(f[..., :k][h]) == u32(s[field_name][v][h])).all(), (v, field_name)
        target.free()


@pytest.mark.gpu
def test_a_list_longer_than_one_launch(R, ctx):
    """65 viewports are two launches, of 64 and of 1: layer 64 is layer 0 of a one-entry list of its viewport and layer 63 repeats layer 0,
    bit for bit - colour, indirect term and surface record.  17 x 9 pixels leave the tile partial on both axes."""
    rng = np.random.default_rng(17)
    size, res, order = (17, 9), (2, 3, 5), 2
    ss = _scene_stage(R, ctx, size)
    half, table = _random_grid(rng, res, order), _random_table(rng)

    def frame(views):
        st = R.DshgiStage(ctx, ss, size, len(views), order, False, True)
        image, tb = ctx.alloc(half.nbytes).upload(half), ctx.alloc(table.nbytes).upload(table)
        st.set_grids([_grid_of(res)], [image])
        st.set_instance_grids(np.zeros(len(ss.scene.instances), dtype=np.int32))
        st.set_brdf_integration(tb, table.shape[1], table.shape[0])
        out = ctx.alloc(size[0] * size[1] * len(views) * 16).zero()
        st.run(views, None, out)
        ctx.sync()
        got = [out.download((len(views), size[1], size[0], 4)), st.download("indirect"), st.download("surface")]
        st.close()
        for b in (image, tb, out):
            b.free()
        return got

    many, one = frame([0] * 64 + [1]), frame([1])
    assert (many[2]["instance_id"][0] >= 0).any() and np.abs(many[1][0]).max() > 0
    for a, b in zip(many, one):
        assert a[64].tobytes() == b[0].tobytes() and a[63].tobytes() == a[0].tobytes()
    assert many[1][64].tobytes() != many[1][0].tobytes(), "the two viewports see the same"


@pytest.mark.gpu
def test_same_bits_for_both_acceleration_structures(R, ctx):
    from tauray_amd import _lib
    rng = np.random.default_rng(9)
    size, res, order = SIZES[1], (3, 2, 1), 4
    half, table = _random_grid(rng, res, order), _random_table(rng)
    got = []
    for strategy in (_lib.AS_ALL_MERGED, _lib.AS_PER_MESH):
        for visibility in (False, True):
            ss = _scene_stage(R, ctx, size, strategy)
            got.append(_run(R, ctx, ss, size, [_grid_of(res)], [half], table, order, visibility)[1])
    assert (got[0].view(np.uint32) == got[2].view(np.uint32)).all() and (got[1].view(np.uint32) == got[3].view(np.uint32)).all()
    assert (got[0] != got[1]).any()


def _quad_scene(size):
    """Three unit quads facing +z at x = 0, 1.5 and 10 (one instance each), seen from above by two cameras."""
    from tauray_amd import scene as S
    from tauray_amd.scene import Camera
    insts, verts, spans, idx = [], [], [], []
    for k, x in enumerate((0.0, 1.5, 10.0)):
        v = np.zeros(4, dtype=S.VERTEX)
        v["pos"] = [(-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)]
        v["normal"] = (0, 0, 1)
        v["tangent"] = (1, 0, 0, 1)
        v["uv"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
        model = np.eye(4)
        model[0, 3] = x
        insts.append(S.make_instance(model, S.make_material(albedo=(0.8, 0.6, 0.4, 1.0), metallic=0.25 * k, roughness=0.5, double_sided=True)))
        verts.append(v)
        spans.append((4 * k, 4, 6 * k, 2))
        idx += [0, 1, 2, 0, 2, 3]
    aspect = size[0] / size[1]
    cams = [Camera(transform=_look_at((0.75, 0.0, 3.0), (0.75, 0.0, 0.0), up=(0, 1, 0)), fov=60.0, aspect=aspect),
            Camera(transform=_look_at((10.0, 0.0, 2.0), (10.0, 0.0, 0.0), up=(0, 1, 0)), fov=60.0, aspect=aspect)]
    return S.SceneDesc(instances=np.concatenate(insts), spans=np.array(spans, dtype=S.MESH_SPAN), vertices=np.concatenate(verts),
                       indices=np.array(idx, dtype=np.uint32), cameras=cams, name="dshgi_quads").finalize(True)


@pytest.mark.gpu
def test_two_grids(R, ctx):
    """The quad at the origin lies in both grids and shades from the denser one, the quad at x = 1.5 only in the large one, the quad at
    x = 10 in neither: it takes the grid of largest volume.  The record's grid index is the model's pick."""
    from tauray_amd.scene import ShGrid, trs_matrix
    rng = np.random.default_rng(21)
    size, order = SIZES[1], 2
    scene = _quad_scene(size)
    ss = R.SceneStage(ctx, scene)
    _STAGES["current"] = None
    grids = [ShGrid(resolution=(2, 2, 2), radius=0.0, transform=trs_matrix((0, 0, 0), (0, 0, 0, 1), (2, 2, 2)), scaling=(2, 2, 2)),
             ShGrid(resolution=(3, 2, 2), radius=0.0, transform=trs_matrix((0, 0, 0), (0, 0, 0, 1), (1, 1, 1)), scaling=(1, 1, 1))]
    picks = R.dshgi_instance_grids(grids, scene.instances)
    model = [M.pick_grid([g.transform for g in grids], [g.scaling for g in grids], [g.resolution for g in grids], [g.radius for g in grids], np.float32(p))
             for p in ((0, 0, 0), (1.5, 0, 0), (10, 0, 0))]
    assert picks.tolist() == model == [1, 0, 0]
    halfs, table = [_random_grid(rng, g.resolution, order) for g in grids], _random_table(rng)
    for visibility in (False, True):
        out, ind, s = _run(R, ctx, ss, size, grids, halfs, table, order, visibility, instance_grids=picks)
        hit = s["instance_id"] >= 0
        assert set(np.unique(s["instance_id"][hit])) == {0, 1, 2}
        assert (s["grid"][hit] == picks[s["instance_id"][hit]]).all() and (s["grid"][~hit] == -1).all()
        mg = [M.Grid(h, g.resolution, np.asarray(g.transform, dtype=np.float32), order) for g, h in zip(grids, halfs)]
        m32, m64 = (M.indirect(s, mg, table, visibility, dt) for dt in (np.float32, np.float64))
        _check_against_models(ind[..., :3], m32, m64, f"two grids, visibility {visibility}")


@pytest.mark.gpu
def test_stage_refusals(R, ctx):
    """The refusals that need a stage, and a stage needs a device."""
    from tauray_amd._lib import TrhipError
    size = SIZES[0]
    fresh = R.Context(0)
    st = R.DshgiStage(fresh, None, size, 2, 2)
    out = fresh.alloc(size[0] * size[1] * 2 * 16)
    half = _constant_grid((1, 1, 1), 2, 1.0)
    image = fresh.alloc(half.nbytes).upload(half)
    table = fresh.alloc(8).upload(np.zeros(2, dtype=np.float32))
    with pytest.raises(TrhipError, match="trhip_dshgi_render: no scene"):
        st.run([0, 1], None, out)
    ss = R.SceneStage(fresh, _box_scene(cameras=_cameras(size)))
    with pytest.raises(TrhipError, match="trhip_dshgi_render: no grids set"):
        st.run([0, 1], None, out)
    with pytest.raises(TrhipError, match="trhip_dshgi_set_grids: no grids"):
        st.set_grids([], [])
    with pytest.raises(TrhipError, match="trhip_dshgi_set_instance_grids: no grids set"):
        st.set_instance_grids([0] * 6)
    st.set_grids([_grid_of((1, 1, 1))], [image])
    with pytest.raises(TrhipError, match="0 instance grids set .*, the scene has 6 instances"):
        st.run([0, 1], None, out)
    with pytest.raises(TrhipError, match="instance 2: grid index 1 is out of range: 1 grids"):
        st.set_instance_grids([0, 0, 1, 0, 0, 0])
    with pytest.raises(TrhipError, match="grid index -2 is out of range"):
        st.set_instance_grids([-2] * 6)
    st.set_instance_grids([0] * 5)
    with pytest.raises(TrhipError, match="5 instance grids set .*, the scene has 6 instances"):
        st.run([0, 1], None, out)
    st.set_instance_grids([0, -1, 0, 0, 0, 0])
    with pytest.raises(TrhipError, match="trhip_dshgi_render: no BRDF-integration table"):
        st.run([0, 1], None, out)
    st.set_brdf_integration(table, 1, 1)
    with pytest.raises(TrhipError, match="viewport 2 out of range"):
        st.run([0, 2], None, out)
    with pytest.raises(TrhipError, match="3 viewports, the stage has 2 layers"):
        st.run([0, 1, 0], None, out)
    st.run([0, 1], None, out)
    fresh.sync()
    with pytest.raises(TrhipError, match="only kept with record_surface"):
        st.download("surface")
    ind = st.download("indirect")
    assert np.isfinite(ind).all()
    inst = np.ascontiguousarray(ss.scene.instances)
    from tauray_amd import _lib
    _lib.check(_lib.lib().trhip_scene_update_instances(fresh.h, inst.ctypes.data, len(inst)))      # invalidates the structure
    with pytest.raises(TrhipError, match="no acceleration structure: call trhip_scene_build_accel first"):
        st.run([0, 1], None, out)
    st.close()
    fresh.close()


def _generated(R, ctx, size, samples):
    buf = R.brdf_integration_table(ctx, size, samples)
    ctx.sync()
    t = buf.download((size, size, 2))
    buf.free()
    return t


@pytest.mark.gpu
def test_generated_table_against_the_model(R, ctx):
    """A sample's term is at most 4 (g <= 4 steps aside, vh / (H.z V.z) is bounded by the cell's 1 / cos_v <= 2 size) - the sum of N terms
    in float32 in one chain is within N eps of its largest partial sum relative, and each term carries a dozen roundings.  So a cell is
    within (N + 16) eps of max(1, its value) of the float64 model; the float32 model, which adds in the same order, mostly has its bits."""
    for size, samples in ((8, 64), (5, 33)):
        got = _generated(R, ctx, size, samples)
        m32, m64 = (M.brdf_integration_table(size, samples, dt) for dt in (np.float32, np.float64))
        assert np.isfinite(got).all() and (got >= 0).all()
        err = np.abs(got.astype(np.float64) - m64)
        same = float((got == m32).mean())
        print(f"\ntable {size} x {size}, {samples} samples: stage - float64 model {err.max():.3e}, {same:.1%} of the cells are the float32 model's bits")
        bound = (samples + 16) * np.finfo(np.float32).eps * np.maximum(1.0, np.abs(m64))
        assert (err <= bound).all()
        _check_against_models(got, m32, m64, f"table {size}")


# Measured on an MI355X: the generated 256 x 256 table of 1024 samples against tests/golden/brdf_integration.exr (the reference's
# data/brdf_integration.exr, channels by name: R = scale, G = bias, row 0 first as texture() addresses it): maximum 0.3708 (the bias at
# cos_v = 0.5 / 256, row 3: generated 0.983, file 0.612), mean 0.03136.  The large differences sit in the grazing columns at low roughness,
# where the rule's separable Smith G and 1024 samples of a lobe of width alpha meet whatever made the file; the rule is kept (DESIGN.md
# section 20).  The bound is twice the measured maximum.
TABLE_MAX_ABS_MEASURED = 3.707785e-01
TABLE_MEAN_ABS_MEASURED = 3.136421e-02


@pytest.mark.gpu
def test_generated_table_against_the_reference_file(R, ctx):
    want = R.load_brdf_integration(TABLE_FIXTURE)
    assert want.shape == (256, 256, 2)
    got = _generated(R, ctx, 256, 1024)
    diff = np.abs(got.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(diff), diff.shape)
    print(f"\ngenerated table against the reference's file: max {diff.max():.6e} at {worst} (generated {got[worst]:.6f}, file {want[worst]:.6f}), mean {diff.mean():.6e}; "
          f"per channel max {diff[..., 0].max():.6e} {diff[..., 1].max():.6e}")
    assert TABLE_MAX_ABS_MEASURED is not None, "the measured distance has not been recorded"
    assert diff.max() <= 2 * TABLE_MAX_ABS_MEASURED


# =====================================================================================================================================
# the whole renderer
TEST_GLB = os.path.join(GOLDEN, "test.glb")      # the reference's test scene: meshes, a camera, lights and one 4 x 4 x 4 grid
RENDERER_SIZE = SIZES[1]
RENDERER_SH = dict(max_bounces=3, samples_per_probe=32, sh_order=2, temporal_ratio=0.01, film=0, film_radius=0.5, indirect_clamping=0.0,
                   regularization_gamma=0.0)


def _renderer(R, ctx, visibility=False, **kw):
    from tauray_amd.gltf import load_glb
    scene = load_glb(TEST_GLB, *RENDERER_SIZE)
    assert len(scene.sh_grids) == 1 and len(scene.cameras) == 1
    ss = R.SceneStage(ctx, scene)
    _STAGES["current"] = None
    opt = R.options_for_scene(scene, max_bounces=3)
    sh = dict(RENDERER_SH, nee_point=opt.nee_point, nee_directional=opt.nee_directional, nee_envmap=opt.nee_envmap, nee_triangles=opt.nee_triangles)
    return scene, ss, opt, R.DshgiRenderer(ctx, ss, scene, RENDERER_SIZE, opt, sh=sh, use_probe_visibility=visibility, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("visibility", [False, True])
def test_renderer_frame_is_direct_plus_indirect(R, ctx, visibility):
    """light_probe.gltf has a grid and nothing to see (no mesh, no camera), so the frame is the reference's test scene, which has one grid.
    Two frames of the renderer are the direct stage plus the indirect stage run by hand on the grids the renderer's own bake left."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    w, h = RENDERER_SIZE
    scene, ss, opt, rr = _renderer(R, ctx, visibility)
    direct = R.DirectStage(ctx, ss, R.copy_options(opt, nee_triangles=0.0, nee_envmap=0.0), DistributionParams(RENDERER_SIZE, DISTRIBUTION_DUPLICATE, 0, 1, True))
    st = R.DshgiStage(ctx, ss, RENDERER_SIZE, 1, 2, visibility, True, opt.projection, opt.min_ray_dist)
    st.set_grids(scene.sh_grids, [s.device_grids()[1] for s in rr.sh.stages])
    st.set_instance_grids(R.dshgi_instance_grids(scene.sh_grids, scene.instances))
    table = R.brdf_integration_table(ctx)
    ctx.sync()
    st.set_brdf_integration(table, 256, 256)
    color, display = ctx.alloc(w * h * 16).zero(), ctx.alloc(w * h * 16).zero()
    u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)      # noqa: E731
    for frame in range(2):
        rr.render()
        got, shown = rr.download("color"), rr.download("display")
        direct.reset_accumulated_samples()
        direct.run(color, 1)
        ctx.sync()
        alone = color.download((1, h, w, 4))
        st.run([0], color, color)
        R.TonemapStage(ctx).run(color, display, w, h, 1)
        ctx.sync()
        want = color.download((1, h, w, 4))
        ind = st.download("indirect")
        assert np.isfinite(got).all() and (ind[..., :3] > 0).any() and (alone != want).any()
        assert (u32(got) == u32(want)).all(), f"frame {frame}"
        assert (u32(shown) == u32(display.download((1, h, w, 4)))).all(), f"frame {frame}"
    t = rr.timings()
    assert t["indirect"]["name"] == "dshgi indirect" and t["indirect"]["frames"] == 2 and t["bake"][0]["frames"] == 2
    s = st.download("surface")
    assert (s["grid"][s["instance_id"] >= 0] == 0).all()
    for x in (rr, direct, st):
        x.close()


@pytest.mark.gpu
def test_renderer_takes_a_table_from_a_file(R, ctx):
    """--brdf-integration=FILE.exr: the file's R and G as texture() reads them.  With the reference's own table the frame moves by no more than
    the tables differ (the specular term is at most incoming_reflection * (fresnel * d_scale + d_bias))."""
    scene, ss, opt, generated = _renderer(R, ctx)
    generated.render()
    a = generated.download("color")
    generated.close()
    scene, ss, opt, loaded = _renderer(R, ctx, brdf_integration=TABLE_FIXTURE)
    loaded.render()
    b = loaded.download("color")
    loaded.close()
    assert np.isfinite(b).all() and (a != b).any()
    print(f"\ngenerated table against the file's: the frame moves by at most {np.abs(a - b).max():.3e} of {np.abs(a).max():.3e}")


@pytest.mark.gpu
def test_cli_frames_are_the_python_hosts(R, ctx, tmp_path):
    """tauray_hip --renderer=dshgi on the reference's test scene: two frames, the second baked into the first's history, are the bits of the
    Python host with the same options - in both modes."""
    w, h = RENDERER_SIZE
    for visibility in (False, True):
        prefix = str(tmp_path / f"dshgi{int(visibility)}_")
        subprocess.run([CLI, TEST_GLB, "--renderer=dshgi", f"--width={w}", f"--height={h}", "--samples-per-probe=32", "--sh-order=2", "--max-ray-depth=3", "--frames=2",
                        "--filetype=raw", "--headless=" + prefix] + (["--use-probe-visibility"] if visibility else []), check=True, capture_output=True, text=True)
        scene, ss, opt, rr = _renderer(R, ctx, visibility)
        for f in range(2):
            rr.render()
            want = rr.download("display")
            got = np.fromfile(f"{prefix}{f}.raw", dtype=np.float32).reshape(want.shape)
            assert np.isfinite(want).all() and want[..., :3].max() > 0
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), f"visibility {visibility}, frame {f}"
        rr.close()


def _animated_glb_with_a_grid(tmp_path):
    """tests/golden/animated.glb with a probe grid around its moving box."""
    import json
    import struct
    data = open(os.path.join(GOLDEN, "animated.glb"), "rb").read()
    n = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + n])
    rest = data[20 + n:]
    doc["nodes"].append({"name": "volume", "scale": [3.0, 3.0, 3.0],
                         "extensions": {"TR_data": {"light_probe": {"type": "GRID", "resolution_x": 2, "resolution_y": 3, "resolution_z": 2, "radius": 0.5}}}})
    doc["scenes"][0]["nodes"].append(len(doc["nodes"]) - 1)
    doc["extensionsUsed"] = sorted(set(doc.get("extensionsUsed", [])) | {"TR_data"})
    text = json.dumps(doc).encode()
    text += b" " * (-len(text) % 4)
    body = struct.pack("<II", len(text), 0x4E4F534A) + text + rest
    path = str(tmp_path / "animated_grid.glb")
    open(path, "wb").write(data[:8] + struct.pack("<I", 12 + len(body)) + body)
    return path


@pytest.mark.gpu
def test_cli_animation_picks_grids_again(tmp_path):
    w, h = RENDERER_SIZE
    prefix = str(tmp_path / "anim")
    r = subprocess.run([CLI, _animated_glb_with_a_grid(tmp_path), "--renderer=dshgi", "--animation", "--framerate=4", f"--width={w}", f"--height={h}", "--samples-per-probe=16",
                        "--sh-order=1", "--max-ray-depth=2", "--frames=2", "--filetype=raw", "--headless=" + prefix, "-t"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[dshgi indirect]" in r.stdout and "[SH path tracing]" in r.stdout
    frames = [np.fromfile(f"{prefix}{f}.raw", dtype=np.float32).reshape(h, w, 4) for f in range(2)]
    assert all(np.isfinite(f).all() for f in frames) and (frames[0] != frames[1]).any()


# =====================================================================================================================================
# end to end, independent of the model and of the oracle
def _lit_box(size, albedo=0.8):
    """The closed box, nothing emits, every wall a dielectric of one albedo; one sphere light under the ceiling; a camera that looks at the floor
    and two walls and does not see the light."""
    from tauray_amd import scene as S
    from tauray_amd.scene import Camera
    scene = _box_scene(emission=[(0.0, 0.0, 0.0)] * 6, albedo=[(albedo,) * 3] * 6, metallic=[0.0] * 6,
                       cameras=[Camera(transform=_look_at((1.2, 0.9, 0.9), (-1.2, -0.9, -1.0)), fov=50.0, aspect=size[0] / size[1])])      # the light is 32 degrees above the axis
    scene.point_lights = S.make_point_light((6.0, 6.0, 6.0), (0.0, 0.0, 0.9), 0.05)
    return scene.finalize(True)


def _end_to_end_means(R, ctx, size=SIZES[1], depth=3, frames=4, spp=2048):
    """Image means (rgb together) of the dshgi frame, of its direct light alone and of the path tracer at depth + 1."""
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    from tauray_amd.scene import ShGrid, trs_matrix
    w, h = size
    scene = _lit_box(size)
    half_extent = tuple((np.array(BOX_HI) - np.array(BOX_LO)) / 2)
    centre = tuple((np.array(BOX_HI) + np.array(BOX_LO)) / 2)
    scene.sh_grids = [ShGrid(resolution=(4, 4, 4), radius=0.0, transform=trs_matrix(centre, (0, 0, 0, 1), half_extent), scaling=half_extent)]
    ss = R.SceneStage(ctx, scene)
    _STAGES["current"] = None
    opt = R.options_for_scene(scene, max_bounces=depth, samples_per_pixel=16, samples_per_pass=16)
    sh = dict(max_bounces=depth, samples_per_probe=512, sh_order=2, temporal_ratio=0.0, nee_point=1.0, nee_directional=0.0, nee_envmap=0.0, nee_triangles=0.0)
    rr = R.DshgiRenderer(ctx, ss, scene, size, opt, sh=sh)
    for _ in range(frames):
        rr.render()
    full = rr.download("color")[0, ..., :3].astype(np.float64)
    ind = rr.indirect.download("indirect")[0, ..., :3].astype(np.float64)
    rr.close()
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=depth + 1, samples_per_pixel=spp, samples_per_pass=16),
                           DistributionParams(size, DISTRIBUTION_DUPLICATE, 0, 1, True))
    color = ctx.alloc(w * h * 16).zero()
    pt.run(color)
    ctx.sync()
    ref = color.download((h, w, 4))[..., :3].astype(np.float64)
    pt.close()
    color.free()
    return full.mean(), (full - ind).mean(), ref.mean()


# Measured on an MI355X (profiles/r17/dshgi.txt): |mean(dshgi) - mean(path tracer)| / mean(path tracer) of the lit box.
# The difference is SH truncation at order 2 and the interpolation between 4 x 4 x 4 probes; nothing derives it.
# dshgi 0.795039, path tracer 0.818438: 2.859 % (the direct light alone, 0.268774, misses by 67.16 %)
END_TO_END_RELATIVE_MEASURED = 0.028590


@pytest.mark.gpu
def test_image_mean_against_the_path_tracer(R, ctx):
    full, direct_only, ref = _end_to_end_means(R, ctx)
    rel, rel_direct = abs(full - ref) / ref, abs(direct_only - ref) / ref
    print(f"\nlit box: image mean dshgi {full:.6f}, direct alone {direct_only:.6f}, path tracer {ref:.6f}: off by {rel:.4%} with the indirect term, {rel_direct:.4%} without")
    assert END_TO_END_RELATIVE_MEASURED is not None, "the measured difference has not been recorded"
    bound = 2 * END_TO_END_RELATIVE_MEASURED
    assert rel_direct > bound, "without the indirect term the frame must miss the bound, or the comparison shows nothing"
    assert rel <= bound
