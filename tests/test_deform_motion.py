"""Motion vectors of skinned and morphed meshes (trhip_scene_set_deformation_motion / trhip_scene_latch_positions /
trhip_scene_get_previous_positions, k_latch_positions, surface_prev_pos).

CPU: the numpy rule (tests/deform_motion_model.py) at float32 against float64 and the share of the motion bound the affine argument uses
up, the ABI, the refusals the arguments alone decide, the command line's usage text, the C++ option plumbing and call order
(tests/deform_motion_check.cc under the host sanitizers) and the Python host's call order against a recording library.  GPU: the plane bit
for bit, affine deformations against the unchanged oracle, the other consumers of surface_prev_pos, that nothing else moves, both hosts."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deform_motion_model as DM
import morph_model as MM
from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "tauray_amd", "tauray_hip")
BT = 256                     # lanes per block of k_latch_positions (bvh_build.hip)
ALL, PER_MESH = 0, 1
SIZE = (64, 64)
f32 = np.float32
VERTEX_COUNTS = (1, BT - 1, BT, BT + 1, 3 * BT + 7)
ENTRY_POINTS = {"trhip_scene_set_deformation_motion": 2, "trhip_scene_latch_positions": 1, "trhip_scene_get_previous_positions": 4}


def motion_bound(reference):
    """The bound tests/test_gpu_parity.py test_animated_glb_playback holds its motion features to."""
    return 1e-5 * max(1.0, float(np.abs(reference).max()))


@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


# ------------------------------------------------------------------------------------------------------------------ the affine cases
# Quarter turns and translations by multiples of 1/8 (deform_motion_model.rigid): the joint at frames A and B, the instance matrix and
# the camera at the previous and the current frame.  The morph target's deltas are D * base + d, so the mesh at weight w is G(w) * base.
JOINT_A, JOINT_B = DM.rigid(1, (0.125, -0.25, 0.0)), DM.rigid(2, (-0.25, 0.125, 0.125))
MODEL_PREV, MODEL = DM.rigid(0, (0.125, 0.125, -0.25)), DM.rigid(0, (-0.125, 0.0, 0.0))
MORPH_D, MORPH_d = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), np.array([0.125, -0.25, 0.125])
WEIGHT_A, WEIGHT_B = 0.5, 1.0
CAMERA_PREV, CAMERA = DM.rigid(0, (0.25, -0.125, 6.0)), DM.rigid(0, (0.0, 0.0, 6.0))


def morph_pose(w):
    g = np.eye(4)
    g[:3, :3] += w * MORPH_D
    g[:3, 3] = w * MORPH_d
    return g


def _sheet(n=9, half=0.75):
    """An n x n sheet in the xy plane facing +z; with n = 9 and half = 0.75 its coordinates are multiples of 3/16."""
    from tauray_amd.scene import VERTEX
    u, vv = np.meshgrid(np.linspace(-half, half, n), np.linspace(-half, half, n))
    v = np.zeros(n * n, dtype=VERTEX)
    v["pos"] = np.stack([u.reshape(-1), vv.reshape(-1), np.zeros(n * n)], axis=1)
    v["normal"] = (0, 0, 1)
    v["tangent"] = (1, 0, 0, 1)
    v["uv"] = v["pos"][:, :2] / (2 * half) + 0.5
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    idx = np.stack([a, a + 1, a + n, a + 1, a + n + 1, a + n], axis=1).reshape(-1).astype(np.uint32)
    return v, idx


def _strip_indices(n):
    if n < 3:
        return np.zeros(3, np.uint32)
    i = np.arange(n - 2, dtype=np.uint32)
    return np.stack([i, i + 1, i + 2], axis=1).reshape(-1)


def _scene(meshes, uses=None, models=None, models_prev=None, camera=CAMERA):
    """A SceneDesc of one instance per entry of `uses` (the mesh it shows; default one per mesh), a point light and a square camera."""
    from tauray_amd import scene as S
    uses = list(range(len(meshes))) if uses is None else uses
    voff, ioff, where = 0, 0, []
    for v, idx in meshes:
        where.append((voff, len(v), ioff, len(idx) // 3))
        voff, ioff = voff + len(v), ioff + len(idx)
    inst = []
    for k, m in enumerate(uses):
        mat = S.make_material(albedo=(0.3 + 0.1 * (k % 5), 0.6, 0.8 - 0.1 * (k % 4), 1), metallic=0.0, roughness=0.6, double_sided=True)
        rec = S.make_instance(np.eye(4) if models is None else models[k], mat)
        if models_prev is not None:
            rec["model_prev"][0] = S.to_glm(models_prev[k])
        inst.append(rec)
    cam = S.Camera(transform=np.array(camera, dtype=np.float64), fov=40.0, near=0.1, far=100.0)
    cam.set_aspect(1.0)
    sc = S.SceneDesc(instances=np.concatenate(inst), spans=np.array([where[m] for m in uses], dtype=S.MESH_SPAN), vertices=np.concatenate([m[0] for m in meshes]),
                     indices=np.concatenate([m[1] for m in meshes]).astype(np.uint32),
                     point_lights=S.make_point_light(np.array([20.0, 19.0, 18.0]), (0.5, 2.0, 3.0), 0.0), cameras=[cam])
    return sc.finalize(True)


def _camera(transform):
    from tauray_amd import scene as S
    cam = S.Camera(transform=np.array(transform, dtype=np.float64), fov=40.0, near=0.1, far=100.0)
    cam.set_aspect(1.0)
    return cam


def _one_joint_skins(n):
    from tauray_amd.scene import SKIN
    skins = np.zeros(n, dtype=SKIN)
    skins["weights"][:, 0] = 1
    return skins


def _affine_scene(models_prev=(MODEL_PREV, np.eye(4))):
    """The sheet under a moving instance matrix in front of a static wall."""
    sheet, wall = _sheet(), _sheet(3, 2.0)
    back = DM.rigid(0, (0.0, 0.0, -1.5))
    return _scene([sheet, wall], models=[MODEL, back], models_prev=[models_prev[0], back]), sheet


def _affine_delta(base):
    return ((MORPH_D @ base["pos"].astype(np.float64).T).T + MORPH_d).astype(f32)[None]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# =========================================================================================================================== CPU
@pytest.mark.parametrize("seed, vertices", [(1, 3), (2, 255), (3, 775)])
def test_model_float32_against_float64(seed, vertices):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2, 2, (vertices, 3)).astype(f32)
    m = np.eye(4)
    m[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    m[:3, 3] = rng.uniform(-3, 3, 3)
    m = m.astype(f32)
    eps = float(np.finfo(f32).eps)
    for _ in range(200):
        tri = rng.integers(0, vertices, 3)
        u = rng.uniform(0, 1)
        v = rng.uniform(0, 1 - u)
        a = DM.previous_world_position(m, pos, tri, u, v)
        b = DM.previous_world_position(m, pos, tri, f32(u), f32(v), dtype=np.float64)
        assert a.dtype == f32
        # 1 - u - v: 2 roundings of a value <= 1; the interpolation: 3 products and 2 sums of magnitudes <= 2; the transform: 3 products and
        # 3 sums of magnitudes <= |m| |p| + |t| <= 2 sqrt(3) + 3 per row: well inside 16 eps of the largest magnitude, 7
        assert np.abs(a.astype(np.float64) - b).max() <= 16 * eps * 7
    # barycentrics at a corner give the vertex, exactly
    assert np.array_equal(DM.interpolate(pos, (0, 1, 2), 0.0, 0.0), pos[0]) and np.array_equal(DM.interpolate(pos, (0, 1, 2), 1.0, 0.0), pos[1])


def test_affine_argument_uses_a_small_share_of_the_bound():
    """Section 2's comparison stands on `model_prev * interp(A * current) = (model_prev * A) * interp(current)`.  With the matrices the
    GPU tests use, both sides are evaluated at float32 (the left as the kernel does, the right as the oracle does) against float64: each
    differs from the exact value by less than a tenth of the motion bound, 1e-6 for values up to 1 - so the bound is left to the kernels."""
    base, idx = _sheet()
    rng = np.random.default_rng(5)
    worst = 0.0
    for prev_pose, cur_pose in ((JOINT_A, JOINT_B), (morph_pose(WEIGHT_A), morph_pose(WEIGHT_B))):
        previous = (prev_pose[:3, :3] @ base["pos"].astype(np.float64).T).T + prev_pose[:3, 3]
        current = (cur_pose[:3, :3] @ base["pos"].astype(np.float64).T).T + cur_pose[:3, 3]
        assert np.array_equal(previous, previous.astype(f32)) and np.array_equal(current, current.astype(f32)), "the poses are exact in float32"
        A = DM.affine_between(prev_pose, cur_pose)
        assert np.abs(A @ np.append(current[7], 1.0) - np.append(previous[7], 1.0)).max() < 1e-12
        for t in rng.integers(0, len(idx) // 3, 300):
            tri = idx[3 * t:3 * t + 3]
            u = rng.uniform(0, 1)
            v = rng.uniform(0, 1 - u)
            exact = DM.previous_world_position(MODEL_PREV, previous, tri, f32(u), f32(v), dtype=np.float64)
            kernel = DM.previous_world_position(MODEL_PREV.astype(f32), previous.astype(f32), tri, u, v)
            oracle = DM.affine_expected(MODEL_PREV, A, current.astype(f32), tri, u, v)
            worst = max(worst, float(np.abs(kernel - exact).max()), float(np.abs(oracle - exact).max()))
    assert worst <= 0.1 * 1e-5, worst


def test_entry_points_declared_exported_and_bound(tmp_path):
    from tauray_amd import _lib
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    src = tmp_path / "sig.c"
    src.write_text('#include "trhip.h"\n'
                   "int (*set_motion)(trhip_device*, int) = trhip_scene_set_deformation_motion;\n"
                   "int (*latch)(trhip_device*) = trhip_scene_latch_positions;\n"
                   "int (*get_previous)(trhip_device*, uint32_t, float*, uint32_t) = trhip_scene_get_previous_positions;\nint main(void) { return 0; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sig.o")])
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tauray_amd", "libtrhip.so")], capture_output=True, text=True)
    for name, args in ENTRY_POINTS.items():
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(L, name)
        assert _lib.SYMBOLS[name][0] is C.c_int and len(_lib.SYMBOLS[name][1]) == args
        if nm.returncode == 0:
            assert re.search(r"\bT %s$" % name, nm.stdout, re.M)


def _refusal(call, *args):
    from tauray_amd import _lib
    assert call(*args) != 0
    return _lib.lib().trhip_last_error().decode()


def test_refusals_the_arguments_decide():
    """What needs no device to be refused is refused before the device is looked at: these run with a null handle."""
    from tauray_amd import _lib
    L = _lib.lib()
    out = np.zeros((4, 3), f32)
    assert "trhip_scene_get_previous_positions: null output" in _refusal(L.trhip_scene_get_previous_positions, None, 0, None, 4)
    assert "null trhip_device" in _refusal(L.trhip_scene_get_previous_positions, None, 0, out.ctypes.data, 4)
    assert "null trhip_device" in _refusal(L.trhip_scene_set_deformation_motion, None, 1)
    assert "null trhip_device" in _refusal(L.trhip_scene_latch_positions, None)


def test_command_line_names_the_option():
    p = subprocess.run([CLI], capture_output=True, text=True)
    assert p.returncode != 0 and "--deformation-motion" in p.stderr + p.stdout
    head = open(os.path.join(ROOT, "tauray_amd", "host", "tauray_hip_cli.cc")).read().split("#include")[0]
    assert "--deformation-motion" in head
    p = subprocess.run([CLI, "--deformation-motions", os.path.join(GOLDEN, "morph.glb")], capture_output=True, text=True)
    assert p.returncode != 0 and "unknown option --deformation-motions" in p.stderr + p.stdout


def test_cpp_host_plumbing_under_the_sanitizers(tmp_path):
    """tests/deform_motion_check.cc: the defaults, and the calls scene_stage::set_scene and scene_stage::apply make, in order."""
    exe = str(tmp_path / "deform_motion_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "deform_motion_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)

    def run(*a):
        p = subprocess.run([exe] + list(a), capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", p.stderr      # a sanitizer report goes to stderr
        return p.stdout.strip()
    assert run("options") == "0 0"
    frame = ["update_instances", "morph 0", "skin 1", "update_cameras", "refit"]
    latched = frame[:1] + ["latch"] + frame[1:]
    upload = ["set_skin 1", "set_morph_targets 0", "morph 0", "skin 1", "build"]
    off = [part.strip().split("\n") for part in run("order", "0").split("--")]
    assert off == [["upload", "set_deformation_motion 0"] + upload, frame, latched, ["set_deformation_motion 1"] + latched[:-1] + ["build"]]
    on = [part.strip().split("\n") for part in run("order", "1").split("--")]
    assert on == [["upload", "set_deformation_motion 1"] + upload[:-1] + ["latch", "build"], latched, latched, ["set_deformation_motion 1"] + latched[:-1] + ["build"]]


class _RecordingLibrary:
    """Stands in for libtrhip: every entry point succeeds and leaves its name behind."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name.replace("trhip_scene_", "") + (f" {args[1]}" if name.endswith("set_deformation_motion") else ""))
            return 0
        return call


def test_python_host_call_order(monkeypatch):
    """SceneStage.animate and pose: latch before morph before skin before the one refit, and only when asked."""
    from tauray_amd import _lib, renderer as R
    from tauray_amd.animation import SceneAnimator
    from tauray_amd.gltf import load_glb
    fake = _RecordingLibrary()
    monkeypatch.setattr(_lib, "lib", lambda: fake)

    class Handle:
        h = None
    scene = load_glb(os.path.join(GOLDEN, "morph.glb"), 48, 32)
    assert len(scene.morphed) == 3 and len(scene.skinned) == 1

    def frame(ss, **kw):
        an = SceneAnimator(scene)
        an.play("")
        fake.calls.clear()
        ss.animate(an, 0, **kw)
        calls = [c for c in fake.calls if c in ("latch_positions", "morph", "skin", "refit_accel", "build_accel")]
        fake.calls.clear()
        ss.pose(an.node_globals, **kw)
        return calls, [c for c in fake.calls if c in ("latch_positions", "morph", "skin", "refit_accel", "build_accel")]
    plain = ["morph"] * 3 + ["skin", "refit_accel"]
    ss = R.SceneStage(Handle(), scene)
    assert fake.calls[:2] == ["upload", "set_deformation_motion 0"] and "latch_positions" not in fake.calls
    assert frame(ss) == (plain, ["skin", "refit_accel"])
    assert frame(ss, deformation_motion=True) == (["latch_positions"] + plain, ["latch_positions", "skin", "refit_accel"])
    ss.set_deformation_motion(True)
    assert frame(ss) == (["latch_positions"] + plain, ["latch_positions", "skin", "refit_accel"])
    assert frame(ss, deformation_motion=False) == (plain, ["skin", "refit_accel"])
    fake.calls.clear()
    ss = R.SceneStage(Handle(), scene, deformation_motion=True)
    assert fake.calls[:2] == ["upload", "set_deformation_motion 1"]
    posed = [c for c in fake.calls if c in ("latch_positions", "morph", "skin", "build_accel")]
    assert posed == ["morph"] * 3 + ["skin", "latch_positions", "build_accel"]      # the rest pose is the first previous pose
    assert frame(ss, refit=False) == (["latch_positions"] + plain[:-1] + ["build_accel"], ["latch_positions", "skin", "build_accel"])


# =========================================================================================================================== GPU
def _feature(R, ctx, ss, fid, size=SIZE):
    from test_accel_strategies import _dup
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    R.FeatureStage(ctx, ss, fid, _dup(size)).run(buf)
    out = buf.download((size[1], size[0], 4))
    buf.free()
    return out


def _refused(R, text, fn, *a, **kw):
    with pytest.raises(R.TrhipError) as e:
        fn(*a, **kw)
    assert text in str(e.value), str(e.value)


# ---- 1. the plane, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("strategy, refit", [(ALL, True), (ALL, False), (PER_MESH, True), (PER_MESH, False)])
def test_the_plane_bit_for_bit(R, ctx, strategy, refit):
    """Skinned spans of 1, 255, 256, 257 and 775 vertices, a static span, morphed spans of the same sizes, a span that is morphed and
    skinned and a skinned span two instances share: pose A, latch, pose B."""
    from tauray_amd.scene import SKIN
    rng = np.random.default_rng(40)
    meshes, dpos = [], {}
    for k, vc in enumerate(VERTEX_COUNTS + (40,) + VERTEX_COUNTS + (300, BT + 1)):
        v, d, _, _ = MM.random_mesh(500 + k, vc, 2, False, False)
        meshes.append((v, _strip_indices(vc)))
        dpos[k] = d
    n = len(VERTEX_COUNTS)
    skinned, static, morphed, both, shared = list(range(n)), n, list(range(n + 1, 2 * n + 1)), 2 * n + 1, (2 * n + 2, 2 * n + 3)
    sc = _scene(meshes, uses=list(range(len(meshes))) + [len(meshes) - 1])
    instances = len(sc.instances)
    assert instances == shared[1] + 1 and tuple(sc.spans[shared[0]]) == tuple(sc.spans[shared[1]])
    ss = R.SceneStage(ctx, sc, as_strategy=strategy, deformation_motion=True)
    uploaded = [ss.vertices(i)["pos"].copy() for i in range(instances)]
    assert all(np.array_equal(uploaded[i], meshes[min(i, len(meshes) - 1)][0]["pos"]) for i in range(instances))
    previous = lambda: [ss.previous_positions(i) for i in range(instances)]
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert same(previous(), uploaded)                                   # the fill: previous = current
    for i in skinned + [both, shared[0]]:
        skins = np.zeros(len(uploaded[i]), dtype=SKIN)
        skins["joints"][:, 1] = 1
        skins["weights"][:, 0] = rng.uniform(0, 1, len(skins))
        skins["weights"][:, 1] = f32(1) - skins["weights"][:, 0]
        ss.set_skin(i, skins)
    for i in morphed + [both]:
        ss.set_morph_targets(i, dpos[i])
    assert same(previous(), uploaded)

    def pose(seed):
        r = np.random.default_rng(seed)
        joints = np.stack([np.eye(4), np.eye(4)]).astype(f32)
        joints[:, :3, :3] += r.uniform(-0.2, 0.2, (2, 3, 3))
        joints[:, :3, 3] = r.uniform(-0.5, 0.5, (2, 3))
        w = r.uniform(-1, 1, 2).astype(f32)
        for i in morphed + [both]:
            ss.morph(i, w, refit=None)
        for i in skinned + [both, shared[0]]:
            ss.skin(i, joints, refit=None)
        ss._accel_after_change(refit)
        return [ss.vertices(i)["pos"].copy() for i in range(instances)], w
    deforming = skinned + morphed + [both] + list(shared)
    pose_a, w_a = pose(1)
    assert same(previous(), uploaded)                                   # nothing is kept before the first latch
    ss.latch_positions()
    pose_b, _ = pose(2)
    got = previous()
    for i in deforming:
        assert got[i].tobytes() == pose_a[i].tobytes(), i
        assert pose_a[i].tobytes() != pose_b[i].tobytes() and pose_a[i].tobytes() != uploaded[i].tobytes(), i
    assert got[static].tobytes() == uploaded[static].tobytes() == pose_b[static].tobytes()
    # instances that share a span have one plane; the morphed and skinned span holds the skinned result, not the skin's source
    assert got[shared[0]].tobytes() == got[shared[1]].tobytes() == pose_a[shared[1]].tobytes()
    assert MM.morph(meshes[both][0], w_a, dpos[both])["pos"].tobytes() != got[both].tobytes()
    pose(3)                                                             # two poses between two latches leave the plane alone
    assert same(pose(2)[0], pose_b) and same(previous(), got)
    ss.latch_positions()                                                # a latch without a new pose: previous = current
    assert same(previous(), pose_b)
    motion = _feature(R, ctx, ss, 6)
    hit = np.isfinite(motion[..., 0])
    assert hit.sum() > 20 and float(np.abs(motion[hit][:, :3]).max()) <= 1e-5
    ss.set_deformation_motion(False)
    _refused(R, "trhip_scene_get_previous_positions: deformation motion is off", ss.previous_positions, 0)
    ss.latch_positions()                                                # succeeds and does nothing
    ss.set_deformation_motion(True)
    assert same(previous(), pose_b)                                     # on again: filled from the current vertices


@pytest.mark.gpu
def test_refusals_on_the_device(R):
    from tauray_amd import _lib
    fresh = R.Context(0)
    out = np.zeros((4, 3), f32)
    L = _lib.lib()
    assert L.trhip_scene_set_deformation_motion(fresh.h, 1) == 0 and L.trhip_scene_latch_positions(fresh.h) == 0      # kept for the upload to come
    assert "trhip_scene_get_previous_positions: no scene" in _refusal(L.trhip_scene_get_previous_positions, fresh.h, 0, out.ctypes.data, 4)
    assert "trhip_scene_get_previous_positions: null output" in _refusal(L.trhip_scene_get_previous_positions, fresh.h, 0, None, 4)
    sheet = _sheet(3)
    ss = R.SceneStage(fresh, _scene([sheet]), deformation_motion=True)
    assert "trhip_scene_get_previous_positions: instance out of range" in _refusal(L.trhip_scene_get_previous_positions, fresh.h, 1, out.ctypes.data, 4)
    assert L.trhip_scene_get_previous_positions(fresh.h, 0, out.ctypes.data, 4) == 0 and np.array_equal(out, sheet[0]["pos"][:4])
    assert np.array_equal(ss.previous_positions(0), sheet[0]["pos"])
    fresh.close()


# ---- 2. affine deformations against the unchanged oracle
def _deform(ss, case, refit):
    """Pose A, latch, pose B of the affine scene's sheet; returns the affine map from the current to the previous pose."""
    base = _sheet()[0]
    if case == "skin":
        ss.set_skin(0, _one_joint_skins(len(base)))
        ss.skin(0, np.array([JOINT_A], f32), refit=True)
        ss.latch_positions()
        ss.skin(0, np.array([JOINT_B], f32), refit=refit)
        return DM.affine_between(JOINT_A, JOINT_B)
    ss.set_morph_targets(0, _affine_delta(base))
    ss.morph(0, np.array([WEIGHT_A], f32), refit=True)
    ss.latch_positions()
    ss.morph(0, np.array([WEIGHT_B], f32), refit=refit)
    return DM.affine_between(morph_pose(WEIGHT_A), morph_pose(WEIGHT_B))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["skin", "morph"])
@pytest.mark.parametrize("strategy, refit", [(ALL, True), (PER_MESH, False)])
def test_affine_deformations_against_the_oracle(R, ctx, oracle, case, strategy, refit):
    """The sheet, every vertex bound to one joint (or morphed by a target that is affine in the base), under a moving instance matrix and
    a moving camera.  The oracle gets the current deformed vertices as a static mesh and model_prev * A in place of model_prev."""
    from tauray_amd.scene import to_glm
    sc, (base, _) = _affine_scene()
    ss = R.SceneStage(ctx, sc, as_strategy=strategy, deformation_motion=True)
    A = _deform(ss, case, refit)
    previous_camera = _camera(CAMERA_PREV)
    ss.set_previous_cameras([previous_camera])
    current = ss.vertices(0)
    assert np.array_equal(ss.previous_positions(0), (A[:3, :3] @ current["pos"].astype(np.float64).T).T + A[:3, 3]), "the plane is A * current, exactly"
    static = copy.copy(sc)
    static.vertices = sc.vertices.copy()
    static.vertices[:len(base)] = current
    static.instances = sc.instances.copy()
    static.instances["model_prev"][0] = to_glm((MODEL_PREV @ A).astype(f32))
    osc = oracle.OracleScene(static)
    osc.set_previous_cameras([previous_camera])
    assert np.array_equal(_bits(_feature(R, ctx, ss, 5)), _bits(osc.render_feature(5, *SIZE)))      # the same hits, bit for bit
    on = {fid: _feature(R, ctx, ss, fid) for fid in (6, 7, 8)}
    ss.set_deformation_motion(False)
    off = {fid: _feature(R, ctx, ss, fid) for fid in (6, 7, 8)}
    for fid in (6, 7, 8):
        ref = osc.render_feature(fid, *SIZE)
        hit = np.isfinite(ref)
        assert hit[..., 0].sum() > 500 and np.array_equal(hit, np.isfinite(on[fid])) and np.array_equal(hit, np.isfinite(off[fid]))
        bound = motion_bound(ref[hit])
        err = float(np.abs(on[fid][hit] - ref[hit]).max())
        print(f"\n{case}, strategy {strategy}: feature {fid}: largest error {err:.3e}, bound {bound:.3e}, switch off differs by {float(np.abs(off[fid][hit] - on[fid][hit]).max()):.3e}")
        assert err <= bound, f"feature {fid}"                          # every pixel, none left out
        assert float(np.abs(off[fid][hit] - on[fid][hit]).max()) > 10 * bound, f"feature {fid}: the rigid motion would pass too"


# ---- 3. the other consumers
@pytest.mark.gpu
def test_path_tracer_targets_and_programs(R, ctx):
    """The screen_motion target is feature 8 with the switch on as it is with the switch off, and the compiled program renders the bits of
    the general kernels in both shading arithmetics."""
    from test_accel_strategies import _dup
    sc, _ = _affine_scene()
    ss = R.SceneStage(ctx, sc, deformation_motion=True)
    _deform(ss, "skin", True)
    ss.set_previous_cameras([_camera(CAMERA_PREV)])
    names = ["color", "screen_motion", "instance_id"]

    def targets(ieee=None, specialize=None):
        pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=2), _dup(SIZE))
        if ieee is not None:
            pt.set_shading_arithmetic(ieee)
        if specialize is not None:
            pt.set_specialization(specialize)
        bufs = {n: ctx.alloc(SIZE[0] * SIZE[1] * R.PathTracerStage.TARGETS[n][0] * 4).zero() for n in names}
        pt.run_targets(bufs)
        out = {n: bufs[n].download((SIZE[1], SIZE[0], R.PathTracerStage.TARGETS[n][0]), R.PathTracerStage.TARGETS[n][1]) for n in names}
        pt.close()
        return out
    agreement = {}
    for on in (True, False):
        ss.set_deformation_motion(on)
        t, f8 = targets(), _feature(R, ctx, ss, 8)
        surface = t["instance_id"][..., 0] >= 0
        assert surface.sum() > 500 and np.array_equal(surface, np.isfinite(f8[..., 0]))
        agreement[on] = (np.array_equal(_bits(t["screen_motion"][surface]), _bits(f8[surface][:, :2])), float(np.abs(t["screen_motion"][surface] - f8[surface][:, :2]).max()), t)
        for ieee in (True, False):
            a, b = targets(ieee, True), targets(ieee, False)
            assert all(np.array_equal(_bits(a[n]), _bits(b[n])) for n in names), f"switch {on}, ieee {ieee}"
    (equal_on, far_on, _), (equal_off, far_off, _) = agreement[True], agreement[False]
    print(f"\nscreen_motion against feature 8: switch on bit-equal {equal_on}, largest difference {far_on:.3e}; switch off {equal_off}, {far_off:.3e}")
    assert equal_on == equal_off and far_on <= 1e-5 and far_off <= 1e-5      # 1e-5: what the target is held to against the oracle (test_gpu_parity.py)
    sheet = agreement[True][2]["instance_id"][..., 0] == 0
    assert float(np.abs(agreement[True][2]["screen_motion"][sheet] - agreement[False][2]["screen_motion"][sheet]).max()) > 1e-3


@pytest.mark.gpu
def test_restir_di_reuses_the_reservoirs_of_the_same_surface_points(R, ctx):
    """ReSTIR DI with temporal reuse on the single-joint sheet moved by its joint, against the same sheet moved by its instance matrix:
    the pixel a pixel's history is fetched from and whether a previous reservoir was found there (the comparison tests/test_restir_di.py
    makes between kernel and model for reprojected pixels).  A pixel whose reprojected position lies within 1e-3 of a pixel boundary may
    round either way and is left out; at most 1 % of the frame may be."""
    from tauray_amd.scene import to_glm
    # temporal_edge_detection (restir_di.hip) reuses a reservoir only where the surface point moved less than a hundredth of its distance
    # from the camera, 0.06 here: the sheet moves by (1/32, 1/32, 0), which is 0.458 of a 64 x 64 frame's pixels (2 * 6 * tan(20 deg) / 64
    # world units each) along both axes
    move_a, move_b = np.eye(4), DM.rigid(0, (0.03125, 0.03125, 0.0))
    sheet, wall = _sheet(), _sheet(3, 2.0)
    back = DM.rigid(0, (0.0, 0.0, -1.5))
    options = dict(candidates=4, spatial_samples=0, temporal_reuse=True, rng_seed=3)

    def frames(ss, step):
        st = R.RestirDiStage(ctx, ss, SIZE, 1, R.restir_di_options(record=True, **options))
        out = ctx.alloc(SIZE[0] * SIZE[1] * 16).zero()
        st.run([0], out)
        step()
        st.run([0], out)
        rec = st.download("temporal")[0]
        st.close()
        out.free()
        return rec, _feature(R, ctx, ss, 9)[..., 0], _feature(R, ctx, ss, 8)

    def by_joint(on):
        sc = _scene([sheet, wall], models=[np.eye(4), back])
        ss = R.SceneStage(ctx, sc, deformation_motion=on)
        ss.set_skin(0, _one_joint_skins(len(sheet[0])))
        ss.skin(0, np.array([move_a], f32), refit=True)

        def step():
            ss.latch_positions()
            ss.skin(0, np.array([move_b], f32), refit=True)
        return frames(ss, step)

    def by_instance():
        sc = _scene([sheet, wall], models=[move_a, back])
        ss = R.SceneStage(ctx, sc)

        def step():
            inst = sc.instances.copy()
            inst["model"][0] = to_glm(move_b)
            inst["model_prev"][0] = to_glm(move_a)
            ss.update_instances(inst, refit=True)
        return frames(ss, step)
    joint, ids, f8 = by_joint(True)
    instance, ids_i, _ = by_instance()
    assert np.array_equal(ids, ids_i, equal_nan=True)
    on_sheet = ids == 0
    m = np.stack([f8[..., 0], 1.0 - f8[..., 1]], -1) * np.array(SIZE, f32) - 0.5      # restir_di.h: the reprojected pixel is int(m)
    near = (np.abs(m - np.round(m)) < 1e-3).any(-1) & on_sheet
    assert on_sheet.sum() > 300 and near.sum() <= 0.01 * SIZE[0] * SIZE[1]
    keep = on_sheet & ~near
    for name in ("px", "py"):
        assert np.array_equal(joint[name][keep], instance[name][keep]), name
    assert np.array_equal(joint["reuse"][keep] != 0, instance["reuse"][keep] != 0)
    # a pixel of this frame is 0.068 world units wide, more than the 0.06 the edge detection allows: a reservoir is reused where both
    # roundings pick the pixel itself, with probability 0.542^2 = 0.29; half of that share shows that history is found at all
    assert (joint["reuse"][keep] != 0).mean() > 0.14, "no history found on the sheet"
    rigid_only, _, _ = by_joint(False)
    moved = (rigid_only["px"][keep] != instance["px"][keep]) | (rigid_only["py"][keep] != instance["py"][keep])
    # the reprojected pixel is rounded up or down at random: a motion of 0.458 pixels moves it with probability 1 - 0.542^2 = 0.71; with the
    # switch off the history is fetched from where the sheet would be had it not deformed, the pixel itself - half of that share shows it
    assert moved.mean() > 0.35, float(moved.mean())


# ---- 4. nothing else moves
def _everything(R, ctx, ss, scene):
    from test_accel_strategies import _dup
    out = [_feature(R, ctx, ss, fid) for fid in (6, 7, 8)]
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=3), _dup(SIZE))
    T = R.PathTracerStage.TARGETS
    bufs = {n: ctx.alloc(SIZE[0] * SIZE[1] * T[n][0] * 4).zero() for n in T}
    pt.run_targets(bufs)
    out += [bufs[n].download((SIZE[1], SIZE[0], T[n][0]), T[n][1]) for n in sorted(T)]
    pt.close()
    return out


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.gpu
def test_nothing_else_moves(R, ctx):
    from tauray_amd.gltf import load_glb
    scene = load_glb(os.path.join(GOLDEN, "test.glb"), *SIZE)
    assert not scene.skinned and not scene.morphed
    ss = R.SceneStage(ctx, scene)
    cam = copy.deepcopy(scene.cameras[0])
    cam.transform = np.array(cam.transform, dtype=np.float64) @ DM.rigid(0, (0.125, 0.0, 0.0))
    ss.set_previous_cameras([cam])
    never = _everything(R, ctx, ss, scene)
    assert np.isfinite(never[2][..., 0]).sum() > 500
    ss.set_deformation_motion(True)
    ss.latch_positions()
    assert _same(_everything(R, ctx, ss, scene), never), "a scene without deforming meshes renders the same bits with the switch on"
    ss.set_deformation_motion(False)
    assert _same(_everything(R, ctx, ss, scene), never)
    # a deforming scene: on, then off, is never on
    sc, (base, _) = _affine_scene()
    plain = R.SceneStage(ctx, sc)
    plain.set_skin(0, _one_joint_skins(len(base)))
    plain.skin(0, np.array([JOINT_A], f32), refit=True)
    plain.skin(0, np.array([JOINT_B], f32), refit=True)
    never = _everything(R, ctx, plain, sc)
    ss = R.SceneStage(ctx, sc, deformation_motion=True)
    _deform(ss, "skin", True)
    assert not _same(_everything(R, ctx, ss, sc)[:3], never[:3])
    ss.set_deformation_motion(False)
    assert _same(_everything(R, ctx, ss, sc), never)
    # an upload with the switch on refills the plane
    ss.set_deformation_motion(True)
    moved = copy.copy(sc)
    moved.vertices = sc.vertices.copy()
    moved.vertices["pos"][:, 2] += f32(0.25)
    ss.set_scene(moved)
    assert np.array_equal(ss.previous_positions(0), moved.vertices["pos"][:len(base)]) and np.array_equal(ss.previous_positions(1), moved.vertices["pos"][len(base):])


# ---- 5. hosts
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["skinned.glb", "morph.glb", "animated.glb"])
def test_both_hosts(R, ctx, tmp_path, name):
    """`tauray_hip FILE --animation --temporal-reprojection=0.75 --deformation-motion --frames=4 --filetype=raw` against RtRenderer with the
    same options playing the same file, bit for bit; and both differ from the run without the flag - on morph.glb.  skinned.glb has a
    skin and a bent rest pose but no animation clip: nothing deforms between its frames, so there the flag must change nothing (the rest
    pose, not the uploaded bind pose, is the first previous pose).  animated.glb is that file with clips that turn two joints of its skin
    (tools/make_animated_glb.py): latch, then skin, with no morph target in play.  Its two animators differ in the last bits of a matrix, so
    the hosts are compared there the way tests/test_bmfr.py compares them on this file - at most 0.2 % of the pixels more than 1e-3 apart,
    means within 1e-4 - and the flag has to move ten times that share of the pixels by more than 1e-3."""
    from tauray_amd.animation import SceneAnimator
    from tauray_amd.gltf import load_glb
    W, H = SIZE
    glb = os.path.join(GOLDEN, name)
    common = [CLI, glb, f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--animation", "--framerate=4", "--temporal-reprojection=0.75", "--frames=4", "--filetype=raw",
              "--format=rgba32"]
    subprocess.check_call(common + ["--deformation-motion", f"--headless={tmp_path / 'on'}"])
    subprocess.check_call(common + [f"--headless={tmp_path / 'off'}"])

    def play(flag):
        scene = load_glb(glb, W, H)
        r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), temporal_reprojection=0.75, deformation_motion=flag)
        an = SceneAnimator(scene)
        an.play("")
        playing = an.is_playing()
        out = []
        for frame in range(4):
            if playing:
                r.scene_update.animate(an, 0 if frame == 0 else 250000, refit=(frame % 3 != 2))
            r.render()
            out.append(r.download("display")[0].copy())
        r.close()
        return out
    on, off = play(True), play(False)
    for frame in range(4):
        for which, ref in (("on", on), ("off", off)):
            got = np.fromfile(f"{tmp_path / which}{frame}.raw", dtype=np.float32).reshape(H, W, 4)
            if name == "animated.glb":
                differing = float((np.abs(got - ref[frame]).max(-1) > 1e-3).mean())
                print(f"\n{name} {which} frame {frame}: {differing:.4%} of the pixels differ between the hosts")
                assert differing < 2e-3 and abs(float(got.mean()) - float(ref[frame].mean())) < 1e-4, (which, frame, differing)
            else:
                assert np.array_equal(_bits(got), _bits(ref[frame])), (which, frame)
    if name == "animated.glb":
        moved = max(float((np.abs(a - b).max(-1) > 1e-3).mean()) for a, b in zip(on, off))
        print(f"\n{name}: the flag moves {moved:.4%} of the pixels of the most affected frame")
        assert moved > 2e-2, moved
    changed = any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(on, off))
    assert changed == bool(load_glb(glb, W, H).animations), "the flag changes the frames of a file that deforms, and of no other"
