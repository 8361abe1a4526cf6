"""The Looking Glass output: the composition stage (trhip_lkg_*, csrc/looking_glass.hip) against
tests/looking_glass_model.py, a numpy model written from the rule of include/trhip.h, the camera rig of both hosts, and the hosts' chains.

How the bounds are set.  Nothing is compared against a figure taken from the code under test.
 * View indices: the order of operations is pinned (csrc/looking_glass.h), so the stage's recorded indices equal the float32 model's exactly.
   Between the float32 and the float64 model an index may differ where fract(d) * N lies within float rounding of a whole number: at most
   0.5 % of the (pixel, channel) entries.
 * dst: on the entries where the two models pick the same view, the stage may be four times as far from the float64 model as the float32
   model is on the same input: another equally valid float32 evaluation order moves results by about that much.
 * Views of one constant colour v: a bilinear sum of four equal taps is v up to the rounding of (1 - w), two products and a sum per level,
   two levels: 8 * 2^-24 covers it for v <= 1.
 * The rig: ndc.x of the point of convergence is compared at 1e-5, the bound of the issue; the cameras' packed matrices are float32.
Measured figures: profiles/r14/looking_glass.txt.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import looking_glass_model as M

EXE = os.path.join(ROOT, "tauray_amd", "tauray_hip")
MISMATCH_CAP = 0.005
# the calibrations of two panels (pitch, slope, center, viewCone, invView, DPI); the screen size is the case's
PORTRAIT = (52.57, -7.19, 0.13, 40.0, True, 324.0)
LANDSCAPE = (49.825, 5.2, 0.18, 40.0, True, 283.0)


def _cal(values, size, invert=None):
    from tauray_amd.looking_glass import LookingGlassCalibration
    pitch, slope, center, cone, inv, dpi = values
    return LookingGlassCalibration(pitch, slope, center, cone, inv if invert is None else invert, dpi, size[0], size[1])


def _opts(cal, n):
    o = cal.stage_options(n)
    return (n, o["pitch"], o["tilt"], o["center"], o["invert"])


def _glb(name, size):
    from tauray_amd.gltf import load_glb
    return load_glb(os.path.join(GOLDEN, name), size[0], size[1])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ======================================================================================================================
# CPU 1: the boundary
LKG_SYMBOLS = ("trhip_lkg_create", "trhip_lkg_destroy", "trhip_lkg_run", "trhip_lkg_get_timings", "trhip_lkg_download")


def test_lkg_symbols_resolve_and_create_refuses_bad_arguments():
    from tauray_amd import _lib
    L = _lib.lib()
    for n in LKG_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.LkgOptionsC) == 24 and C.sizeof(_lib.LkgTimingsC) == 72
    out = C.c_void_p()

    def err(opt, vw, vh, ow, oh):
        rc = L.trhip_lkg_create(None, C.byref(opt) if opt is not None else None, vw, vh, ow, oh, C.byref(out))
        assert rc != 0 and not out.value
        return L.trhip_last_error().decode()
    good = lambda **kw: _lib.LkgOptionsC(**dict(dict(viewport_count=8, pitch=15.4, tilt=-0.18, center=0.13, invert=1, record_view_indices=0), **kw))
    for sizes in ((0, 32, 96, 128), (24, 0, 96, 128), (24, 32, 0, 128), (24, 32, 96, 0)):
        assert "zero" in err(good(), *sizes)
    assert "viewport_count" in err(good(viewport_count=0), 24, 32, 96, 128) and "viewport_count" in err(good(viewport_count=256), 24, 32, 96, 128)
    assert "finite" in err(good(pitch=float("nan")), 24, 32, 96, 128) and "finite" in err(good(center=float("inf")), 24, 32, 96, 128)
    assert "options" in err(None, 24, 32, 96, 128)
    assert "device" in err(good(), 24, 32, 96, 128) and "device" in err(good(viewport_count=255, invert=0), 2, 2, 130, 3)     # good arguments, no device: no CPU fallback
    assert L.trhip_lkg_run(None, None, None, None, None) != 0 and L.trhip_lkg_download(None, 0, None, 0) != 0


def test_renderer_refuses_a_multi_device_looking_glass_output():
    from tauray_amd import renderer as R
    from tauray_amd.looking_glass import LookingGlassOutput
    lg = LookingGlassOutput(_cal(PORTRAIT, (96, 128)), 8)
    opt = R.make_options()
    for shard in ("pixels", "views", "samples"):
        with pytest.raises(ValueError, match="would have to be gathered first"):
            R.RtRenderer(None, None, opt, (48, 64), world_size=2, rank=0, shard=shard, looking_glass=lg)
    with pytest.raises(ValueError, match="frames_per_launch must be 1"):
        R.RtRenderer(None, None, opt, (48, 64), looking_glass=lg, frames_per_launch=2)
    with pytest.raises(ValueError, match="the rig has 8 views"):
        R.RtRenderer(None, None, opt, (48, 64), looking_glass=lg, viewports=4)
    with pytest.raises(ValueError, match="perspective"):
        R.RtRenderer(None, None, R.make_options(projection=1), (48, 64), looking_glass=lg)
    with pytest.raises(ValueError, match="1..255"):
        LookingGlassOutput(_cal(PORTRAIT, (96, 128)), 256)
    with pytest.raises(ValueError, match="not an option"):
        R.LookingGlassStage(None, (24, 32), (96, 128), dict(bogus=1))


CALIBRATION_ARG = "--lkg-calibration=0,52.57,-7.19,0.13,0,40,1,0,324,96,128,0,0,0"


def test_cli_knows_the_looking_glass_options():
    h = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    for word in ("--display=headless|looking-glass", "--lkg-params=", "--lkg-calibration="):
        assert word in h.stdout + h.stderr, word
    glb = os.path.join(GOLDEN, "test.glb")
    lg = ["--display=looking-glass"]
    for args, word in ((lg, "no display service is read here"), (["--display=openxr"], "not built"), (["--display=window"], "not built"),
                       (["--display=frame-server"], "not built"), (["--display=bogus"], "headless or looking-glass"),
                       (lg + [CALIBRATION_ARG, "--fake-devices=2"], "gathered first"),
                       (lg + [CALIBRATION_ARG, "--shard=views", "--process-count=2", "--process-rank=0"], "gathered first"),
                       (lg + [CALIBRATION_ARG, "--frames-per-launch=2"], "frames-per-launch"),
                       (lg + [CALIBRATION_ARG, "--camera-grid=2,1,0.1,0.1"], "camera-grid"),
                       (lg + [CALIBRATION_ARG, "--lkg-params=300"], "1..255"), (lg + [CALIBRATION_ARG, "--lkg-params=8,bogus=2"], "not one of its fields"),
                       (lg + ["--lkg-calibration=0,52.57,-7.19"], "screenW"), (lg + ["--lkg-calibration=0,x"], "not a number")):
        r = subprocess.run([EXE, glb, "--width=24", "--height=32", "--headless=/dev/null"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


def test_option_parsers_of_the_python_host():
    from tauray_amd import looking_glass as LG
    c = LG.parse_calibration(CALIBRATION_ARG.split("=", 1)[1])
    assert c == _cal(PORTRAIT, (96, 128)) and c.size == (96, 128)
    named = LG.parse_calibration("0,52.57,-7.19,center=0.13,viewCone=40,invView=1,DPI=324,screenW=96,screenH=128")
    assert named == c
    p = LG.parse_params("8,midplane=3", c)
    assert (p.viewports, p.midplane, p.depth, p.relative_dist) == (8, 3.0, 2.0, 2.0)
    d = LG.LookingGlassOutput(c)
    assert (d.viewports, d.midplane, d.depth, d.relative_dist) == (48, 2.0, 2.0, 2.0)
    # corrected_pitch = screen_w / dpi * pitch * sin(atan(|slope|)), tilt = screen_h / (screen_w * slope)
    assert abs(c.corrected_pitch - 96 / 324.0 * 52.57 * np.sin(np.arctan(7.19))) < 1e-5 and abs(c.tilt - 128 / (96 * -7.19)) < 1e-7
    with pytest.raises(ValueError, match="not one of its fields"):
        LG.parse_calibration("0,1,2,bogus=3")
    for text, word in (("8.5", "whole number"), ("0", "1..255"), ("300", "1..255"), ("8,0", "at least 0.001"), ("8,2,2,2,2", "more than 4")):      # what the CLI refuses
        with pytest.raises(ValueError, match=word):
            LG.parse_params(text, c)
    with pytest.raises(ValueError, match="screenW"):
        LG.parse_calibration("0,52.57,-7.19")


# ======================================================================================================================
# CPU 2: the model against closed forms
def _random_views(n, size, seed=3, lo=-0.2, hi=1.3):
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo, hi, (n, size[1], size[0], 4)).astype(np.float32)
    v[..., 3] = 1.0
    return v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_one_view_is_its_bilinear_resample(dtype):
    for out_size, view_size in (((37, 23), (7, 5)), ((64, 64), (64, 64)), ((5, 9), (11, 3))):
        views = _random_views(1, view_size)
        out, idx = M.compose(views, out_size, *_opts(_cal(PORTRAIT, out_size), 1), dtype=dtype)
        assert not idx.any()
        want = M.resample(views[0], out_size, dtype)
        assert np.array_equal(out[..., :3], want[..., :3]) and (out[..., 3] == 1).all()
        if out_size == view_size:
            assert np.array_equal(out[..., :3], views[0][..., :3].astype(dtype))      # texel centres on pixel centres: a copy
    # ... and the resample is the textbook one: a ramp comes back as a ramp away from the clamped border
    ramp = np.zeros((1, 4, 8, 4), np.float32)
    ramp[0, :, :, 0] = np.arange(8)[None, :]
    out, _ = M.compose(ramp, (16, 4), *_opts(_cal(PORTRAIT, (16, 4)), 1))
    x = (np.arange(16) + 0.5) / 16 * 8 - 0.5
    assert np.allclose(out[0, :, 0], np.clip(x, 0, 7), atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_constant_views_show_their_index(dtype):
    n, out_size = 8, (96, 128)
    views = np.ones((n, 32, 24, 4), np.float32) * ((np.arange(n, dtype=np.float32) + 1) / n)[:, None, None, None]
    out, idx = M.compose(views, out_size, *_opts(_cal(PORTRAIT, out_size), n), dtype=dtype)
    want = (idx[..., :3].astype(np.float64) + 1) / n
    assert np.abs(out[..., :3] - want).max() <= 8 * 2.0 ** -24
    assert len(np.unique(idx[..., :3])) == n, "every view shows somewhere"
    assert (idx[..., 0] != idx[..., 2]).mean() > 0.2, "the sub-pixels of a pixel come from different views"


def test_model_invert_negates_the_calibration():
    n, out_size = 8, (96, 128)
    cal = _cal(PORTRAIT, out_size, invert=False)
    o, oi = _opts(cal, n), _opts(_cal(PORTRAIT, out_size, invert=True), n)
    for dtype in (np.float32, np.float64):
        a, b = M.calibration_vector(*o[1:], out_size[0], dtype), M.calibration_vector(*oi[1:], out_size[0], dtype)
        assert np.array_equal(a, -b) and a[0] == dtype(np.float32(cal.corrected_pitch)) and a[3] == -dtype(np.float32(cal.center))
        assert a[1] == dtype(np.float32(cal.tilt)) * dtype(np.float32(cal.corrected_pitch)) and a[2] == a[0] / (dtype(3) * dtype(96))
    # fract(-d) = 1 - fract(d): the views mirror, but for the entries that sit on a boundary
    plain, mirrored = M.view_indices(out_size, *o)[..., :3].astype(int), M.view_indices(out_size, *oi)[..., :3].astype(int)
    assert (plain + mirrored == n - 1).mean() > 0.999


def test_model_center_shifted_by_one_changes_nothing():
    n, out_size = 8, (96, 128)
    views = _random_views(n, (24, 32))
    pitch, tilt = _opts(_cal(PORTRAIT, out_size), n)[1:3]
    a, ia = M.compose(views, out_size, n, pitch, tilt, 0.125, True)           # 0.125 and 1.125 are float32 numbers: d moves by exactly 1
    b, ib = M.compose(views, out_size, n, pitch, tilt, 1.125, True)
    same = (ia == ib).all(-1)
    assert same.mean() >= 1 - 1e-4, "beyond float rounding"
    assert np.array_equal(a[same], b[same])


CASES_32_64 = [((96, 128), 8, PORTRAIT), ((37, 23), 5, PORTRAIT), ((1536, 2048), 48, PORTRAIT), ((3840, 2160), 45, LANDSCAPE)]


@pytest.mark.parametrize("out_size,n,panel", CASES_32_64, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 2 else None)
def test_float32_model_picks_the_views_of_the_float64_model(out_size, n, panel):
    o = _opts(_cal(panel, out_size), n)
    a, b = M.view_indices(out_size, *o, dtype=np.float32), M.view_indices(out_size, *o, dtype=np.float64)
    share = float((a[..., :3] != b[..., :3]).mean())
    print(f"\n{out_size[0]}x{out_size[1]} / {n} views: the float32 and float64 models pick different views on {share:.3e} of the (pixel, channel) entries")
    assert share <= MISMATCH_CAP
    assert int(np.abs(a[..., :3].astype(int) - b[..., :3]).max()) in (0, 1, n - 1), "a differing entry sits on a boundary between neighbouring views"


# ======================================================================================================================
# CPU 3: the cameras
RIGS = [(8, 2.0, 0.5, 2.0), (5, 1.5, 1.0, 3.0), (48, 2.0, 2.0, 2.0)]      # viewports, midplane, depthiness, relative_dist


def _rig(scene, rig, cal):
    from tauray_amd.looking_glass import looking_glass_cameras
    return looking_glass_cameras(scene, *rig, cal)


def test_python_rig_is_the_rule_at_float64():
    from tauray_amd.scene import perspective_matrix
    cal = _cal(PORTRAIT, (1536, 2048))
    for rig in RIGS:
        n, midplane, depth, rd = rig
        scene = _glb("test.glb", (48, 64))
        frame = np.array(scene.cameras[0].transform, dtype=np.float64)
        cams = _rig(scene, rig, cal)
        assert len(cams) == n == len(scene.cameras)
        vfov = np.degrees(2 * np.arctan(1 / (2 * rd)))
        for i, cam in enumerate(cams):
            offset = ((i + 0.5) / n) * 2 - 1
            pan = -np.tan(np.radians(offset * cal.view_cone * depth))
            P = perspective_matrix(vfov, 1536 / 2048, 0.01, 300.0)
            P[0, 2] = pan
            d = P @ np.array([0, 0, 1.0, 1.0])
            d = d / d[2]
            local = np.eye(4)
            local[:3, 3] = midplane * d[:3]
            assert abs(cam.fov - vfov) < 1e-12 and abs(cam.aspect - 0.75) < 1e-15 and (cam.near, cam.far) == (0.01, 300.0)
            assert abs(cam.fov_offset[0] - pan) < 1e-12 * max(1, abs(pan)) and cam.fov_offset[1] == 0
            assert np.abs(np.array(cam.transform) - frame @ local).max() < 1e-12
            packed = cam.pack()
            assert np.abs(packed["pan"][0] - np.array([pan, 0, 0, 0])).max() < 1e-6 * max(1, abs(pan))
            assert np.abs(packed["proj_inverse"][0].astype(np.float64).reshape(4, 4).T @ P - np.eye(4)).max() < 1e-5 * max(1, abs(pan))
        # a second rig over the same scene hangs on the same frame, not on the first rig's view 0
        again = _rig(scene, rig, cal)
        assert all(np.array_equal(a.transform, b.transform) for a, b in zip(cams, again))


def test_views_converge_and_the_pan_is_antisymmetric():
    cal = _cal(PORTRAIT, (1536, 2048))
    for rig in RIGS:
        n, midplane = rig[0], rig[1]
        scene = _glb("test.glb", (48, 64))
        frame = np.array(scene.cameras[0].transform, dtype=np.float64)
        cams = _rig(scene, rig, cal)
        data = scene.camera_data()
        vp = [data["view_proj"][i].astype(np.float64).reshape(4, 4).T for i in range(n)]      # glm is column-major

        def ndc_x(i, t):
            c = vp[i] @ (frame @ np.array([0.0, 0.0, t, 1.0]))
            return c[0] / c[3]
        # the point on the rig's axis that the outermost views agree on: bisection on ndc_x(0, t) - ndc_x(n - 1, t) in front of the cameras
        f = lambda t: ndc_x(0, t) - ndc_x(n - 1, t)
        lo, hi = midplane - 100.0 * midplane, midplane - 1e-3 * midplane
        assert f(lo) * f(hi) < 0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if f(lo) * f(mid) > 0 else (lo, mid)
        t = 0.5 * (lo + hi)
        want = ndc_x(0, t)
        worst = max(abs(ndc_x(i, t) - want) for i in range(n))
        print(f"\nrig {rig}: the views converge at z = {t:.6f} of the reference frame, ndc.x = {want:.3e}, worst difference {worst:.3e}")
        assert worst <= 1e-5
        for i in range(n):
            a, b = cams[i], cams[n - 1 - i]
            assert abs(a.fov_offset[0] + b.fov_offset[0]) <= 1e-12 * max(1.0, abs(a.fov_offset[0]))
            la, lb = np.linalg.inv(frame) @ a.transform, np.linalg.inv(frame) @ b.transform
            assert abs(la[0, 3] + lb[0, 3]) < 1e-12 and abs(la[2, 3] - midplane) < 1e-12 and abs(la[1, 3]) < 1e-12
        if n % 2:
            assert cams[n // 2].fov_offset[0] == 0 or abs(cams[n // 2].fov_offset[0]) < 1e-15
        assert cams[0].fov_offset[0] > 0 > cams[-1].fov_offset[0] and cams[0].transform[0][3] != cams[-1].transform[0][3]


def test_cpp_host_packs_the_same_rig(tmp_path):
    from tauray_amd.animation import SceneAnimator
    exe = str(tmp_path / "looking_glass_cameras_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DTAURAY_HIP_WITH_ZLIB", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "looking_glass_cameras_check.cc"), "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz",
                           "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    for name, size, rig, panel, screen in (("test.glb", (48, 64), RIGS[0], PORTRAIT, (96, 128)), ("animated.glb", (96, 54), RIGS[1], LANDSCAPE, (3840, 2160)),
                                           ("test.glb", (420, 560), RIGS[2], PORTRAIT, (1536, 2048))):
        cal = _cal(panel, screen)
        updates = 3
        args = [exe, os.path.join(GOLDEN, name), str(size[0]), str(size[1])] + [repr(v) for v in rig] + \
               [repr(panel[0]), repr(panel[1]), repr(panel[2]), repr(panel[3]), str(int(panel[4])), repr(panel[5]), str(screen[0]), str(screen[1]), str(updates)]
        out = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split("\n")
        tag, bp, bt = out[0].split()
        assert tag == "calibration" and np.array([int(bp, 16), int(bt, 16)], np.uint32).view(np.float32).tolist() == [cal.corrected_pitch, cal.tilt], name
        scene = _glb(name, size)
        _rig(scene, rig, cal)
        animator = SceneAnimator(scene)
        animator.play("", False)
        first = None
        for step in range(updates + 1):
            if step:
                animator.update(0 if step == 1 else 16667)
            tag, s, hexbytes = out[1 + step].split()
            assert tag == "step" and int(s) == step
            mine = scene.camera_data().tobytes()
            assert len(mine) == rig[0] * 320
            assert bytes.fromhex(hexbytes) == mine, f"{name}: the hosts pack different rigs at step {step}"
            first = first or mine
        assert (mine != first) == (name == "animated.glb"), "the rig follows the animation of the first camera's node"


# ======================================================================================================================
# GPU
@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


# (output size, views, view size): ragged tiles and views smaller than a tile; several tiles; one pixel; one view of the output's size
# (texel centres on pixel centres); the most views the stage takes
STAGE_CASES = {"37x23-5": ((37, 23), 5, (7, 5)), "96x128-8": ((96, 128), 8, (24, 32)), "1x1-3": ((1, 1), 3, (3, 2)), "64x64-1": ((64, 64), 1, (64, 64)),
               "130x3-255": ((130, 3), 255, (2, 2))}


@functools.lru_cache(maxsize=None)
def _case(name, invert):
    """The inputs of a case and both models on them, computed once."""
    out_size, n, view_size = STAGE_CASES[name]
    views = _random_views(n, view_size, seed=len(name))
    o = _opts(_cal(PORTRAIT, out_size, invert=invert), n)
    m32, i32 = M.compose(views, out_size, *o, dtype=np.float32)
    m64, i64 = M.compose(views, out_size, *o, dtype=np.float64)
    for a in (views, m32, i32, m64, i64):
        a.setflags(write=False)
    return views, o, m32, i32, m64, i64


def _run_stage(R, ctx, views, out_size, o, record=True, stream=None, stage=None, want=("dst", "dst8")):
    n, pitch, tilt, center, invert = o
    own = stage is None
    stage = stage or R.LookingGlassStage(ctx, (views.shape[2], views.shape[1]), out_size,
                                         dict(viewport_count=n, pitch=pitch, tilt=tilt, center=center, invert=invert, record_view_indices=record))
    src = ctx.alloc(views.nbytes).upload(np.ascontiguousarray(views))
    px = out_size[0] * out_size[1]
    dst = ctx.alloc(px * 16).upload(np.full(px * 4, 7.0, np.float32)) if "dst" in want else None
    dst8 = ctx.alloc(px * 4).upload(np.full(px * 4, 9, np.uint8)) if "dst8" in want else None
    ctx.sync()
    stage.run(src, dst, dst8, stream)
    ctx.sync(stream)
    res = {"dst": dst.download((out_size[1], out_size[0], 4)) if dst is not None else None,
           "dst8": dst8.download((out_size[1], out_size[0], 4), np.uint8) if dst8 is not None else None,
           "idx": stage.view_indices() if record else None}
    if own:
        stage.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [True, False])
@pytest.mark.parametrize("case", list(STAGE_CASES))
def test_stage_is_the_model(R, ctx, case, invert):
    """The recorded view indices are the float32 model's exactly; dst is within four times the float32 model's own deviation from the float64
    model where the two models pick the same view; dst_rgba8 is the quantisation of the stage's own dst."""
    views, o, m32, i32, m64, i64 = _case(case, invert)
    out_size = STAGE_CASES[case][0]
    got = _run_stage(R, ctx, views, out_size, o)
    assert np.array_equal(got["idx"], i32), f"{case}: {(got['idx'] != i32).sum()} view indices differ from the pinned order's"
    assert float((i32 != i64).mean()) <= MISMATCH_CAP
    agree = (i32 == i64)[..., :3]
    own = float(np.abs(m32[..., :3].astype(np.float64) - m64[..., :3])[agree].max())
    dev = float(np.abs(got["dst"][..., :3].astype(np.float64) - m64[..., :3])[agree].max())
    print(f"\n{case} invert={invert}: stage - float64 model {dev:.3e}, float32 model - float64 model {own:.3e}, ratio {dev / own if own else 0:.2f}; "
          f"stage == float32 model bit for bit: {np.array_equal(_bits(got['dst']), _bits(m32))}")
    assert dev <= 4 * own
    assert (got["dst"][..., 3] == 1).all()
    assert np.array_equal(got["dst8"], M.quantise(got["dst"]))
    assert (got["dst8"][..., 3] == 255).all()
    if case != "1x1-3":      # the random views reach below 0 and above 1: both ends of the clamp are exercised (one pixel need not reach them)
        assert got["dst8"][..., :3].min() == 0 and got["dst8"][..., :3].max() == 255


@pytest.mark.gpu
def test_constant_views_show_their_index_on_the_device(R, ctx):
    for (out_size, n, view_size) in (STAGE_CASES["96x128-8"], STAGE_CASES["130x3-255"], STAGE_CASES["37x23-5"]):
        views = np.ones((n, view_size[1], view_size[0], 4), np.float32) * ((np.arange(n, dtype=np.float32) + 1) / np.float32(n))[:, None, None, None]
        got = _run_stage(R, ctx, views, out_size, _opts(_cal(PORTRAIT, out_size), n))
        want = (got["idx"][..., :3].astype(np.float64) + 1) / n
        assert np.abs(got["dst"][..., :3] - want).max() <= 8 * 2.0 ** -24
        assert len(np.unique(got["idx"][..., :3])) > min(n, 8) // 2 and not got["idx"][..., 3].any()


@pytest.mark.gpu
def test_a_nan_view_shows_only_where_it_is_selected(R, ctx):
    out_size, n, view_size = STAGE_CASES["96x128-8"]
    views = _random_views(n, view_size).copy()
    views[5, ..., :3] = np.nan
    views[2, 3, 4, :3] = -np.inf                      # one texel of another view
    got = _run_stage(R, ctx, views, out_size, _opts(_cal(PORTRAIT, out_size), n))
    nan = np.isnan(got["dst"][..., :3])
    assert nan.any() and np.array_equal(nan, got["idx"][..., :3] == 5)
    bad = ~np.isfinite(got["dst"][..., :3]) & ~nan
    assert (got["idx"][..., :3][bad] == 2).all()
    assert np.array_equal(got["dst8"], M.quantise(got["dst"])) and (got["dst8"][..., :3][nan] == 0).all()      # clamped in the 8-bit output


@pytest.mark.gpu
def test_runs_are_bit_reproducible_with_and_without_the_recorded_indices(R, ctx):
    views, o, m32, i32, _, _ = _case("37x23-5", True)
    out_size = STAGE_CASES["37x23-5"][0]
    a = _run_stage(R, ctx, views, out_size, o)
    b = _run_stage(R, ctx, views, out_size, o)
    stream = ctx.create_stream()
    c = _run_stage(R, ctx, views, out_size, o, stream=stream)
    ctx.destroy_stream(stream)
    d = _run_stage(R, ctx, views, out_size, o, record=False)            # the kernel without the extra store
    for other in (b, c, d):
        assert a["dst"].tobytes() == other["dst"].tobytes() and a["dst8"].tobytes() == other["dst8"].tobytes()
    assert np.array_equal(a["idx"], c["idx"])
    # either output alone is the same output
    only = _run_stage(R, ctx, views, out_size, o, record=False, want=("dst",))
    only8 = _run_stage(R, ctx, views, out_size, o, record=False, want=("dst8",))
    assert only["dst"].tobytes() == a["dst"].tobytes() and only8["dst8"].tobytes() == a["dst8"].tobytes()
    stage = R.LookingGlassStage(ctx, STAGE_CASES["37x23-5"][2], out_size, dict(viewport_count=o[0], pitch=o[1], tilt=o[2], center=o[3], invert=o[4]))
    assert stage.timings()["frames"] == 0
    with pytest.raises(RuntimeError, match="both null"):
        stage.run(ctx.alloc(views.nbytes), None, None)
    with pytest.raises(RuntimeError, match="record_view_indices"):
        stage.view_indices()
    _run_stage(R, ctx, views, out_size, o, record=False, stage=stage)
    _run_stage(R, ctx, views, out_size, o, record=False, stage=stage)
    t = stage.timings()
    assert t["name"] == "looking glass composition" and t["frames"] == 2 and t["total_ms"] > 0
    stage.close()


# ---- the hosts
E2E = dict(view=(48, 64), screen=(96, 128), rig=(8, 2.0, 0.5, 2.0), sources=[1, 4, 6])


@pytest.mark.gpu
def test_renderer_composes_what_the_stage_composes_and_the_cli_writes_the_same_frame(R, ctx, tmp_path):
    """test.glb, 8 views of 48 x 64 to a 96 x 128 panel, three of them path traced and the others reprojected: RtRenderer's `composed` is the
    stage run by hand on the renderer's display layers, and `tauray_hip --display=looking-glass` writes that frame bit for bit."""
    from tauray_amd import exr
    from tauray_amd.looking_glass import LookingGlassOutput
    (W, H), screen, rig, sources = E2E["view"], E2E["screen"], E2E["rig"], E2E["sources"]
    cal = _cal(PORTRAIT, screen)
    scene = _glb("test.glb", (W, H))
    r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), spatial_reprojection=sources, looking_glass=LookingGlassOutput(cal, *rig))
    r.render()
    display, composed, composed8 = r.download("display"), r.download("composed"), r.download("composed8")
    t = r.post.lkg.timings()
    r.close()
    assert display.shape == (rig[0], H, W, 4) and composed.shape == (screen[1], screen[0], 4) and t["frames"] == 1
    by_hand = _run_stage(R, ctx, display, screen, _opts(cal, rig[0]))
    assert np.array_equal(_bits(composed), _bits(by_hand["dst"])) and np.array_equal(composed8, by_hand["dst8"])
    finite = np.isfinite(composed[..., :3])
    assert finite.mean() > 0.5 and np.isfinite(display[sources]).all()
    m64, i64 = M.compose(display, screen, *_opts(cal, rig[0]))
    agree = (by_hand["idx"] == i64)[..., :3] & finite & np.isfinite(m64[..., :3])
    assert agree.mean() > 0.45 and np.abs(composed[..., :3] - m64[..., :3])[agree].max() < 1e-5
    assert len(np.unique(by_hand["idx"][..., :3])) == rig[0]
    prefix = str(tmp_path / "lkg")
    common = [EXE, os.path.join(GOLDEN, "test.glb"), f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--display=looking-glass",
              "--lkg-params=" + ",".join(map(repr, rig)), CALIBRATION_ARG, "--spatial-reprojection=" + ",".join(map(str, sources)), "--format=rgba32"]
    subprocess.check_call(common + ["--filetype=raw", f"--headless={prefix}"])
    assert sorted(os.listdir(tmp_path)) == ["lkg.raw"], "one composed file, not a file per view"
    got = np.fromfile(prefix + ".raw", dtype=np.float32).reshape(screen[1], screen[0], 4)
    assert np.array_equal(_bits(got), _bits(composed)), f"{(_bits(got) != _bits(composed)).any(-1).mean():.3%} of the pixels differ between the hosts"
    subprocess.check_call(common + ["--compression=zip", f"--headless={prefix}x"])
    img = np.asarray(exr.load_exr_rgba(prefix + "x.exr"))
    assert img.shape[:2] == (screen[1], screen[0])
    assert np.array_equal(np.isfinite(img[..., :3]), finite) and np.array_equal(img[..., :3][finite], composed[..., :3][finite])
    # frame slots: two frames one at a time and two in flight compose the same panels bit for bit
    panels = {}
    for slots in (1, 2):
        scene = _glb("test.glb", (W, H))
        r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), spatial_reprojection=sources, looking_glass=LookingGlassOutput(cal, *rig),
                         frames_in_flight=slots)
        panels[slots] = []
        for f in range(2):
            r.render()
            panels[slots].append(r.download("composed").tobytes())
        r.close()
    assert panels[1] == panels[2] and panels[1][0] == composed.tobytes() and panels[1][0] != panels[1][1]


@pytest.mark.gpu
def test_chain_with_taa_denoiser_and_animation_through_both_hosts(R, ctx, tmp_path):
    """animated.glb, 4 views of 32 x 24 to a 64 x 48 panel behind --denoiser=bmfr --taa=4 --animation: three composed frames per host, finite, moving,
    and the same between the hosts within the tolerance tests/test_taa.py uses between them (the C++ host marks the animated instances dynamic,
    the Python host does not: another acceleration structure, the same frame up to the order of equal hits)."""
    from tauray_amd.animation import SceneAnimator
    from tauray_amd.looking_glass import LookingGlassOutput
    (W, H), screen, rig, frames = (32, 24), (64, 48), (4, 2.0, 0.25, 2.0), 3
    cal = _cal(LANDSCAPE, screen)
    arg = "--lkg-calibration=0,49.825,5.2,0.18,0,40,1,0,283,64,48,0,0,0"
    prefix = str(tmp_path / "a")
    subprocess.check_call([EXE, os.path.join(GOLDEN, "animated.glb"), f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--filetype=raw", "--display=looking-glass",
                           "--lkg-params=" + ",".join(map(repr, rig)), arg, "--denoiser=bmfr", "--taa=4", "--animation", f"--frames={frames}", f"--headless={prefix}"])
    files = sorted(os.listdir(tmp_path))
    assert files == [f"a{f}.raw" for f in range(frames)]
    out = [np.fromfile(f"{prefix}{f}.raw", dtype=np.float32).reshape(screen[1], screen[0], 4) for f in range(frames)]
    assert all(np.isfinite(o).all() and (o[..., 3] == 1).all() and o[..., :3].max() > 0.05 for o in out)
    assert not np.array_equal(out[0], out[2])
    scene = _glb("animated.glb", (W, H))
    r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), denoiser="bmfr", taa=4, looking_glass=LookingGlassOutput(cal, *rig))
    animator = SceneAnimator(r.scene_update.scene)
    animator.play("", False)
    for f in range(frames):
        r.scene_update.animate(animator, 0 if f == 0 else 16667)
        r.render()
        ref = r.download("composed")
        differing = float((np.abs(out[f] - ref).max(-1) > 1e-3).mean())
        assert np.isfinite(ref).all()
        assert differing < 2e-3 and abs(float(out[f].mean()) - float(ref.mean())) < 1e-4, f"frame {f}: {differing:.3%} of the composed pixels differ between the hosts"
    r.close()


@pytest.mark.gpu
def test_one_real_view_stays_inside_its_neighbourhood(R, ctx):
    from tauray_amd.looking_glass import LookingGlassOutput
    (W, H), screen = E2E["view"], E2E["screen"]
    scene = _glb("test.glb", (W, H))
    r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), looking_glass=LookingGlassOutput(_cal(PORTRAIT, screen), 1, 2.0, 0.5, 2.0))
    r.render()
    view, composed = r.download("display")[0], r.download("composed")
    r.close()
    assert np.isfinite(composed).all() and (composed[..., 3] == 1).all() and composed[..., :3].std() > 0.01
    (x0, x1, _), (y0, y1, _) = M.bilinear_taps(screen, (W, H), np.float32)
    taps = np.stack([view[y[:, None], x[None, :], :3] for y in (y0, y1) for x in (x0, x1)])
    eps = 8 * 2.0 ** -24 * np.abs(taps).max(0)
    assert (composed[..., :3] >= taps.min(0) - eps).all() and (composed[..., :3] <= taps.max(0) + eps).all()
