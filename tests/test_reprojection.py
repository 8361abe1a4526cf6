"""Sparse light fields (csrc/reprojection.hip): the first-hit G-buffer pass, the spatial and the temporal reprojection
stage against tests/reprojection_model.py, a numpy model written from the algorithm, and against properties that need no model.

How the bounds are set.  Nothing is compared against a figure taken from the code under test.
 * Decisions.  Reprojection has thresholds (z/w < 1, cos > 0.99, distance^2 < 0.01, inside / outside, weight > 1e-5), so two correct
   implementations can decide a pixel differently; at most 0.5 % of a layer may (LEFT_OUT_CAP, the project's allowance for threshold
   decisions).  What is compared is the canonical decision (kind, source slot, the absolute tap pixels that are kept
   and weigh more than 1e-3), not the raw tap origin: a projection that lands on a pixel centre - which every point near the grid's plane
   of convergence does - floors to either neighbour, and the tap that then differs weighs ~0.
 * Values.  On every filled pixel the stage's value is compared with the float64 model evaluated under the stage's own recorded decisions
   (no thresholds left); the tolerance per layer is four times the float32 model's largest deviation from the float64 model on the same
   inputs and decisions, measured when the test runs.
 * The affine property: a tap is kept only within distance 0.1 of the destination's position, so a convex combination of an affine
   function's values at the taps is within |grad f| * 0.1 of its value there.
Measured figures: profiles/r11/reprojection.txt.
"""
import copy
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import reprojection_model as M

LEFT_OUT_CAP = 0.005
EXE = os.path.join(ROOT, "tauray_amd", "tauray_hip")


# ======================================================================================================================
# CPU: the model against closed forms
def _perspective(fov_deg=60.0, aspect=1.0, near=0.1, far=100.0):
    f = 1.0 / np.tan(np.radians(fov_deg) / 2)
    p = np.zeros((4, 4))
    p[0, 0], p[1, 1] = f / aspect, f
    p[2, 2], p[2, 3] = (far + near) / (near - far), 2 * far * near / (near - far)
    p[3, 2] = -1
    return p


def _glm(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).T)      # [column][row]


def _wall_camera(w, h, cam_z=0.0, wall_z=-2.0, shift=(0.0, 0.0)):
    """A camera at (0, 0, cam_z) looking down -z at the wall z = wall_z: its view_proj and the G-buffer of the wall as it sees it (pos at
    the pixel centres, displaced by `shift` pixels), normal +z."""
    proj = _perspective()
    view = np.eye(4)
    view[2, 3] = -cam_z
    dist = cam_z - wall_z
    ys, xs = np.mgrid[0:h, 0:w]
    ndc_x, ndc_y = (xs + 0.5 + shift[0]) / w * 2 - 1, 1 - (ys + 0.5 + shift[1]) / h * 2
    pos = np.stack([ndc_x * dist / proj[0, 0], ndc_y * dist / proj[1, 1], np.full(xs.shape, wall_z), np.zeros(xs.shape)], -1)
    nrm = M.octahedral_pack(np.broadcast_to(np.array([0.0, 0.0, 1.0]), (h, w, 3)))
    return _glm(proj @ view), pos, nrm


def _layers(*arrays):
    return np.stack(arrays)


def test_model_same_camera_reproduces_the_source():
    w, h = 24, 16
    vp, pos, nrm = _wall_camera(w, h)
    rng = np.random.default_rng(0)
    colour = rng.uniform(0, 1, (h, w, 4))
    ids = np.zeros((h, w), np.int32)
    src = dict(color=_layers(colour), normal=_layers(nrm), pos=_layers(pos), instance_id=_layers(ids))
    dst = dict(normal=_layers(nrm), pos=_layers(pos), instance_id=_layers(ids))
    m = M.SpatialModel((w, h), 2, [0])
    out = m.run(np.stack([vp, vp]), src, dst)
    assert np.array_equal(out[0], colour)
    # the projection lands on the pixel centre to ~1e-15 of a pixel: whichever origin floor() takes, the blend is the source's pixel
    assert np.abs(out[1] - colour).max() < 1e-12
    assert (m.last["decisions"]["kind"] == M.REPROJECTED).all()
    c = M.canonical(m.last["decisions"], m.last["weights"])
    ys, xs = np.mgrid[0:h, 0:w]
    assert (c[0, ..., 2] == ys * 65536 + xs).all() and (c[0, ..., 3:] == -1).all()
    # float32: the same, to float32 rounding of a 24-pixel coordinate
    out32 = M.SpatialModel((w, h), 2, [0], dtype=np.float32).run(np.stack([vp, vp]), src, dst)
    assert out32.dtype == np.float32 and np.abs(out32[1] - colour).max() < 1e-4


def test_model_drops_taps_across_a_normal_change_and_farther_than_the_limit():
    w, h = 24, 16
    # a wall 0.5 away: pixels are 0.024 x 0.036 apart on it, so a tap is 0.022 from the destination in the wall's plane
    vp, pos, nrm = _wall_camera(w, h, wall_z=-0.5)
    _, dpos, _ = _wall_camera(w, h, wall_z=-0.5, shift=(0.5, 0.5))        # every destination pixel sits between four source pixels
    ids = np.zeros((h, w), np.int32)
    colour = np.random.default_rng(1).uniform(0, 1, (h, w, 4))
    turned = nrm.copy()
    turned[:, 10] = M.octahedral_pack(np.array([1.0, 0.0, 0.0]))          # column 10 faces +x
    far = pos.copy()
    far[5, :, 2] -= 0.11                                                    # row 5 lies 0.11 behind the wall: |d|^2 = 0.0126
    near = pos.copy()
    near[5, :, 2] -= 0.09                                                   # 0.09 behind it: |d|^2 = 0.0086
    dst = dict(normal=_layers(nrm), pos=_layers(dpos), instance_id=_layers(ids))
    m = M.SpatialModel((w, h), 2, [0])

    def bits(spos, snrm):
        m.run(np.stack([vp, vp]), dict(color=_layers(colour), normal=_layers(snrm), pos=_layers(spos), instance_id=_layers(ids)), dst)
        d = m.last["decisions"][0]
        assert (d["ox"][:-1, :-1] == np.arange(w - 1)[None]).all() and (d["oy"][:-1, :-1] == np.arange(h - 1)[:, None]).all()
        return d["bits"]
    b = bits(pos, nrm)
    assert (b[:-1, :-1] == 15).all() and (b[:-1, -1] == 0b0101).all() and (b[-1, :-1] == 0b0011).all() and b[-1, -1] == 1
    b = bits(pos, turned)
    assert (b[:-1, 9] == 0b0101).all() and (b[:-1, 10] == 0b1010).all() and (b[:-1, 8] == 15).all()
    b = bits(far, nrm)
    assert (b[4, :-1] == 0b0011).all() and (b[5, :-1] == 0b1100).all() and (b[3, :-1] == 15).all()
    assert (bits(near, nrm)[4:6, :-1] == 15).all()
    # a kept set is renormalised: the two left taps of a pixel left of column 10 share the weight
    m.run(np.stack([vp, vp]), dict(color=_layers(colour), normal=_layers(turned), pos=_layers(pos), instance_id=_layers(ids)), dst)
    assert np.abs(m.last["weights"][0, 3, 9] - [0.5, 0, 0.5, 0]).max() < 1e-9


def test_model_prefers_the_nearer_of_two_sources():
    w, h = 24, 16
    vp_near, pos_near, nrm = _wall_camera(w, h, cam_z=0.0)
    vp_far, pos_far, _ = _wall_camera(w, h, cam_z=1.0)
    vp_dst, pos_dst, _ = _wall_camera(w, h, cam_z=0.5)
    ids = np.zeros((h, w), np.int32)
    red, blue = np.zeros((h, w, 4)), np.zeros((h, w, 4))
    red[..., 0], blue[..., 2] = 1, 1
    dst = dict(normal=_layers(nrm), pos=_layers(pos_dst), instance_id=_layers(ids))
    for order in ((0, 1), (1, 0)):       # viewport 0 = far, 1 = near, 2 = destination; the list in both orders
        cams = np.stack([vp_far, vp_near, vp_dst])
        img = {0: (blue, pos_far), 1: (red, pos_near)}
        src = dict(color=_layers(*[img[v][0] for v in order]), normal=_layers(nrm, nrm), pos=_layers(*[img[v][1] for v in order]),
                   instance_id=_layers(ids, ids))
        m = M.SpatialModel((w, h), 3, list(order))
        out = m.run(cams, src, dst)
        d = m.last["decisions"][0]
        # the near camera sees less of the wall than the destination: inside its image it wins, outside the far one fills in
        inner = np.zeros((h, w), bool)
        inner[4:-4, 6:-6] = True
        assert (d["kind"] == M.REPROJECTED).all()
        assert (d["slot"][inner] == order.index(1)).all() and np.abs(out[2][inner] - red[inner]).max() < 1e-9
        assert (d["slot"][0] == order.index(0)).all() and np.abs(out[2][0] - blue[0]).max() < 1e-9


def test_model_copies_no_surface_pixels_from_a_source_without_a_surface():
    w, h = 16, 8
    vp, pos, nrm = _wall_camera(w, h)
    rng = np.random.default_rng(2)
    c0, c1 = rng.uniform(0, 1, (h, w, 4)), rng.uniform(0, 1, (h, w, 4))
    ids_dst = np.zeros((h, w), np.int32)
    ids_dst[:, :8] = -1                     # the destination's left half is sky
    ids0 = np.zeros((h, w), np.int32)       # source 0 has a surface everywhere
    ids1 = np.zeros((h, w), np.int32)
    ids1[:, :4] = -1                        # source 1 shows sky in columns 0-3
    pos_nan = pos.copy()
    pos_nan[:, 4:6, :3] = np.nan            # ... and, marked by a NaN pos instead of the id, in columns 4-5
    src = dict(color=_layers(c0, c1), normal=_layers(nrm, nrm), pos=_layers(pos, pos_nan), instance_id=_layers(ids0, ids1))
    dst = dict(normal=_layers(nrm), pos=_layers(pos), instance_id=_layers(ids_dst))
    m = M.SpatialModel((w, h), 3, [0, 1])
    out = m.run(np.stack([vp, vp, vp]), src, dst)
    d = m.last["decisions"][0]
    assert (d["kind"][:, :6] == M.SKY_COPY).all() and (d["slot"][:, :6] == 1).all() and np.array_equal(out[2][:, :6], c1[:, :6])
    assert (d["kind"][:, 6:8] == M.NONE).all() and np.isnan(out[2][:, 6:8]).all()
    assert (d["kind"][:, 8:] == M.REPROJECTED).all() and np.isfinite(out[2][:, 8:]).all()
    other = M.SpatialModel((w, h), 3, [0, 1], default_value=(7.0, 7.0, 7.0, 1.0)).run(np.stack([vp, vp, vp]), src, dst)
    assert (other[2][:, 6:8] == [7.0, 7.0, 7.0, 1.0]).all()


def _identity_motion(w, h, layers=1):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.repeat(np.stack([(xs + 0.5) / w, 1 - (ys + 0.5) / h], -1)[None], layers, 0)


def test_temporal_model_with_a_fixed_camera_is_the_recursion():
    w, h, r = 16, 12, 0.75
    _, pos, nrm = _wall_camera(w, h)
    ids = np.zeros((1, h, w), np.int32)
    ids[0, :2] = -1                                   # two rows of sky: they keep their colour and are never a tap
    rng = np.random.default_rng(3)
    m = M.TemporalModel((w, h), 1, r)
    c = None
    for n in range(6):
        x = rng.uniform(0, 1, (1, h, w, 4))
        out = m.run(dict(color=x, normal=_layers(nrm), pos=_layers(pos), screen_motion=_identity_motion(w, h), instance_id=ids))
        c = x if c is None else (1 - r) * x + r * c
        c[0, :2] = x[0, :2]
        assert np.abs(out - c).max() < 1e-12, n
        assert (m.last["decisions"]["kind"][0, 2:] == (M.REPROJECTED if n else M.NONE)).all() and (m.last["decisions"]["kind"][0, :2] == M.NONE).all()
    m.reset_history()
    x = rng.uniform(0, 1, (1, h, w, 4))
    assert np.array_equal(m.run(dict(color=x, normal=_layers(nrm), pos=_layers(pos), screen_motion=_identity_motion(w, h), instance_id=ids)), x)


# ======================================================================================================================
# CPU: the condition of the allowance, on the oracle's targets
def _grid_scene(scene, gw, gh, spacing):
    from tauray_amd.scene import generate_camera_grid
    s = copy.copy(scene)
    s.cameras = generate_camera_grid(scene.cameras[0], gw, gh, spacing, spacing, 5.0)
    return s


def _split(targets, total, sources):
    """Targets of every viewport [total, ...] -> the stage's source images (list order) and destination images (ascending)."""
    dests = [v for v in range(total) if v not in sources]
    src = {n: targets[n][sources] for n in ("color", "normal", "pos", "instance_id")}
    dst = {n: targets[n][dests] for n in ("normal", "pos", "instance_id")}
    return src, dst


@pytest.mark.parametrize("spacing", [0.02, 0.05, 0.3])
def test_threshold_decisions_stay_under_the_cap_on_oracle_targets(oracle, test_glb_128, spacing):
    """The float32 model against the float64 model on the targets the oracle renders of test.glb, a 3 x 3 grid at 128 x 128: canonical
    decisions differ on at most 0.5 % of a destination layer (measured here: at most 0.025 %), raw tap origins on many more (10 - 17 %:
    test.glb lies near the grid's plane of convergence)."""
    scene = _grid_scene(test_glb_128, 3, 3, spacing)
    osc = oracle.OracleScene(scene)
    opt = oracle.options_for_scene(scene, max_bounces=1)
    t = osc.render_pt_targets(opt, 128, 128, ["color", "normal", "pos", "instance_id"], viewports=9)
    t = dict(t, instance_id=t["instance_id"][..., 0])
    vp = scene.camera_data()["view_proj"]
    for sources in ([4], [0, 2, 4, 6, 8]):
        src, dst = _split(t, 9, sources)
        m64, m32 = M.SpatialModel((128, 128), 9, sources), M.SpatialModel((128, 128), 9, sources, dtype=np.float32)
        m64.run(vp, src, dst)
        m32.run(vp, src, dst)
        share = M.differing_share(M.canonical(m64.last["decisions"], m64.last["weights"]), M.canonical(m32.last["decisions"], m32.last["weights"]))
        raw = ((m64.last["decisions"]["ox"] != m32.last["decisions"]["ox"]) | (m64.last["decisions"]["oy"] != m32.last["decisions"]["oy"])).mean()
        filled = (m64.last["decisions"]["kind"] == M.REPROJECTED).mean()
        print(f"\nspacing {spacing} sources {sources}: canonical decisions differ on at most {share.max():.4%} of a layer, raw origins on {raw:.2%}; "
              f"{filled:.1%} of the destination pixels are reprojected")
        assert share.max() <= LEFT_OUT_CAP
        assert filled > 0.5


def test_value_under_given_decisions_has_no_threshold_left(oracle, test_glb_128):
    """The value under given decisions takes the success of the try as given too.  At spacing 0.3 the float32 model accepts a few pixels
    whose only kept taps lie in the column that weighs ~1e-5 (two float32 steps of a coordinate near 100) where the float64 model's sum
    stays below 1e-5: evaluated under the float32 model's decisions, the float64 model is finite on every filled pixel (the inputs are
    finite) and its weights are a convex combination."""
    scene = _grid_scene(test_glb_128, 3, 3, 0.3)
    opt = oracle.options_for_scene(scene, max_bounces=1)
    t = oracle.OracleScene(scene).render_pt_targets(opt, 128, 128, ["color", "normal", "pos", "instance_id"], viewports=9)
    t = dict(t, instance_id=t["instance_id"][..., 0])
    assert np.isfinite(t["color"]).all()
    vp = scene.camera_data()["view_proj"]
    sources = [0, 2, 4, 6, 8]
    src, dst = _split(t, 9, sources)
    m32, m64 = M.SpatialModel((128, 128), 9, sources, dtype=np.float32), M.SpatialModel((128, 128), 9, sources)
    m32.run(vp, src, dst)
    dec = m32.last["decisions"]
    o64 = m64.run(vp, src, dst, decisions=dec)
    for d, v in enumerate(v for v in range(9) if v not in sources):
        filled = dec[d]["kind"] != M.NONE
        assert np.isfinite(o64[v][filled]).all() and np.isnan(o64[v][~filled]).all()
        rp = dec[d]["kind"] == M.REPROJECTED
        assert np.abs(m64.last["weights"][d][rp].sum(-1) - 1).max() < 1e-12 and (m64.last["weights"][d][rp] >= 0).all()


def test_temporal_threshold_decisions_stay_under_the_cap_on_oracle_targets(oracle, test_glb_128, oracle_scene_128):
    """The same for the temporal stage with a fixed camera, where screen_motion lands on the pixel centres: four frames of the oracle's
    targets, canonical decisions of the float32 model against the float64 model's."""
    names = ["color", "normal", "pos", "screen_motion", "instance_id"]
    opt = oracle.options_for_scene(test_glb_128, max_bounces=2)
    m64, m32 = M.TemporalModel((128, 128), 1, 0.75), M.TemporalModel((128, 128), 1, 0.75, dtype=np.float32)
    for f in range(4):
        t = oracle_scene_128.render_pt_targets(opt, 128, 128, names, frame_counter=f, samples_accumulated=0)
        t = dict(t, instance_id=t["instance_id"][..., 0])
        m64.run(t)
        o32 = m32.run(t)
        share = M.differing_share(M.canonical(m64.last["decisions"], m64.last["weights"]), M.canonical(m32.last["decisions"], m32.last["weights"]))
        raw = ((m64.last["decisions"]["ox"] != m32.last["decisions"]["ox"]) | (m64.last["decisions"]["oy"] != m32.last["decisions"]["oy"])).mean()
        print(f"\ntemporal, fixed camera, frame {f}: canonical decisions differ on {share.max():.4%} of the layer, raw origins on {raw:.2%}")
        assert share.max() <= LEFT_OUT_CAP
        assert np.isfinite(o32).all()
        if f:
            assert (m64.last["decisions"]["kind"] == M.REPROJECTED).mean() > 0.5      # a fixed camera keeps most of its history


# ======================================================================================================================
# CPU: the boundary
REPROJECTION_SYMBOLS = ("trhip_gbuffer_render", "trhip_spatial_reprojection_create", "trhip_spatial_reprojection_destroy", "trhip_spatial_reprojection_run",
                        "trhip_spatial_reprojection_get_timings", "trhip_spatial_reprojection_download", "trhip_temporal_reprojection_create",
                        "trhip_temporal_reprojection_destroy", "trhip_temporal_reprojection_run", "trhip_temporal_reprojection_reset_history",
                        "trhip_temporal_reprojection_get_timings", "trhip_temporal_reprojection_download")


def test_reprojection_symbols_resolve():
    from tauray_amd import _lib
    L = _lib.lib()
    for n in REPROJECTION_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.GbufferTargetsC) == 24 and C.sizeof(_lib.ReprojectionImagesC) == 40 and C.sizeof(_lib.ReprojectionTimingsC) == 8
    assert np.dtype(_lib.REPROJECTION_RECORD).itemsize == 8 and np.dtype(_lib.REPROJECTION_RECORD) == M.RECORD


def test_create_refuses_bad_arguments_and_a_missing_device():
    from tauray_amd import _lib
    L = _lib.lib()
    out = C.c_void_p()
    nan4 = (C.c_float * 4)(*([float("nan")] * 4))

    def spatial(w, h, total, sources, dv=nan4):
        src = (C.c_uint32 * max(len(sources), 1))(*sources)
        rc = L.trhip_spatial_reprojection_create(None, w, h, total, src if sources is not None else None, len(sources), dv, C.byref(out))
        assert rc != 0 and not out.value
        return L.trhip_last_error().decode()
    assert "zero" in spatial(0, 64, 9, [4])
    assert "no source" in spatial(64, 64, 9, [])
    assert "out of range" in spatial(64, 64, 9, [9])
    assert "twice" in spatial(64, 64, 9, [4, 4])
    assert "nothing to reproject" in spatial(64, 64, 2, [0, 1])
    assert "default_value" in spatial(64, 64, 9, [4], None)
    assert "device" in spatial(64, 64, 9, [0, 4, 8])               # good arguments, no device: no CPU fallback

    def temporal(w, h, layers, ratio):
        rc = L.trhip_temporal_reprojection_create(None, w, h, layers, ratio, C.byref(out))
        assert rc != 0 and not out.value
        return L.trhip_last_error().decode()
    assert "zero" in temporal(64, 0, 1, 0.5)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        assert "ratio" in temporal(64, 64, 1, bad)
    assert "device" in temporal(64, 64, 3, 0.75)
    assert L.trhip_spatial_reprojection_run(None, None, None, None, None) != 0 and L.trhip_temporal_reprojection_run(None, None, None) != 0
    assert L.trhip_temporal_reprojection_reset_history(None) != 0
    t = _lib.GbufferTargetsC()
    one = (C.c_uint32 * 1)(0)
    assert L.trhip_gbuffer_render(None, 0, one, 1, 1e-4, C.byref(t), 64, 64, None) != 0 and "device" in L.trhip_last_error().decode()


def test_renderer_refuses_what_reprojection_cannot_do():
    from tauray_amd import renderer as R
    new = lambda **kw: R.RtRenderer(None, None, None, (64, 64), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="empty"):
        new(viewports=9, spatial_reprojection=[])
    with pytest.raises(ValueError, match="out of range"):
        new(viewports=9, spatial_reprojection=[0, 9])
    with pytest.raises(ValueError, match="out of range"):
        new(viewports=9, spatial_reprojection=[-1])
    with pytest.raises(ValueError, match="every viewport"):
        new(viewports=3, spatial_reprojection=[0, 1, 2])
    with pytest.raises(ValueError, match="twice"):
        new(viewports=9, spatial_reprojection=[4, 4])
    for shard in ("pixels", "views", "samples"):
        with pytest.raises(ValueError, match="one device"):
            new(viewports=9, spatial_reprojection=[4], world_size=2, shard=shard)
        with pytest.raises(ValueError, match="one device"):
            new(temporal_reprojection=0.5, world_size=2, shard=shard)
    with pytest.raises(ValueError, match="denoiser"):
        new(viewports=9, spatial_reprojection=[4], denoiser="bmfr")
    with pytest.raises(ValueError, match="denoiser"):
        new(temporal_reprojection=0.5, denoiser="bmfr")
    with pytest.raises(ValueError, match="accumulate"):
        new(temporal_reprojection=0.5, accumulate=True)
    with pytest.raises(ValueError, match="frames_per_launch"):
        new(viewports=9, spatial_reprojection=[4], frames_per_launch=2)
    with pytest.raises(ValueError, match="ratio"):
        new(temporal_reprojection=1.0)
    assert R.viewport_runs([0, 4, 8]) == [(0, 4, 3)] and R.viewport_runs([18, 19, 20]) == [(18, 1, 3)]
    assert R.viewport_runs([0, 1, 5]) == [(0, 1, 2), (5, 1, 1)] and R.viewport_runs([7, 2]) == [(7, 1, 1), (2, 1, 1)]


def test_cli_knows_both_options_and_refuses_the_same_combinations():
    h = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--spatial-reprojection" in h.stdout + h.stderr and "--temporal-reprojection" in h.stdout + h.stderr
    glb = os.path.join(GOLDEN, "test.glb")

    def refused(*args):
        r = subprocess.run([EXE, glb, "--width=32", "--height=32", "--headless=/dev/null", *args], capture_output=True, text=True)
        assert r.returncode != 0, args
        return r.stderr
    grid = "--camera-grid=3,3,0.02,0.02"
    assert "out of range" in refused(grid, "--spatial-reprojection=0,9")
    assert "every viewport" in refused("--camera-grid=2,1,0.02,0.02", "--spatial-reprojection=0,1")
    assert "spatial-reprojection" in refused(grid, "--spatial-reprojection=")
    assert "twice" in refused(grid, "--spatial-reprojection=4,4")
    assert "denoiser" in refused(grid, "--spatial-reprojection=4", "--denoiser=bmfr")
    assert "denoiser" in refused("--temporal-reprojection=0.5", "--denoiser=bmfr")
    assert "accumulat" in refused("--temporal-reprojection=0.5", "--accumulation")
    assert "one device" in refused(grid, "--spatial-reprojection=4", "--fake-devices=2")
    assert "ratio" in refused("--temporal-reprojection=1.5")


# ======================================================================================================================
# GPU
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


def _glb(name, size):
    from tauray_amd.gltf import load_glb
    return load_glb(os.path.join(GOLDEN, name), size[0], size[1])


def _sponza(size, tris=30000, envmap=True):
    from tauray_amd import scenes
    s = scenes.sponza_class(seed=1, target_tris=tris, width=size[0], height=size[1])
    if not envmap:
        s.envmap = None
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pack_f32(n):
    """octahedral_pack in float32, operation by operation as the kernels evaluate it."""
    n = n.astype(np.float32)
    one, two = np.float32(1), np.float32(2)
    nn = n / ((np.abs(n[..., 0]) + np.abs(n[..., 1])) + np.abs(n[..., 2]))[..., None]
    sx = np.where(nn[..., 0] >= 0, one, np.float32(0)) * two - one
    sy = np.where(nn[..., 1] >= 0, one, np.float32(0)) * two - one
    lower = np.stack([(one - np.abs(nn[..., 1])) * sx, (one - np.abs(nn[..., 0])) * sy], -1)
    return np.where(nn[..., 2:3] >= 0, nn[..., :2], lower).astype(np.float32)


# ---- 1. the G-buffer pass
@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,strategy", [("test.glb", 0), ("test.glb", 1), ("sponza", 0), ("sponza", 2)])
def test_gbuffer_pass_is_the_feature_stage(R, ctx, scene_name, strategy):
    """pos.xyz and the instance id equal trhip_feature_render features 3 and 9 bit for bit, the normal is the packing of feature 1; for a
    viewport list out of order (with a repeat), on the merged and the two-level acceleration structure; sponza_class shows sky (misses)."""
    size = (96, 64)
    w, h = size
    scene = _grid_scene(_glb("test.glb", size) if scene_name == "test.glb" else _sponza(size), 3, 3, 0.05)
    ss = R.SceneStage(ctx, scene, as_strategy=strategy)
    views = [5, 0, 7, 2, 5]
    g = R.GbufferStage(ctx, ss, size, scene.cameras[0].projection)
    t = g.alloc_targets(len(views))
    g.run(views, t)
    ctx.sync()
    normal, pos = t["normal"].download((len(views), h, w, 2)), t["pos"].download((len(views), h, w, 4))
    ids = t["instance_id"].download((len(views), h, w), np.int32)
    buf = ctx.alloc(w * h * 16)
    misses = 0
    for l, v in enumerate(views):
        feat = {}
        for f in (1, 3, 9):
            R.FeatureStage(ctx, ss, f, _dup(size), scene.cameras[0].projection).run(buf, v)
            ctx.sync()
            feat[f] = buf.download((h, w, 4))
        hit = ~np.isnan(feat[9][..., 0])
        misses += int((~hit).sum())
        assert np.array_equal(ids[l] >= 0, hit)
        assert np.array_equal(ids[l][hit], feat[9][..., 0][hit].astype(np.int32)) and (ids[l][~hit] == -1).all()
        assert np.array_equal(_bits(pos[l][..., :3])[hit], _bits(feat[3][..., :3])[hit]) and (pos[l][..., 3] == 0).all()
        assert np.array_equal(_bits(normal[l])[hit], _bits(_pack_f32(feat[1][..., :3]))[hit])
        origin = scene.camera_data()["origin"][v][:3]
        assert np.array_equal(_bits(pos[l][..., :3][~hit]), _bits(np.broadcast_to(origin, pos[l][..., :3][~hit].shape)))
        assert np.isfinite(normal[l]).all()
    assert np.array_equal(_bits(pos[0]), _bits(pos[4]))          # the repeated viewport
    assert misses > 0 or scene_name != "sponza", "sponza_class must show sky"
    # a null target is not written, the others are the same
    t2 = g.alloc_targets(len(views))
    g.run(views, dict(t2, normal=None))
    ctx.sync()
    assert np.array_equal(_bits(t2["pos"].download((len(views), h, w, 4))), _bits(pos)) and not t2["normal"].download((len(views), h, w, 2)).any()


@pytest.mark.gpu
def test_gbuffer_pass_of_a_list_longer_than_one_launch(R, ctx):
    """65 viewports are two launches, of 64 and of 1: layer 64 is layer 0 of a one-entry list of its viewport and layer 63 repeats layer 0,
    bit for bit.  17 x 9 pixels leave the tile partial on both axes."""
    size = (17, 9)
    w, h = size
    scene = _grid_scene(_glb("test.glb", size), 2, 1, 0.05)
    ss = R.SceneStage(ctx, scene)
    g = R.GbufferStage(ctx, ss, size, scene.cameras[0].projection)

    def frame(views):
        t = g.alloc_targets(len(views))
        g.run(views, t)
        ctx.sync()
        got = [t["normal"].download((len(views), h, w, 2)), t["pos"].download((len(views), h, w, 4)), t["instance_id"].download((len(views), h, w), np.int32)]
        for b in t.values():
            b.free()
        return got

    many, one = frame([0] * 64 + [1]), frame([1])
    assert (many[2][0] >= 0).any()
    for a, b in zip(many, one):
        assert a[64].tobytes() == b[0].tobytes() and a[63].tobytes() == a[0].tobytes()
    assert many[1][64].tobytes() != many[1][0].tobytes(), "the two viewports see the same"


# ---- 2. the path tracer on a viewport list
@pytest.mark.gpu
@pytest.mark.parametrize("sources", [[0, 4, 8], [0, 1, 5], [7, 2]])
def test_active_layers_equal_the_full_render(R, ctx, sources):
    """With a viewport list, layer l shows viewport list[l] with its camera and its RNG stream: the active layers of the sparse frame equal
    the same viewports of a full nine-view render bit for bit - one frame, and three accumulated frames."""
    size = (96, 96)
    scene = _grid_scene(_glb("test.glb", size), 3, 3, 0.05)
    opt = R.options_for_scene(scene, max_bounces=3)
    for accumulate, frames in ((False, 1), (True, 3)):
        full = R.RtRenderer(ctx, scene, opt, size, viewports=9, accumulate=accumulate)
        sparse = R.RtRenderer(ctx, scene, opt, size, viewports=9, accumulate=accumulate, spatial_reprojection=sources)
        assert not sparse.fused_tonemap and full.fused_tonemap
        for _ in range(frames):
            full.render()
            sparse.render()
        a, b = full.download("color"), sparse.download("color")
        assert b.shape == a.shape == (9, 96, 96, 4)
        for v in sources:
            assert np.array_equal(_bits(a[v]), _bits(b[v])), f"viewport {v}, {frames} frame(s)"
        da, db = full.download("display"), sparse.download("display")
        for v in sources:
            assert np.array_equal(_bits(da[v]), _bits(db[v])), f"display of viewport {v}"
        others = [v for v in range(9) if v not in sources]
        assert not any(np.array_equal(a[v], b[v]) for v in others), "a reprojected view is not a path-traced view"
        full.close()
        sparse.close()


# ---- 3. the spatial stage against the model
def _sparse_frame(R, ctx, scene, size, total, sources, **kw):
    """One frame of RtRenderer(spatial_reprojection=sources): the stage's inputs, decisions and output, downloaded."""
    w, h = size
    r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), size, viewports=total, spatial_reprojection=sources, **kw)
    r.render(tonemap=False)
    r.sync()
    S, D = len(sources), total - len(sources)
    slot = r.current
    src = dict(color=slot.color.download((S, h, w, 4)), normal=slot.features["normal"].download((S, h, w, 2)),
               pos=slot.features["pos"].download((S, h, w, 4)), instance_id=slot.features["instance_id"].download((S, h, w), np.int32))
    dst = dict(normal=r.post.destination_targets["normal"].download((D, h, w, 2)), pos=r.post.destination_targets["pos"].download((D, h, w, 4)),
               instance_id=r.post.destination_targets["instance_id"].download((D, h, w), np.int32))
    out = r.download("color")
    dec = r.post.spatial.decisions()
    vp = r.scene_update.camera_data.view(np.float32).reshape(total, 80)[:, 32:48].reshape(total, 4, 4)
    timings = r.post.spatial.timings()
    r.close()
    return vp, src, dst, out, dec, timings


def _check_against_model(label, size, total, sources, vp, src, dst, out, dec):
    dests = [v for v in range(total) if v not in sources]
    m64, m32 = M.SpatialModel(size, total, sources), M.SpatialModel(size, total, sources, dtype=np.float32)
    o64 = m64.run(vp, src, dst, decisions=dec)
    o32 = m32.run(vp, src, dst, decisions=dec)
    own = M.SpatialModel(size, total, sources)
    own.run(vp, src, dst)
    share = M.differing_share(M.canonical(own.last["decisions"], own.last["weights"]), M.canonical(dec, m64.last["weights"]))
    assert share.max() <= LEFT_OUT_CAP, f"{label}: canonical decisions differ from the float64 model's on {share.max():.3%} of a layer"
    for s, v in enumerate(sources):
        assert np.array_equal(_bits(out[v]), _bits(src["color"][s])), f"{label}: source layer {v} must pass bit for bit"
    worst_ratio, worst_gpu, worst_model, filled_total = 0.0, 0.0, 0.0, 0
    for d, v in enumerate(dests):
        kind = dec[d]["kind"]
        filled = kind != M.NONE
        assert np.isnan(out[v][~filled]).all(), f"{label}: viewport {v}: a pixel without a decision must hold default_value"
        finite_in = np.isfinite(o64[v]).all(-1)          # the path tracer's rare NaN sample reprojects as NaN in model and stage alike
        assert np.array_equal(np.isfinite(out[v]).all(-1)[filled], finite_in[filled]), f"{label}: viewport {v}: a NaN that is not default_value"
        sky = kind == M.SKY_COPY
        assert np.array_equal(_bits(out[v][sky]), _bits(o64[v][sky].astype(np.float32))), f"{label}: viewport {v}: a no-surface copy is a copy"
        m = filled & finite_in
        filled_total += int(m.sum())
        if not m.any():
            continue
        model_dev = float(np.abs(o32[v][m].astype(np.float64) - o64[v][m]).max())
        gpu_dev = float(np.abs(out[v][m].astype(np.float64) - o64[v][m]).max())
        worst_model, worst_gpu = max(worst_model, model_dev), max(worst_gpu, gpu_dev)
        worst_ratio = max(worst_ratio, gpu_dev / model_dev if model_dev > 0 else (0.0 if gpu_dev == 0 else np.inf))
        print(f"\nspatial [{label}] viewport {v}: {int(m.sum())} filled pixels, deviation from the float64 model: model32 {model_dev:.3e} gpu {gpu_dev:.3e}")
        assert gpu_dev <= 4 * model_dev, f"{label}: viewport {v} deviates {gpu_dev:.3e} from the float64 model, the float32 model {model_dev:.3e}"
    print(f"\nspatial [{label}] {size[0]}x{size[1]} {total} views, sources {sources}: decisions differ on at most {share.max():.4%} of a layer; "
          f"{filled_total} filled pixels, largest deviation model32 {worst_model:.2e} gpu {worst_gpu:.2e}, worst GPU/model ratio {worst_ratio:.2f}")
    return worst_ratio


SPATIAL_CASES = {
    "glb-3x3-one": ("test.glb", (128, 128), (3, 3), 0.05, [4]),
    "glb-3x3-two": ("test.glb", (128, 128), (3, 3), 0.05, [8, 0]),
    "glb-3x3-five": ("test.glb", (128, 128), (3, 3), 0.3, [0, 2, 4, 6, 8]),
    "glb-5x1-one": ("test.glb", (128, 128), (5, 1), 0.05, [2]),
    # sponza_class is 30 units long: at 256 x 144 a pixel covers about 0.05 units at 10 units' distance, half the 0.1 limit of a tap
    "sponza-3x3-one": ("sponza", (256, 144), (3, 3), 0.05, [4]),
    "sponza-5x1-two": ("sponza", (256, 144), (5, 1), 0.1, [0, 4]),
    "sponza-3x3-five-no-envmap": ("sponza-no-envmap", (256, 144), (3, 3), 0.05, [0, 2, 4, 6, 8]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SPATIAL_CASES))
def test_spatial_stage_is_the_model(R, ctx, case):
    name, size, (gw, gh), spacing, sources = SPATIAL_CASES[case]
    base = _glb("test.glb", size) if name == "test.glb" else _sponza(size, envmap=(name == "sponza"))
    scene = _grid_scene(base, gw, gh, spacing)
    vp, src, dst, out, dec, _ = _sparse_frame(R, ctx, scene, size, gw * gh, sources)
    if name == "sponza":
        assert (dst["instance_id"] < 0).any() and (dec["kind"] == M.SKY_COPY).any(), "the scene must show sky"
    assert (dec["kind"] == M.REPROJECTED).mean() > 0.1, "the case must exercise the reprojection"
    _check_against_model(case, size, gw * gh, sources, vp, src, dst, out, dec)


# ---- 4. the temporal stage against the model
TEMPORAL_IMAGES = ("color", "normal", "pos", "screen_motion", "instance_id")


def _alloc_images(R, ctx, size, layers):
    w, h = size
    return {n: ctx.alloc(layers * w * h * R.PathTracerStage.TARGETS[n][0] * 4).zero() for n in TEMPORAL_IMAGES}


def _download_images(R, bufs, size, layers):
    w, h = size
    out = {n: b.download((layers, h, w, R.PathTracerStage.TARGETS[n][0]), R.PathTracerStage.TARGETS[n][1]) for n, b in bufs.items()}
    out["instance_id"] = out["instance_id"][..., 0]
    return out


def _orbit(cam0, angle):
    c = copy.deepcopy(cam0)
    ca, sa = np.cos(angle), np.sin(angle)
    rot = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1.0]])
    c.transform = rot @ np.asarray(cam0.transform, float)
    return c


def _frame_source(R, ctx, scene, size, layers, cameras_of_frame=None, animate=None):
    ss = R.SceneStage(ctx, scene)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=3), _dup(size))
    bufs = _alloc_images(R, ctx, size, layers)
    state = {"prev": None}

    def render(f):
        if animate is not None:
            animate(ss, f)
        elif cameras_of_frame is not None:
            cams = cameras_of_frame(f)
            ss.update_cameras(cams)
            ss.set_previous_cameras(state["prev"] or cams)
            state["prev"] = cams
        pt.reset_accumulated_samples()
        pt.run_targets(bufs, layers)
        ctx.sync()
        return bufs
    return render, pt


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fixed", "orbit", "animated", "fixed-no-id-two-layers"])
def test_temporal_stage_is_the_model(R, ctx, case):
    """Eight frames; the models continue with the stage's decisions, so that one pixel decided differently does not make the rest of the
    sequence incomparable."""
    size, layers, frames, ratio = (128, 128), 1, 8, 0.75
    if case == "animated":
        from tauray_amd.animation import SceneAnimator
        size = (128, 96)
        scene = _glb("animated.glb", size)
        holder = {}

        def animate(ss, f):
            if "a" not in holder:
                holder["a"] = SceneAnimator(ss.scene)
                holder["a"].play("", loop=True)
            ss.animate(holder["a"], 0 if f == 0 else round(1000000.0 / 24.0))
        render, pt = _frame_source(R, ctx, scene, size, layers, animate=animate)
    elif case == "orbit":
        scene = _glb("test.glb", size)
        cam0 = scene.cameras[0]
        render, pt = _frame_source(R, ctx, scene, size, layers, cameras_of_frame=lambda f: [_orbit(cam0, 0.02 * f)])
    elif case == "fixed":
        size = (128, 72)
        render, pt = _frame_source(R, ctx, _sponza(size), size, layers)
    else:
        layers = 2
        scene = _grid_scene(_glb("test.glb", size), 2, 1, 0.3)
        render, pt = _frame_source(R, ctx, scene, size, layers)
    use_id = case != "fixed-no-id-two-layers"
    stage = R.TemporalReprojectionStage(ctx, size, layers, ratio)
    m64, m32 = M.TemporalModel(size, layers, ratio), M.TemporalModel(size, layers, ratio, dtype=np.float32)
    own = M.TemporalModel(size, layers, ratio)
    worst = [0.0, 0.0, 0.0, 0.0]
    for f in range(frames):
        bufs = render(f)
        t = _download_images(R, bufs, size, layers)
        images = dict(bufs)
        if not use_id:
            images["instance_id"], t["instance_id"] = None, None
        stage.run(images)
        ctx.sync()
        got = bufs["color"].download((layers, size[1], size[0], 4))
        dec = stage.decisions()
        own.history = None if m64.history is None else tuple(x.copy() for x in m64.history)      # the decisions the model makes on the same history
        own.run(t)
        o64, o32 = m64.run(t, decisions=dec), m32.run(t, decisions=dec)
        share = M.differing_share(M.canonical(own.last["decisions"], own.last["weights"]), M.canonical(dec, m64.last["weights"]))
        assert share.max() <= LEFT_OUT_CAP, f"{case} frame {f}: canonical decisions differ on {share.max():.3%} of a layer"
        if f == 0:
            assert (dec["kind"] == M.NONE).all() and np.array_equal(_bits(got), _bits(t["color"])), "the first frame only stores history"
        else:
            surface = ~M.no_surface(t["pos"], t["instance_id"])
            assert (dec["kind"] == M.REPROJECTED)[surface].mean() > 0.3, "the case must exercise the reprojection"
        untouched = dec["kind"] == M.NONE
        assert np.array_equal(_bits(got[untouched]), _bits(t["color"][untouched])), f"{case} frame {f}: a pixel without a kept tap keeps its colour"
        m = np.isfinite(o64).all(-1)
        assert np.array_equal(np.isfinite(got).all(-1), m)
        model_dev = float(np.abs(o32[m].astype(np.float64) - o64[m]).max())
        gpu_dev = float(np.abs(got[m].astype(np.float64) - o64[m]).max())
        print(f"\ntemporal [{case}] frame {f}: decisions differ on {share.max():.4%}; deviation from the float64 model: model32 {model_dev:.3e} gpu {gpu_dev:.3e}")
        assert gpu_dev <= 4 * model_dev, f"{case} frame {f}: deviates {gpu_dev:.3e} from the float64 model, the float32 model {model_dev:.3e}"
        assert np.array_equal(_bits(stage.download("previous_color")), _bits(got)), "the blended colour becomes the history"
        worst = [max(worst[0], float(share.max())), max(worst[1], model_dev), max(worst[2], gpu_dev),
                 max(worst[3], gpu_dev / model_dev if model_dev > 0 else (0.0 if gpu_dev == 0 else np.inf))]
    print(f"\ntemporal [{case}] {size[0]}x{size[1]}x{layers}, {frames} frames: decisions differ on at most {worst[0]:.4%}; largest deviation "
          f"model32 {worst[1]:.2e} gpu {worst[2]:.2e}, worst GPU/model ratio {worst[3]:.2f}")
    # reset_history equals a new stage
    bufs = render(frames)
    t = _download_images(R, bufs, size, layers)
    keep = {n: ctx.alloc(b.nbytes).upload(t[n] if n != "instance_id" else t[n][..., None]) for n, b in bufs.items()}
    stage.reset_history()
    fresh = R.TemporalReprojectionStage(ctx, size, layers, ratio)
    for s, imgs in ((stage, bufs), (fresh, keep)):
        s.run(imgs)
        s.run(imgs)
    ctx.sync()
    assert np.array_equal(_bits(bufs["color"].download((layers, size[1], size[0], 4))), _bits(keep["color"].download((layers, size[1], size[0], 4))))
    assert stage.timings()["frames"] == frames + 2 and stage.timings()["total_ms"] > 0
    stage.close()
    fresh.close()
    pt.close()


# ---- 5. properties that need no model
def _upload(ctx, images):
    out = {}
    for n, a in images.items():
        a = np.ascontiguousarray(a, dtype=np.int32 if n == "instance_id" else np.float32)
        out[n] = ctx.alloc(a.nbytes).upload(a)
    return out


@pytest.mark.gpu
def test_spatial_stage_properties(R, ctx):
    size, total, sources = (256, 144), 9, [0, 4, 8]
    w, h = size
    scene = _grid_scene(_sponza(size), 3, 3, 0.05)
    vp, src, dst, out, dec, timings = _sparse_frame(R, ctx, scene, size, total, sources)
    assert timings["frames"] == 1 and timings["total_ms"] > 0
    dests = [v for v in range(total) if v not in sources]
    # the sources' colour an affine function of pos (sky: a constant)
    grad = np.array([[0.3, -0.2, 0.1], [0.05, 0.4, -0.3], [-0.25, 0.15, 0.2]])
    offset = np.array([2.0, 3.0, 4.0])
    f = lambda p: p[..., :3].astype(np.float64) @ grad.T + offset      # noqa: E731
    src_ns = M.no_surface(src["pos"], src["instance_id"])
    colour = np.concatenate([np.where(src_ns[..., None], 9.0, f(src["pos"])), np.ones(src_ns.shape + (1,))], -1).astype(np.float32)
    ss = R.SceneStage(ctx, scene)          # the stage reads the scene's cameras
    stage = R.SpatialReprojectionStage(ctx, size, total, sources)
    d_src, d_dst = _upload(ctx, dict(src, color=colour)), _upload(ctx, dst)
    outs = []
    for stream in (None, ctx.create_stream()):
        full = ctx.alloc(total * w * h * 16).zero()
        stage.run(d_src, d_dst, full, stream)
        ctx.sync(stream)
        outs.append(full.download((total, h, w, 4)))
        if stream is not None:
            ctx.destroy_stream(stream)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "two runs, on the default stream and on a stream of its own, give the same bits"
    got, d2 = outs[0], stage.decisions()
    for s, v in enumerate(sources):
        assert np.array_equal(_bits(got[v]), _bits(colour[s])), "source layers pass bit for bit"
    lip = float(np.linalg.norm(grad, 2))               # |grad f|: the largest change of f per unit distance
    worst = 0.0
    for d, v in enumerate(dests):
        kind = d2[d]["kind"]
        assert np.array_equal(np.isnan(got[v]).any(-1), kind == M.NONE), "no NaN other than default_value"
        rp = kind == M.REPROJECTED
        err = np.linalg.norm(got[v][rp][:, :3].astype(np.float64) - f(dst["pos"][d][rp]), axis=-1)
        worst = max(worst, float(err.max()))
        assert (err <= lip * 0.1).all(), f"viewport {v}: a reprojected pixel is {err.max():.4f} from f(pos), the limit is {lip * 0.1:.4f}"
        assert (got[v][kind == M.SKY_COPY][:, :3] == 9.0).all()
        # kept taps are inside the image
        for k in range(4):
            kept = rp & (((d2[d]["bits"] >> k) & 1) == 1)
            x, y = d2[d]["ox"][kept].astype(int) + (k & 1), d2[d]["oy"][kept].astype(int) + (k >> 1)
            assert ((x >= 0) & (x < w) & (y >= 0) & (y < h)).all()
    print(f"\nspatial affine property: largest |colour - f(pos)| {worst:.4f}, limit {lip * 0.1:.4f}")
    # a layer no source sees (its surface lies behind every source camera) is all default_value
    hidden = {n: a.copy() for n, a in dst.items()}
    back = scene.camera_data()["view_inverse"][4]          # [column][row]: column 2 = the camera's +z (backwards), column 3 = its position
    hidden["pos"][0, ..., :3] = back[3][:3] + back[2][:3] * 5.0
    hidden["instance_id"][0] = 0
    other = R.SpatialReprojectionStage(ctx, size, total, sources, default_value=(1.0, 2.0, 3.0, 4.0))
    full = ctx.alloc(total * w * h * 16).zero()
    d_hidden = _upload(ctx, hidden)
    other.run(d_src, d_hidden, full)
    ctx.sync()
    o = full.download((total, h, w, 4))
    assert (o[dests[0]] == [1.0, 2.0, 3.0, 4.0]).all() and (other.decisions()[0]["kind"] == M.NONE).all()
    assert np.isfinite(o).all()
    stage.close()
    other.close()
    del ss


# ---- 6. hosts
@pytest.mark.gpu
def test_renderer_with_both_options_equals_the_stages_driven_by_hand(R, ctx):
    size, total, sources, ratio = (96, 96), 9, [0, 4, 8], 0.6
    w, h = size
    scene = _grid_scene(_glb("test.glb", size), 3, 3, 0.05)
    opt = R.options_for_scene(scene, max_bounces=3)
    r = R.RtRenderer(ctx, scene, opt, size, viewports=total, spatial_reprojection=sources, temporal_reprojection=ratio)
    assert not r.fused_tonemap and r.post.spatial is not None and r.post.temporal is not None
    frames = []
    for _ in range(3):
        r.render()
        frames.append(r.download("display").copy())
    r.close()
    ss = R.SceneStage(ctx, scene)
    pt = R.PathTracerStage(ctx, ss, opt, _dup(size))
    pt.set_shard(viewport_base=0, viewport_stride=4)
    S, dests = len(sources), [v for v in range(total) if v not in sources]
    bufs = _alloc_images(R, ctx, size, S)
    temporal, spatial = R.TemporalReprojectionStage(ctx, size, S, ratio), R.SpatialReprojectionStage(ctx, size, total, sources)
    gb, tm = R.GbufferStage(ctx, ss, size, opt.projection, opt.min_ray_dist), R.TonemapStage(ctx)
    dst = gb.alloc_targets(len(dests))
    full, display = ctx.alloc(total * w * h * 16), ctx.alloc(total * w * h * 16)
    for f in range(3):
        ss.set_previous_camera_data(ss.camera_data)
        pt.reset_accumulated_samples()
        pt.run_targets(bufs, S)
        temporal.run(bufs)
        gb.run(dests, dst)
        spatial.run({n: bufs[n] for n in spatial.SOURCES}, dst, full)
        tm.run(full, display, w, h, total)
        assert np.array_equal(_bits(display.download((total, h, w, 4))), _bits(frames[f])), f"frame {f}"
    assert not np.array_equal(frames[0], frames[2])
    # frames in flight: the same frames (the temporal history is one chain on the default stream)
    r2 = R.RtRenderer(ctx, scene, opt, size, viewports=total, spatial_reprojection=sources, temporal_reprojection=ratio, frames_in_flight=2)
    for f in range(3):
        r2.render()
        assert np.array_equal(_bits(r2.download("display")), _bits(frames[f])), f"two slots, frame {f}"
    r2.close()
    for s in (temporal, spatial, pt):
        s.close()


@pytest.mark.gpu
def test_cli_writes_the_light_field_like_the_python_host(R, ctx, tmp_path):
    """`tauray_hip --camera-grid=9,5,... --spatial-reprojection=18,...,26`: 45 EXR files in natural view order, equal to the Python host's."""
    from tauray_amd import exr
    W, H, gw, gh = 96, 54, 9, 5
    sources = list(range(18, 27))
    glb = os.path.join(GOLDEN, "test.glb")
    scene = _grid_scene(_glb("test.glb", (W, H)), gw, gh, 0.02)
    r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), viewports=gw * gh, spatial_reprojection=sources)
    r.render()
    ref = r.download("display")
    r.close()
    prefix = str(tmp_path / "lf")
    common = [EXE, glb, f"--width={W}", f"--height={H}", "--max-ray-depth=3", f"--camera-grid={gw},{gh},0.02,0.02",
              "--spatial-reprojection=" + ",".join(map(str, sources))]
    subprocess.check_call(common + ["--filetype=raw", f"--headless={prefix}"])
    for v in range(gw * gh):
        got = np.fromfile(f"{prefix}{v}_.raw", dtype=np.float32).reshape(H, W, 4)
        assert np.array_equal(_bits(got), _bits(ref[v])), f"view {v}"
    eprefix = str(tmp_path / "lfx")
    subprocess.check_call(common + ["--filetype=exr", f"--headless={eprefix}"])
    files = sorted(p for p in os.listdir(tmp_path) if p.startswith("lfx") and p.endswith(".exr"))
    assert len(files) == gw * gh
    for v in (0, 18, 22, 44):
        img = exr.load_exr_rgba(f"{eprefix}{v}_.exr")
        a, b = np.asarray(img)[..., :3], ref[v][..., :3]
        both = np.isfinite(a) & np.isfinite(b)
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.abs(a[both] - b[both]).max() <= 1e-3 * max(1.0, float(np.abs(b[both]).max())), f"view {v}"
    # the temporal stage through the CLI: frame 0 is the plain frame, later frames are blended
    t_prefix, p_prefix = str(tmp_path / "t"), str(tmp_path / "p")
    one = [EXE, glb, f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--filetype=raw", "--frames=3"]
    subprocess.check_call(one + ["--temporal-reprojection=0.75", f"--headless={t_prefix}"])
    subprocess.check_call(one + [f"--headless={p_prefix}"])
    scene1 = _glb("test.glb", (W, H))
    r = R.RtRenderer(ctx, scene1, R.options_for_scene(scene1, max_bounces=3), (W, H), temporal_reprojection=0.75)
    for f in range(3):
        r.render()
        got = np.fromfile(f"{t_prefix}{f}.raw", dtype=np.float32).reshape(H, W, 4)
        plain = np.fromfile(f"{p_prefix}{f}.raw", dtype=np.float32).reshape(H, W, 4)
        assert np.array_equal(_bits(got), _bits(r.download("display")[0])), f"temporal frame {f}"
        assert np.array_equal(got, plain) == (f == 0)
    r.close()


# ---- 7. full size
def _rms(a, b, mask):
    d = (a[..., :3].astype(np.float64) - b[..., :3])[mask]
    return float(np.sqrt((d * d).mean()))


@pytest.mark.gpu
def test_full_size_sparse_frame_is_cheaper_than_the_full_frame(R, ctx):
    """Config 5's scene, 1920 x 1080 x 45, the centre row's nine views active.  A frame's time is taken on the host around render() +
    sync (the frame's launches back to back, nothing else on the device); medians of 5 after 2 warm-ups, both renderers alive in the
    same test; the yardstick is the full 45-view render.  Figures: profiles/r11/reprojection.txt."""
    from tauray_amd import scenes
    W, H, V = 1920, 1080, 45
    sources = list(range(18, 27))
    scene = _grid_scene(scenes.sponza_class(width=W, height=H), 9, 5, 0.02)
    opt = R.options_for_scene(scene, max_bounces=4)

    def frame_ms(r):
        times = []
        for i in range(7):
            r.sync()
            t0 = time.perf_counter()
            r.render(tonemap=False)
            r.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times[2:]))
    full = R.RtRenderer(ctx, scene, opt, (W, H), viewports=V, use_torch=False)
    full_ms = frame_ms(full)
    full_pt = full.timings()["path_tracing_ms"]
    full.close()
    sparse = R.RtRenderer(ctx, scene, opt, (W, H), viewports=V, use_torch=False, spatial_reprojection=sources)
    sparse_ms = frame_ms(sparse)
    stages = {"path_tracing_ms": sparse.timings()["path_tracing_ms"], "spatial_ms": sparse.post.spatial.timings()["total_ms"]}
    dec = sparse.post.spatial.decisions()
    filled = float((dec["kind"] != M.NONE).mean())
    out = sparse.download("color")
    sparse.close()
    assert np.isfinite(out[sources]).all()
    print(f"\nfull size 1920x1080x45, 9 sources: full frame {full_ms:.2f} ms (path tracing {full_pt:.2f} ms), sparse frame {sparse_ms:.2f} ms "
          f"({stages}), ratio {full_ms / sparse_ms:.2f}; {filled:.2%} of the destination pixels filled")
    assert sparse_ms < full_ms
