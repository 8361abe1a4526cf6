"""Temporal antialiasing: the camera jitter of both hosts, the stage (trhip_taa_*, csrc/taa.hip) against
tests/taa_model.py, a numpy model written from the algorithm, and against properties that need no model.

How the bounds are set.  Nothing is compared against a figure taken from the code under test.
 * The stage (test_stage_is_the_model).  Every frame the float64 model gets the stage's own history from before the frame and the frame's
   inputs as the stage read them.  The algorithm has decisions (the dilation offset of a strict depth comparison, inside / outside, no
   surface): a pixel whose decision byte differs from the float64 model's own is left out, at most 0.5 % of a frame.
   For the other pixels the tolerance per frame is four times the larger deviation from the float64 model of the two float32 models
   (csrc/taa.h's order of operations with exp2(g * log2 c), and the same with numpy.power), measured on the same inputs where they decide
   like the float64 model: another equally valid float32 evaluation order moves results by about that much.
 * Jitter removal (test_unjittered_motion_is_the_pixel_centre): four times the deviation of the same chain - projection of the surface
   position with the previous camera, unjitter - evaluated at float32 against float64 on the oracle's positions and cameras.
Measured figures: profiles/r13/taa.txt.
"""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import taa_model as M

LEFT_OUT_CAP = 0.005
COMBOS = [(True, False), (True, True), (False, False), (False, True)]      # (edge_dilation, anti_shimmer)


def _identity_motion(w, h, layers=1):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.repeat(np.stack([(xs + 0.5) / w, 1 - (ys + 0.5) / h], -1)[None], layers, 0).astype(np.float32)


def _camera_data(cams):
    return np.concatenate([c.pack() for c in cams])


def _default_cameras(n=1):
    from tauray_amd.scene import Camera
    return _camera_data([Camera() for _ in range(n)])


def _glb(name, size):
    from tauray_amd.gltf import load_glb
    return load_glb(os.path.join(GOLDEN, name), size[0], size[1])


# ======================================================================================================================
# CPU 1: the jitter of both hosts
def test_jitter_sequence_is_the_halton_sequence():
    from tauray_amd.scene import get_camera_jitter_sequence
    base2 = [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16]
    base3 = [1 / 3, 2 / 3, 1 / 9, 4 / 9, 7 / 9, 2 / 9, 5 / 9, 8 / 9]
    for n, size in ((8, (64, 48)), (3, (1920, 1080)), (1, (5, 3))):
        seq = get_camera_jitter_sequence(n, size)
        assert len(seq) == n
        for i, (jx, jy) in enumerate(seq):
            ex, ey = (base2[i] * 2 - 1) / size[0], (base3[i] * 2 - 1) / size[1]
            # float32 sums of at most three digits, one product, one difference, one quotient: a few ulps of the unit interval over the resolution
            assert abs(jx - ex) <= 4 * 2.0 ** -24 / size[0] and abs(jy - ey) <= 4 * 2.0 ** -24 / size[1], (n, i)
            assert abs(jx) <= 1.0 / size[0] and abs(jy) <= 1.0 / size[1]
    assert get_camera_jitter_sequence(0, (64, 48)) == []


def test_camera_pack_with_and_without_jitter():
    from tauray_amd.scene import Camera, get_camera_jitter_sequence, PROJ_ORTHOGRAPHIC
    cam = Camera(fov=50.0, aspect=1.5, fov_offset=(0.03, -0.02))
    cam.transform = np.array([[0.8, 0, 0.6, 1.0], [0, 1, 0, 2.0], [-0.6, 0, 0.8, 3.0], [0, 0, 0, 1.0]])
    plain = cam.pack()
    assert plain["pan"][0][2] == 0 and plain["pan"][0][3] == 0
    assert cam.get_jitter() == (0.0, 0.0)
    cam.step_jitter()                                     # no sequence: nothing to step
    assert cam.pack().tobytes() == plain.tobytes()
    zero = copy.deepcopy(cam)
    zero.set_jitter([(0.0, 0.0)])                         # a sequence that moves nothing moves nothing
    for name in ("view", "view_inverse", "view_proj", "origin", "dof_params", "projection_info", "pan"):
        assert zero.pack()[name].tobytes() == plain[name].tobytes(), name
    cam.set_jitter([])
    assert cam.pack().tobytes() == plain.tobytes()
    seq = get_camera_jitter_sequence(8, (64, 48))
    cam.set_jitter(seq)
    seen = []
    for step in range(9):
        j = cam.get_jitter()
        assert j == seq[step % 8]
        seen.append(j)
        packed = cam.pack()
        moved = copy.deepcopy(cam)
        moved.set_jitter([])
        moved.fov_offset = (cam.fov_offset[0] + j[0], cam.fov_offset[1] + j[1])       # projection[2][0..1] move by the jitter
        want = moved.pack()
        for name in ("view", "view_inverse", "view_proj", "origin", "dof_params", "projection_info"):
            assert packed[name].tobytes() == want[name].tobytes(), (step, name)
        # the inverse of a jittered projection is taken in closed form (both hosts, the same operations): its analytic zeros are exact zeros
        # where the LU inverse of the unjittered path leaves 1e-17
        assert np.abs(packed["proj_inverse"].astype(np.float64) - want["proj_inverse"]).max() <= 1e-15 * np.abs(want["proj_inverse"]).max()
        pan = packed["pan"][0]
        assert pan[2] == np.float32(j[0]) and pan[3] == np.float32(j[1])
        assert pan[0] == np.float32(np.float32(cam.fov_offset[0]) + np.float32(j[0])) and pan[1] == np.float32(np.float32(cam.fov_offset[1]) + np.float32(j[1]))
        cam.step_jitter()
    assert len(set(seen[:8])) == 8 and seen[8] == seen[0]
    ortho = Camera(projection=PROJ_ORTHOGRAPHIC)
    before = ortho.pack().tobytes()
    ortho.set_jitter(seq)
    ortho.step_jitter()
    assert ortho.pack().tobytes() == before               # jitter applies to perspective cameras only


def test_cpp_host_packs_the_same_jittered_cameras(tmp_path):
    from tauray_amd.scene import get_camera_jitter_sequence
    exe = str(tmp_path / "taa_jitter_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DTAURAY_HIP_WITH_ZLIB", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "taa_jitter_check.cc"), "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz",
                           "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    for name, size, n in (("test.glb", (64, 48), 8), ("animated.glb", (200, 120), 5)):
        out = subprocess.run([exe, os.path.join(GOLDEN, name), str(size[0]), str(size[1]), str(n), str(n + 1)], capture_output=True, text=True, check=True).stdout.split("\n")
        seq = get_camera_jitter_sequence(n, size)
        for i in range(n):
            tag, bx, by = out[i].split()
            assert tag == "jitter" and np.array([int(bx, 16), int(by, 16)], np.uint32).view(np.float32).tolist() == [seq[i][0], seq[i][1]], (name, i)
        scene = _glb(name, size)
        for cam in scene.cameras:
            cam.set_jitter(seq)
        for step in range(n + 2):
            if step:
                for cam in scene.cameras:
                    cam.step_jitter()
            tag, s, hexbytes = out[n + step].split()
            assert tag == "step" and int(s) == step
            assert bytes.fromhex(hexbytes) == scene.camera_data().tobytes(), f"{name}: the hosts pack different cameras at jitter step {step}"


# ======================================================================================================================
# CPU 2: the model against closed forms
def _brute_ranges(m):
    """lo / hi [11][h][w] with plain loops: the window of clamped neighbours."""
    h, w = m.shape[:2]
    lo = np.full((11, h, w), np.inf)
    hi = np.full((11, h, w), -np.inf)
    for y in range(h):
        for x in range(w):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = m[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]
                    r = M.AXES.astype(np.float64) @ q
                    lo[:, y, x] = np.minimum(lo[:, y, x], r - 1e-5)
                    hi[:, y, x] = np.maximum(hi[:, y, x], r + 1e-5)
    return lo, hi


def _run64(src, history, motion, alpha, gamma=2.2, anti_shimmer=False, have=True):
    L, h, w = src.shape[:3]
    cams = _default_cameras(L)
    model = M.TaaModel((w, h), L, alpha=alpha, gamma=gamma, edge_dilation=False, anti_shimmer=anti_shimmer)
    out = model.run(src, motion, None, np.zeros((L, h, w), np.int32), cams, cams, history=history, have_history=have)
    return out, model.decisions


def test_model_constant_image_comes_back_for_any_history():
    rng = np.random.default_rng(1)
    w, h = 16, 8
    sigma_min = np.linalg.svd(M.AXES.astype(np.float64), compute_uv=False).min()
    for shimmer in (False, True):
        src = np.empty((1, h, w, 4), np.float32)
        src[..., :3] = np.array([0.5, 0.25, 0.8], np.float32)
        src[..., 3] = 0.7
        history = rng.uniform(0, 3, (1, h, w, 4)).astype(np.float32)
        out, dec = _run64(src, history, _identity_motion(w, h), 0.125, anti_shimmer=shimmer)
        assert not (dec & M.OUTSIDE).any()
        # the clipped history lies in the k-DOP of half-width 1e-5 around map(c): |A x|_inf <= 1e-5 bounds |x| by sqrt(11) 1e-5 / sigma_min(A);
        # back through unmap, whose derivative at the mapped value m is d/dm m^(1/g) (times 1/m' = m under the logarithm)
        c = src[0, 0, 0, :3].astype(np.float64)
        m = c ** np.float64(np.float32(2.2))
        radius = np.sqrt(11) * 1e-5 / sigma_min
        slope = (1 / 2.2) * m ** (1 / 2.2 - 1) * (m if shimmer else 1.0)
        bound = 1.05 * (slope * radius).max()
        assert np.abs(out[..., :3] - c).max() <= bound
        assert np.array_equal(out[..., 3], src[..., 3].astype(np.float64))


def test_model_alpha_one_returns_the_input():
    rng = np.random.default_rng(2)
    w, h = 16, 8
    src = rng.uniform(0.01, 2, (2, h, w, 4)).astype(np.float32)
    history = rng.uniform(0, 2, (2, h, w, 4)).astype(np.float32)
    for shimmer in (False, True):
        out, _ = _run64(src, history, _identity_motion(w, h, 2), 1.0, anti_shimmer=shimmer)
        assert np.abs(out / src.astype(np.float64) - 1).max() <= 1e-13          # the map / unmap round trip at float64
        first, _ = _run64(src, history, _identity_motion(w, h, 2), 0.125, anti_shimmer=shimmer, have=False)       # no history: alpha = 1
        assert np.array_equal(first, out)


def test_model_unclipped_history_is_the_exponential_moving_average():
    rng = np.random.default_rng(3)
    w, h, N, alpha = 16, 8, 6, 0.25
    S = rng.uniform(0.1, 1.0, (1, h, w, 4)).astype(np.float32)
    pad = np.pad(S[0].astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H0 = sum(pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1))[None] / 9      # inside the window's hull
    hist = H0
    for n in range(1, N + 1):
        hist, dec = _run64(S, hist, _identity_motion(w, h), alpha, gamma=1.0)       # gamma 1: the map is the identity, the hull stays convex
        want = S + (1 - alpha) ** n * (H0 - S)
        assert np.abs(hist[..., :3] - want[..., :3]).max() <= 1e-12, n
        assert not dec.any() or set(np.unique(dec)) == {4}                         # offset (0, 0), inside, a surface


def test_model_history_outside_the_kdop_is_pulled_onto_its_boundary():
    rng = np.random.default_rng(4)
    w, h = 9, 7
    m = rng.uniform(0.2, 0.8, (h, w, 3))
    lo, hi = M.window_ranges(m, np.float64)
    blo, bhi = _brute_ranges(m)
    assert np.abs(lo - blo).max() <= 1e-15 and np.abs(hi - bhi).max() <= 1e-15      # the same window, up to the order of a dot product's sum
    flat = m.reshape(-1, 3)
    far = rng.uniform(3, 6, flat.shape) * rng.choice([-1.0, 1.0], flat.shape)
    clipped, length = M.kdop_clip(flat, far, lo.reshape(11, -1), hi.reshape(11, -1), np.float64)
    assert ((length > 0) & (length < 1)).all()
    proj = np.einsum("ak,nk->an", M.AXES.astype(np.float64), clipped)
    slack_lo, slack_hi = proj - lo.reshape(11, -1), hi.reshape(11, -1) - proj
    assert slack_lo.min() >= -1e-12 and slack_hi.min() >= -1e-12                   # inside the min / max of every axis
    assert (np.minimum(slack_lo, slack_hi).min(0) <= 1e-12).all()                  # and on the boundary of one
    inside, length = M.kdop_clip(flat, flat + 1e-7, lo.reshape(11, -1), hi.reshape(11, -1), np.float64)
    assert (length == 1).all() and np.array_equal(inside, flat + (flat + 1e-7 - flat))
    # an axis whose t0 / t1 is NaN (0 * inf: the dilation absorbed, no movement along the axis) does not decide the clip
    big = np.array([[4.0e6, 1.0, 1.0]], np.float32)
    lo32, hi32 = M.window_ranges(np.repeat(np.repeat(big[None], 3, 0), 3, 1).reshape(3, 3, 3), np.float32)
    assert lo32[0, 1, 1] == big[0, 0]                                              # 1e-5 is absorbed at 4e6
    c32, l32 = M.kdop_clip(big, big + np.array([[0.0, 0.5, 0.0]], np.float32), lo32[:, 1, 1][:, None], hi32[:, 1, 1][:, None], np.float32)
    assert np.isfinite(c32).all() and np.isfinite(l32).all()


def test_model_bicubic_identity_and_outside():
    rng = np.random.default_rng(5)
    w, h = 16, 8
    hist = rng.uniform(0, 2, (h, w, 4))
    ys, xs = np.mgrid[0:h, 0:w]
    got = M.bicubic(hist, ((xs + 0.5) / w).ravel(), ((ys + 0.5) / h).ravel(), np.float64)
    assert np.array_equal(got, hist[..., :3].reshape(-1, 3))                      # the centre texel, exactly
    # the filter reproduces a linear ramp between texel centres (Catmull-Rom interpolates polynomials up to degree 2)
    ramp = np.repeat((np.arange(w) * 0.1)[None, :, None], h, 0).repeat(4, 2)
    at = M.bicubic(ramp, np.array([5.25 / w]), np.array([3.5 / h]), np.float64)
    assert np.abs(at - 0.475).max() <= 1e-14
    src = rng.uniform(0, 1, (1, h, w, 4)).astype(np.float32)
    motion = _identity_motion(w, h)
    motion[0, 2, 3] = (-0.2, 0.5)
    motion[0, 4, 5] = (0.5, 1.4)
    motion[0, 6, 7] = (1.0 + 3.0 / w, 0.5)
    out, dec = _run64(src, rng.uniform(0, 1, (1, h, w, 4)).astype(np.float32), motion, 0.125)
    for y, x in ((2, 3), (4, 5), (6, 7)):
        assert dec[0, y, x] & M.OUTSIDE and np.array_equal(out[0, y, x], src[0, y, x].astype(np.float64))
    assert ((dec & M.OUTSIDE) != 0).sum() == 3


# ======================================================================================================================
# CPU 3 and 4: on the oracle's targets
@functools.lru_cache(maxsize=None)
def _oracle_sequence(size, frames, jitter):
    """test.glb, static, a fixed perspective camera with a jitter sequence: per frame the oracle's targets and the camera pair."""
    from oracle import binding as B
    from tauray_amd.scene import get_camera_jitter_sequence
    w, h = size
    scene = _glb("test.glb", size)
    cam = scene.cameras[0]
    cam.set_jitter(get_camera_jitter_sequence(jitter, size))
    opt = B.options_for_scene(scene, max_bounces=3)
    out = []
    prev_cam = copy.deepcopy(cam)
    for f in range(frames):
        cam.step_jitter()
        osc = B.OracleScene(scene)
        osc.set_previous_cameras([prev_cam])
        t = osc.render_pt_targets(opt, w, h, ["color", "screen_motion", "pos", "instance_id"], frame_counter=f, samples_accumulated=0)
        out.append(dict(src=B.tonemap(t["color"]).astype(np.float32), motion=t["screen_motion"], pos=t["pos"], ids=t["instance_id"][..., 0],
                        cur=_camera_data([cam]), prev=_camera_data([prev_cam])))
        prev_cam = copy.deepcopy(cam)
    return out


def _projected_unjittered(pos, cur, prev, dt):
    """get_camera_projection(previous, pos) then the unjitter, for a static scene: where a surface pixel's own position was last frame."""
    p = pos.astype(dt)
    c = M._mul(M._mat(prev, "view_proj", dt), p[..., 0], p[..., 1], p[..., 2], dt(1))
    mo = np.stack([(c[0] / c[3]) * dt(0.5) + dt(0.5), (c[1] / c[3]) * dt(0.5) + dt(0.5)], -1)
    uv, _, _, _ = M.reprojected_uv(mo, None, None, cur, prev, False, True, dt)
    return uv


def test_unjittered_motion_is_the_pixel_centre(oracle):
    size = (64, 48)
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    centre = np.stack([(xs + 0.5) / w, (ys + 0.5) / h], -1)
    worst = bound_min = 0.0
    for f, t in enumerate(_oracle_sequence(size, 9, 8)):
        surf = t["ids"][0] >= 0
        assert surf.mean() > 0.3
        uv, _, _, nosurf = M.reprojected_uv(t["motion"][0], None, t["ids"][0], t["cur"][0], t["prev"][0], False, True, np.float64)
        assert np.array_equal(nosurf, ~surf)
        dev = float(np.abs(uv[surf] - centre[surf]).max())
        u32 = _projected_unjittered(t["pos"][0], t["cur"][0], t["prev"][0], np.float32)
        u64 = _projected_unjittered(t["pos"][0], t["cur"][0], t["prev"][0], np.float64)
        bound = 4 * float(np.abs(u32[surf].astype(np.float64) - u64[surf]).max())
        print(f"\nTAA unjitter frame {f}: |uv - centre| max {dev:.3e}, float32 chain vs float64 {bound / 4:.3e}, bound {bound:.3e}; jitter {t['cur'][0]['pan'][2:]}")
        assert dev <= bound, f"frame {f}: the unjittered motion of a surface pixel is {dev:.3e} from its centre (bound {bound:.3e})"
        if f:
            assert np.abs(t["cur"][0]["pan"][2:] - t["prev"][0]["pan"][2:]).max() > 0.1 / max(size)      # the frames are jittered against each other
        worst, bound_min = max(worst, dev), bound


def test_float32_models_decide_like_the_float64_model_on_oracle_targets(oracle):
    """The condition of the 0.5 % allowance and the yardstick of the GPU test, exercised without a GPU: test.glb 64 x 48, fixed camera, a
    jitter sequence of 8, 8 frames; every model variant continues from the float64 model's history, as the stage's comparison does."""
    size = (64, 48)
    worst = {}
    for edge, shimmer in COMBOS:
        kw = dict(alpha=1 / 8, gamma=2.2, edge_dilation=edge, anti_shimmer=shimmer)
        m64 = M.TaaModel(size, **kw)
        variants = [M.TaaModel(size, dtype=np.float32, **kw), M.TaaModel(size, dtype=np.float32, pow_mode="power", **kw)]
        hist = None
        for f, t in enumerate(_oracle_sequence(size, 8, 8)):
            args = (t["src"], t["motion"], t["pos"], t["ids"], t["cur"], t["prev"])
            h32 = None if hist is None else hist.astype(np.float32)
            o64 = m64.run(*args, history=h32, have_history=hist is not None)
            for v in variants:
                o = v.run(*args, history=h32, have_history=hist is not None)
                share = float((v.decisions != m64.decisions).mean())
                assert share <= LEFT_OUT_CAP, f"frame {f} {kw}: {share:.3%} of the pixels decide differently at float32"
                assert np.isfinite(o).all()
                same = v.decisions == m64.decisions
                dev = float(np.abs(o[same].astype(np.float64) - o64[same]).max())
                worst[(edge, shimmer)] = max(worst.get((edge, shimmer), 0.0), dev)
                # display values lie in [0, 1]: a float32 evaluation that moved one by 2^-10 would be visible at ten bits.  Not under
                # anti-shimmer: there a dark, flat window has a k-DOP of half-width 1e-5 in log space, the bicubic filter's float32 rounding
                # (1e-7 of the bright texels under its negative lobes) is 1e-5 relative to a dark history value, the logarithm makes that an
                # absolute 2e-5, and the clip length along the flat axis is 1e-5 over that - anywhere in [0, 1] at either precision
                if not shimmer:
                    assert dev <= 2.0 ** -10, f"frame {f} {kw}: float32 deviates {dev:.3e}"
            if f:
                assert not (m64.decisions & M.OUTSIDE).all()
            hist = o64
    print("\nTAA float32 models vs float64 on oracle targets, largest deviation per (edge dilation, anti-shimmer): " + ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))


# ======================================================================================================================
# CPU: the boundary
TAA_SYMBOLS = ("trhip_taa_create", "trhip_taa_destroy", "trhip_taa_run", "trhip_taa_reset_history", "trhip_taa_get_timings", "trhip_taa_download")


def test_taa_symbols_resolve_and_create_refuses_bad_arguments():
    from tauray_amd import _lib
    L = _lib.lib()
    for n in TAA_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.TaaOptionsC) == 24 and C.sizeof(_lib.TaaImagesC) == 5 * 8 and C.sizeof(_lib.TaaTimingsC) == 72
    out = C.c_void_p()

    def err(opt, w, h, layers):
        rc = L.trhip_taa_create(None, C.byref(opt) if opt is not None else None, w, h, layers, C.byref(out))
        assert rc != 0 and not out.value
        return L.trhip_last_error().decode()
    good = lambda **kw: _lib.TaaOptionsC(**dict(dict(alpha=0.125, gamma=2.2, edge_dilation=1, anti_shimmer=0, base_camera_index=0, projection=0), **kw))
    assert "zero" in err(good(), 0, 64, 1) and "zero" in err(good(), 64, 0, 1) and "zero" in err(good(), 64, 64, 0)
    for a in (0.0, -0.5, 1.5, float("nan")):
        assert "alpha" in err(good(alpha=a), 64, 64, 1)
    assert "equirectangular" in err(good(projection=2), 64, 64, 1)
    assert "options" in err(None, 64, 64, 1)
    assert "device" in err(good(), 64, 64, 1) and "device" in err(good(alpha=1.0, projection=1), 64, 64, 1)      # good arguments, no device: no CPU fallback
    assert L.trhip_taa_run(None, None, None) != 0 and L.trhip_taa_reset_history(None) != 0


def test_renderer_refuses_what_taa_cannot_do():
    from tauray_amd import renderer as R
    opt = R.make_options()
    with pytest.raises(ValueError, match="gathering them from several is not built"):
        R.RtRenderer(None, None, opt, (64, 64), world_size=2, rank=0, taa=8)
    with pytest.raises(ValueError, match="accumulate must be False"):
        R.RtRenderer(None, None, opt, (64, 64), taa=8, accumulate=True)
    with pytest.raises(ValueError, match="frames_per_launch must be 1"):
        R.RtRenderer(None, None, opt, (64, 64), taa=8, frames_per_launch=2)
    with pytest.raises(ValueError, match="reprojection and taa is not built"):
        R.RtRenderer(None, None, opt, (64, 64), taa=8, temporal_reprojection=0.5)
    with pytest.raises(ValueError, match="reprojection and taa is not built"):
        R.RtRenderer(None, None, opt, (64, 64), taa=8, viewports=4, spatial_reprojection=[0, 2])
    with pytest.raises(ValueError, match="equirectangular"):
        R.RtRenderer(None, None, R.make_options(projection=2), (64, 64), taa=8)
    with pytest.raises(ValueError, match="must be positive"):
        R.RtRenderer(None, None, opt, (64, 64), taa=-1)


def test_cli_knows_the_taa_option():
    exe = os.path.join(ROOT, "tauray_amd", "tauray_hip")
    h = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--taa=N" in h.stdout + h.stderr and "anti-shimmer" in h.stdout + h.stderr
    glb = os.path.join(GOLDEN, "test.glb")
    for args, word in ((["--taa=0"], "sequence"), (["--taa=x"], "sequence"), (["--taa=8,edge-dilation=maybe"], "neither on nor off"), (["--taa=8,bogus=1"], "--taa=N"),
                       (["--taa=8", "--accumulation"], "accumulation"), (["--taa=8", "--frames-per-launch=2"], "frames-per-launch"),
                       (["--taa=8", "--temporal-reprojection=0.5"], "reprojection"), (["--taa=8", "--fake-devices=2"], "one device"),
                       (["--taa=8", "--renderer=direct"], "path-tracer")):
        r = subprocess.run([exe, glb, "--width=32", "--height=32", "--headless=/dev/null"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


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


def _set_camera_data(R, ctx, ss, cur, prev):
    """The packed cameras of a recorded frame back onto the device."""
    from tauray_amd import _lib
    cur = np.ascontiguousarray(cur)
    R.check(_lib.lib().trhip_scene_update_cameras(ctx.h, cur.ctypes.data, len(cur)))
    ss.camera_data = cur
    ss.set_previous_camera_data(prev)


def _orbit(cam0, angle):
    c = copy.deepcopy(cam0)
    ca, sa = np.cos(angle), np.sin(angle)
    rot = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1.0]])
    c.transform = rot @ np.asarray(cam0.transform, float)
    return c


_CARRIER = {}


def _carrier(R, ctx, cameras=2):
    """A scene stage whose cameras the synthetic sequences overwrite (the stage reads the device scene's cameras)."""
    if cameras not in _CARRIER:
        from tauray_amd import scene as S
        scene = _glb("test.glb", (32, 32))
        if cameras > 1:
            scene.cameras = S.generate_camera_grid(scene.cameras[0], cameras, 1, 0.3, 0.3, 5.0)
        _CARRIER[cameras] = (R.SceneStage(ctx, scene), scene)
    return _CARRIER[cameras]


@functools.lru_cache(maxsize=None)
def _synthetic_sequence(size, layers, frames, seed=7, value=None):
    """Random colours, motions around the identity with some pointing outside, random depths, some pixels without a surface; cameras of
    test.glb's grid, jittered."""
    from tauray_amd import scene as S
    from tauray_amd.scene import get_camera_jitter_sequence
    rng = np.random.default_rng(seed)
    w, h = size
    cams = S.generate_camera_grid(_glb("test.glb", (32, 32)).cameras[0], layers, 1, 0.3, 0.3, 5.0) if layers > 1 else [_glb("test.glb", (32, 32)).cameras[0]]
    for c in cams:
        c.set_jitter(get_camera_jitter_sequence(8, size))
    prev = _camera_data(cams)
    out = []
    for f in range(frames):
        for c in cams:
            c.step_jitter()
        cur = _camera_data(cams)
        src = rng.uniform(0, 1.5, (layers, h, w, 4)).astype(np.float32)
        src[rng.uniform(size=(layers, h, w)) < 0.05] = 0.0                       # black pixels: the map's c <= 0 branch
        if value is not None:
            src[...] = value
        motion = _identity_motion(w, h, layers) + rng.uniform(-3, 3, (layers, h, w, 2)).astype(np.float32) / np.array([w, h], np.float32)
        far = rng.uniform(size=(layers, h, w)) < 0.1
        motion[far] += rng.uniform(-1.5, 1.5, (int(far.sum()), 2)).astype(np.float32)
        pos = np.zeros((layers, h, w, 4), np.float32)
        pos[..., :3] = rng.uniform(-4, 4, (layers, h, w, 3))
        ids = rng.integers(0, 5, (layers, h, w)).astype(np.int32)
        ids[rng.uniform(size=(layers, h, w)) < 0.15] = -1
        out.append(dict(src=src, motion=motion.astype(np.float32), pos=pos, ids=ids, cur=cur, prev=prev))
        prev = cur
    return out


def _render_sequence(R, ctx, scene, size, frames, jitter=8, cameras_of_frame=None, animate=None, bmfr=False, **opt_kw):
    """Frames of a scene as the renderer's chain produces them - path tracer, (BMFR,) tonemap - with the cameras jittered: per frame the
    downloaded display-space colour, screen motion, pos, instance id and the camera pair on the device."""
    from tauray_amd.scene import get_camera_jitter_sequence
    w, h = size
    layers = len(scene.cameras)
    seq = get_camera_jitter_sequence(jitter, size)
    for c in scene.cameras:
        c.set_jitter(seq)
    ss = R.SceneStage(ctx, scene)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, **opt_kw), _dup(size))
    names = R.BmfrStage.FEATURES if bmfr else ("color", "screen_motion", "pos", "instance_id")
    bufs = {n: ctx.alloc(layers * w * h * R.PathTracerStage.TARGETS[n][0] * 4).zero() for n in names}
    stage = R.BmfrStage(ctx, size, layers) if bmfr else None
    disp = ctx.alloc(layers * w * h * 16)
    tm = R.TonemapStage(ctx)
    prev = ss.camera_data.copy()
    out = []
    for f in range(frames):
        if animate is not None:
            animate(ss, f)
        cams = cameras_of_frame(f) if cameras_of_frame is not None else scene.cameras
        if cameras_of_frame is not None:
            for c in cams:
                c.set_jitter(seq)
                c.jitter_index = f % jitter
        for c in cams:
            c.step_jitter()
        ss.update_cameras(cams)
        ss.set_previous_camera_data(prev)
        pt.reset_accumulated_samples()
        pt.run_targets(bufs, layers)
        if stage is not None:
            stage.run(bufs, f)
        tm.run(bufs["color"], disp, w, h, layers)
        ctx.sync()
        out.append(dict(src=disp.download((layers, h, w, 4)), motion=bufs["screen_motion"].download((layers, h, w, 2)),
                        pos=bufs["pos"].download((layers, h, w, 4)), ids=bufs["instance_id"].download((layers, h, w), np.int32),
                        cur=ss.camera_data.copy(), prev=prev.copy()))
        prev = ss.camera_data.copy()
    if stage is not None:
        stage.close()
    pt.close()
    return out


_SCENE_SEQUENCES = {}


def _scene_sequence(R, ctx, case):
    """(frames, perspective) of a rendered sequence, rendered once per session."""
    if case not in _SCENE_SEQUENCES:
        _SCENE_SEQUENCES[case] = _render_scene_sequence(R, ctx, case)
    return _SCENE_SEQUENCES[case]


def _render_scene_sequence(R, ctx, case):
    if case == "glb-fixed":
        return _render_sequence(R, ctx, _glb("test.glb", (200, 120)), (200, 120), 16, max_bounces=3), True
    if case == "glb-orbit":
        scene = _glb("test.glb", (200, 120))
        cam0 = copy.deepcopy(scene.cameras[0])
        return _render_sequence(R, ctx, scene, (200, 120), 8, cameras_of_frame=lambda f: [_orbit(cam0, 0.02 * f)], max_bounces=3), True
    if case == "animated":
        from tauray_amd.animation import SceneAnimator
        scene = _glb("animated.glb", (128, 96))
        holder = {}

        def animate(ss, f):
            if "a" not in holder:
                holder["a"] = SceneAnimator(ss.scene)
                holder["a"].play("", loop=True)
            ss.animate(holder["a"], 0 if f == 0 else round(1000000.0 / 24.0))
        return _render_sequence(R, ctx, scene, (128, 96), 6, animate=animate, max_bounces=3), True
    if case == "envmap":
        from tauray_amd.hdr import set_envmap
        scene = set_envmap(_glb("test.glb", (128, 96)), os.path.join(GOLDEN, "sky.hdr"))
        return _render_sequence(R, ctx, scene, (128, 96), 5, max_bounces=3), True
    if case == "orthographic":
        from tauray_amd.scene import PROJ_ORTHOGRAPHIC
        scene = _glb("test.glb", (128, 96))
        cam = scene.cameras[0]
        cam.projection = PROJ_ORTHOGRAPHIC
        cam.ortho = (-6.0, 6.0, -4.5, 4.5, 0.1, 10.0)       # the ray origins lie in front of the room: about two thirds of the pixels see a surface
        cam0 = copy.deepcopy(cam)
        return _render_sequence(R, ctx, scene, (128, 96), 5, cameras_of_frame=lambda f: [_orbit(cam0, 0.01 * f)], max_bounces=3), False
    raise KeyError(case)


def _compare_sequence(R, ctx, label, ss, frames, edge, shimmer, perspective=True, use_id=True):
    """Runs the recorded frames through a stage, each against the models one step at a time."""
    L, h, w = frames[0]["src"].shape[:3]
    size = (w, h)
    kw = dict(alpha=1 / 8, gamma=2.2, edge_dilation=edge, anti_shimmer=shimmer)
    stage = R.TaaStage(ctx, size, L, dict(kw, projection=0 if perspective else 1))
    m64 = M.TaaModel(size, L, perspective=perspective, **kw)
    variants = [M.TaaModel(size, L, perspective=perspective, dtype=np.float32, **kw), M.TaaModel(size, L, perspective=perspective, dtype=np.float32, pow_mode="power", **kw)]
    dst = ctx.alloc(L * h * w * 16).zero()
    worst = dict(left_out=0.0, model=0.0, gpu=0.0, ratio=0.0, surface_min=1.0, blended_min=1.0, miss_blended_max=0.0)
    for f, t in enumerate(frames):
        _set_camera_data(R, ctx, ss, t["cur"], t["prev"])
        ids = t["ids"] if use_id else None
        bufs = dict(src=ctx.alloc(t["src"].nbytes).upload(t["src"]), dst=dst, screen_motion=ctx.alloc(t["motion"].nbytes).upload(t["motion"]),
                    pos=ctx.alloc(t["pos"].nbytes).upload(t["pos"]), instance_id=ctx.alloc(t["ids"].nbytes).upload(t["ids"]) if use_id else None)
        before = stage.download("history")
        stage.run(bufs)
        got, hist, dec = dst.download((L, h, w, 4)), stage.download("history"), stage.download("decisions")
        assert got.tobytes() == hist.tobytes(), f"{label} frame {f}: dst and the new history differ"
        assert np.isfinite(got).all(), f"{label} frame {f}: not finite"
        args = (t["src"], t["motion"], t["pos"], ids, t["cur"], t["prev"])
        o64 = m64.run(*args, history=before, have_history=f > 0)
        left_out = dec != m64.decisions
        share = float(left_out.mean())
        keep = ~left_out
        model_dev = 0.0
        for v in variants:
            o = v.run(*args, history=before, have_history=f > 0)
            same = keep & (v.decisions == m64.decisions)
            model_dev = max(model_dev, float(np.abs(o[same].astype(np.float64) - o64[same]).max()) if same.any() else 0.0)
        gpu_dev = float(np.abs(got[keep].astype(np.float64) - o64[keep]).max()) if keep.any() else 0.0
        worst["left_out"], worst["model"], worst["gpu"] = max(worst["left_out"], share), max(worst["model"], model_dev), max(worst["gpu"], gpu_dev)
        worst["ratio"] = max(worst["ratio"], gpu_dev / model_dev if model_dev > 0 else (0.0 if gpu_dev == 0 else np.inf))
        blended = (dec & M.OUTSIDE) == 0
        worst["surface_min"] = min(worst["surface_min"], float((t["ids"] >= 0).mean()))
        if f:
            worst["blended_min"] = min(worst["blended_min"], float(blended.mean()))
            worst["miss_blended_max"] = max(worst["miss_blended_max"], float((blended & ((dec & M.NO_SURFACE) != 0)).mean()))
        print(f"TAA stage [{label}] frame {f}: left out {share:.4%}, model32 {model_dev:.3e}, gpu {gpu_dev:.3e}")
        assert share <= LEFT_OUT_CAP, f"{label} frame {f}: {share:.3%} of the pixels decide differently from the model"
        assert gpu_dev <= 4 * model_dev, f"{label} frame {f}: deviates {gpu_dev:.3e} from the float64 model, the float32 models {model_dev:.3e}"
        assert np.array_equal(got[..., 3], t["src"][..., 3]), f"{label} frame {f}: alpha must pass through"
    print(f"\nTAA stage [{label}] {w}x{h}x{L} edge {edge} shimmer {shimmer}, {len(frames)} frames: left out max {worst['left_out']:.4%}, "
          f"model32 {worst['model']:.2e}, gpu {worst['gpu']:.2e}, worst ratio {worst['ratio']:.2f}; surface pixels min {worst['surface_min']:.1%}, "
          f"blended (not passed through) min {worst['blended_min']:.1%}, misses blended max {worst['miss_blended_max']:.1%}")
    stage.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("edge,shimmer", COMBOS)
@pytest.mark.parametrize("case", ["synthetic-37x23x2", "synthetic-5x3"])
def test_stage_is_the_model_on_synthetic_images(R, ctx, case, edge, shimmer):
    """Measured on one MI355X (profiles/r13/taa.txt): no pixel left out; 37 x 23 x 2: largest deviation from the float64 model 1.1e-5 to
    1.8e-5 for the float32 models and the kernel alike, worst per-frame ratio 1.03; 5 x 3: 2.7e-7 to 3.7e-6, worst ratio 1.49 (edge dilation
    and anti-shimmer).  Fifteen pixels have none in the ill-conditioned regime that dominates larger images, so that figure is the accuracy
    of the colour map's exp2 / log2 / log / exp alone: the kernel takes them at double, rounded once (csrc/taa.h); with the device library's
    float versions (one to two ulps against numpy's half) this case shows 5.4."""
    size, layers = ((37, 23), 2) if case == "synthetic-37x23x2" else ((5, 3), 1)
    ss, _ = _carrier(R, ctx, layers)
    _compare_sequence(R, ctx, case, ss, _synthetic_sequence(size, layers, 4), edge, shimmer)


@pytest.mark.gpu
@pytest.mark.parametrize("edge,shimmer", COMBOS)
def test_stage_is_the_model_on_test_glb(R, ctx, edge, shimmer):
    """test.glb 200 x 120, fixed camera, jitter 8, 16 frames of the path tracer -> tonemap chain, every option combination.
    Under anti-shimmer the float32 models themselves deviate by 0.3 to 0.5 from the float64 model on this scene (dark flat windows whose clip
    length is ill-conditioned at either precision: DESIGN.md section 16), so the value bound is loose there: those two combinations hold the
    decisions, finiteness and alpha; anti-shimmer values are held tightly (1e-5) by the synthetic sequences."""
    frames, perspective = _scene_sequence(R, ctx, "glb-fixed")
    ss, _ = _carrier(R, ctx, 1)
    _assert_not_trivial("glb-fixed", _compare_sequence(R, ctx, "glb-fixed", ss, frames, edge, shimmer, perspective))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["glb-orbit", "animated", "envmap", "envmap-no-id", "orthographic"])
def test_stage_is_the_model_on_scenes(R, ctx, case):
    frames, perspective = _scene_sequence(R, ctx, "envmap" if case == "envmap-no-id" else case)
    ss, _ = _carrier(R, ctx, 1)
    worst = _compare_sequence(R, ctx, case, ss, frames, True, False, perspective, use_id=(case != "envmap-no-id"))
    _assert_not_trivial(case, worst)
    if case in ("envmap", "orthographic"):      # the sequences that are there for their misses: they are blended, not passed through
        assert worst["miss_blended_max"] >= 0.01, f"{case}: no pixel without a surface goes through the history read"


def _assert_not_trivial(label, worst):
    """A sequence compares something: surfaces in every frame, most pixels blended with the history after the first frame, and float32
    models that differ from the float64 model (a bound of zero would hold for a frame that is passed through)."""
    assert worst["surface_min"] >= 0.05, f"{label}: {worst['surface_min']:.1%} surface pixels"
    assert worst["blended_min"] >= 0.5, f"{label}: only {worst['blended_min']:.1%} of a frame is blended with the history"
    assert worst["model"] > 0, f"{label}: the float32 models do not deviate from the float64 model: nothing is compared"


# ---- properties that need no model
def _run_frames(R, ctx, ss, frames, opts, stream=None, stage=None, alias=False):
    L, h, w = frames[0]["src"].shape[:3]
    own = stage is None
    stage = stage or R.TaaStage(ctx, (w, h), L, opts)
    outs = []
    for t in frames:
        _set_camera_data(R, ctx, ss, t["cur"], t["prev"])
        src = ctx.alloc(t["src"].nbytes).upload(t["src"])
        dst = src if alias else ctx.alloc(t["src"].nbytes).zero()
        ctx.sync()
        stage.run(dict(src=src, dst=dst, screen_motion=ctx.alloc(t["motion"].nbytes).upload(t["motion"]), pos=ctx.alloc(t["pos"].nbytes).upload(t["pos"]),
                       instance_id=ctx.alloc(t["ids"].nbytes).upload(t["ids"])), stream)
        ctx.sync(stream)
        outs.append(dst.download((L, h, w, 4)))
    if own:
        stage.close()
    return outs


@pytest.mark.gpu
def test_runs_are_bit_reproducible_and_reset_history_starts_over(R, ctx):
    frames = _synthetic_sequence((37, 23), 2, 4)
    ss, _ = _carrier(R, ctx, 2)
    opts = dict(alpha=1 / 8, gamma=2.2, edge_dilation=True, anti_shimmer=True)
    a = _run_frames(R, ctx, ss, frames, opts)
    b = _run_frames(R, ctx, ss, frames, opts)
    stream = ctx.create_stream()
    c = _run_frames(R, ctx, ss, frames, opts, stream=stream)
    ctx.destroy_stream(stream)
    d = _run_frames(R, ctx, ss, frames, opts, alias=True)                       # dst = src goes through the new history
    for f in range(len(frames)):
        assert a[f].tobytes() == b[f].tobytes() == c[f].tobytes() == d[f].tobytes(), f"frame {f}"
    stage = R.TaaStage(ctx, (37, 23), 2, opts)
    _run_frames(R, ctx, ss, frames[2:], opts, stage=stage)
    stage.reset_history()
    again = _run_frames(R, ctx, ss, frames, opts, stage=stage)
    t = stage.timings()
    assert t["name"] == "temporal antialiasing (2 viewports)" and t["frames"] == 6 and t["total_ms"] > 0
    stage.close()
    for f in range(len(frames)):
        assert again[f].tobytes() == a[f].tobytes(), f"frame {f} after reset_history"


@pytest.mark.gpu
def test_first_frame_finite_outputs_and_alpha(R, ctx):
    ss, _ = _carrier(R, ctx, 2)
    frames = _synthetic_sequence((37, 23), 2, 3)
    for edge, shimmer in COMBOS:
        opts = dict(alpha=1 / 8, gamma=2.2, edge_dilation=edge, anti_shimmer=shimmer)
        outs = _run_frames(R, ctx, ss, frames, opts)
        src = frames[0]["src"]
        # the first frame: unmap(map(c)), two powers (and a logarithm and an exponential) at float32, each a few ulps scaled by its
        # exponent g |log2 c| <= 2.2 * 24 over the colours used; black stays black except under anti-shimmer, where map(0) = -10
        lit = src[..., :3] > 1e-2
        rel = np.abs(outs[0][..., :3][lit] / src[..., :3][lit] - 1)
        assert rel.max() <= 64 * 2.0 ** -23, (edge, shimmer, rel.max())
        if not shimmer:
            assert (outs[0][..., :3][src[..., :3] == 0] == 0).all()
        for f, o in enumerate(outs):
            assert np.isfinite(o).all()
            assert np.array_equal(o[..., 3], frames[f]["src"][..., 3])
        bright = _run_frames(R, ctx, ss, _synthetic_sequence((37, 23), 2, 3, value=1000.0), opts)         # 1000^2.2 = 4e6 absorbs the 1e-5 dilation
        for o in bright:
            assert np.isfinite(o).all() and np.abs(o[..., :3] / 1000.0 - 1).max() <= 64 * 2.0 ** -23


# ---- it antialiases
@pytest.mark.gpu
def test_it_antialiases(R, ctx):
    """test.glb, fixed camera, 1 spp per frame with BMFR, jitter 8, frame 16: RMS error against a 1024-spp reference (box film of one pixel,
    tonemapped) over the pixels within two pixels of an instance-id edge, with TAA and without.  Measured: profiles/r13/taa.txt."""
    from tauray_amd import renderer as RR
    size = (200, 120)
    w, h = size
    scene = _glb("test.glb", size)
    ss = R.SceneStage(ctx, scene)
    ref_pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=3, film=RR.FILM_BOX, film_radius=0.5), _dup(size))
    ref_buf, ref_disp = ctx.alloc(w * h * 16).zero(), ctx.alloc(w * h * 16)
    for _ in range(1024):
        ref_pt.run(ref_buf)
    R.TonemapStage(ctx).run(ref_buf, ref_disp, w, h)
    ref = ref_disp.download((h, w, 4))
    ref_pt.close()
    figures = {}
    ids = None
    for taa in (0, 8):
        scene = _glb("test.glb", size)
        r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), size, denoiser="bmfr", taa=taa)
        for f in range(17):
            r.render()
        img = r.download("display")[0]
        if taa:
            ids = r.current.features["instance_id"].download((h, w), np.int32)
            assert r.post.taa.timings()["frames"] == 17
        r.close()
        figures[taa] = img
    edge = np.zeros((h, w), bool)
    edge[:, 1:] |= ids[:, 1:] != ids[:, :-1]
    edge[1:, :] |= ids[1:, :] != ids[:-1, :]
    near = edge.copy()
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near |= np.roll(np.roll(edge, dy, 0), dx, 1)
    near &= np.isfinite(ref).all(-1)                 # the path tracer's rare NaN sample
    assert near.mean() > 0.02
    rms = {k: float(np.sqrt(((v[..., :3][near] - ref[..., :3][near]) ** 2).mean())) for k, v in figures.items()}
    print(f"\nTAA antialiasing: edge pixels {near.mean():.2%}; RMS error at edges without TAA {rms[0]:.4f}, with TAA {rms[8]:.4f}, ratio {rms[8] / rms[0]:.3f}")
    assert rms[8] < rms[0]


# ---- the hosts
@pytest.mark.gpu
def test_renderer_and_cli_produce_the_same_frames(R, ctx, tmp_path):
    """RtRenderer(taa=8) and tauray_hip --taa=8 --headless: the same display frames of test.glb, within the tolerance the C++-host tests use
    between the two hosts (tests/test_cpp_host.py)."""
    W, H, frames = 160, 120, 6
    glb = os.path.join(GOLDEN, "test.glb")
    exe = os.path.join(ROOT, "tauray_amd", "tauray_hip")
    for extra, kw in (([], {}), (["--denoiser=bmfr"], dict(denoiser="bmfr"))):
        prefix = str(tmp_path / ("t" + str(len(extra))))
        subprocess.check_call([exe, glb, f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--filetype=raw", "--taa=8", f"--frames={frames}", f"--headless={prefix}"] + extra)
        scene = _glb("test.glb", (W, H))
        r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), taa=8, **kw)
        plain, one_slot = None, []
        for f in range(frames):
            r.render()
            ref = r.download("display")[0]
            one_slot.append(ref)
            got = np.fromfile(f"{prefix}{f}.raw", dtype=np.float32).reshape(H, W, 4)
            differing = float((np.abs(got - ref).max(-1) > 1e-3).mean())
            assert differing < 2e-3 and abs(float(got.mean()) - float(ref.mean())) < 1e-4, f"{extra} frame {f}: {differing:.4%} of the pixels differ"
            if f == 0:
                plain = ref
        assert float((np.abs(plain - ref).max(-1) > 1e-3).mean()) > 0.01, "the history does nothing"
        r.close()
        # two frames in flight: the stage's history is one chain in frame order, the same frames bit for bit
        scene = _glb("test.glb", (W, H))
        r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), taa=8, frames_in_flight=2, **kw)
        for f in range(frames):
            r.render()
            assert r.download("display")[0].tobytes() == one_slot[f].tobytes(), f"{extra} frame {f} differs with two frames in flight"
        r.close()
