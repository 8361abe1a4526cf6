"""The BMFR denoiser stage (trhip_bmfr_*, csrc/bmfr.hip) against tests/bmfr_model.py, a numpy model written
from the algorithm, and against properties that need no model.

How the bounds are set.  Nothing is compared against a figure taken from the code under test.
 * The fit (test_fit_is_least_squares).  Per block and channel b the fitted values of the GPU's weights w must be within c |b| of the
   optimum's: |A (w - w*)|_2 <= c |b|_2 at float64, w* = numpy.linalg.lstsq at float64.  c is measured when the test runs: the model's
   own float32 Householder QR on the same matrices, in the given row order and in one permuted row order; per family the largest
   |A (w32 - w*)| / |b| it shows, times four (another equally valid reduction order moves float32 results by about that much).
 * The stage (test_stage_is_the_model).  Reprojection has thresholds (cos > 0.9, the position test, inside / outside), so a tap can be
   kept by one implementation and dropped by the other: a pixel whose accept bits differ from the float64 model's own is left out of the
   comparison, at most 0.5 % of a frame, and the model then continues with the stage's bits so that one such pixel
   does not make the rest of its block and of the sequence incomparable.  For the other pixels the tolerance per frame and quantity is four
   times the largest deviation of the float32 model from the float64 model on the same inputs and bits.  History lengths must be equal
   (to the float32 rounding of a bilinear blend of lengths <= 255: 1e-4).
Measured figures: profiles/r10/bmfr.txt.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import bmfr_model as M

LEFT_OUT_CAP = 0.005
FEATURE_NAMES = ("color", "diffuse", "albedo", "normal", "pos", "screen_motion", "instance_id")


# ======================================================================================================================
# CPU: the model against closed forms
def _oct_pack(n):
    n = n / np.abs(n).sum(-1, keepdims=True)
    return np.where(n[..., 2:3] >= 0, n[..., :2], (1 - np.abs(n[..., 1::-1])) * (np.where(n[..., :2] >= 0, 1.0, 0.0) * 2 - 1))


def _identity_motion(w, h, layers=1):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.repeat(np.stack([(xs + 0.5) / w, 1 - (ys + 0.5) / h], -1)[None], layers, 0).astype(np.float32)


def _wall(w, h, layers=1, normal=(0.0, 0.0, 1.0)):
    """A flat wall facing the camera: constant normal, z constant, x / y a pixel grid."""
    ys, xs = np.mgrid[0:h, 0:w]
    pos = np.stack([xs * 0.05, ys * 0.05, np.full_like(xs, 2.0, dtype=float), np.zeros_like(xs, dtype=float)], -1)[None].repeat(layers, 0)
    nrm = _oct_pack(np.broadcast_to(np.asarray(normal, float), (layers, h, w, 3)).copy())
    return pos, nrm


def _targets_from(diffuse_rgb, albedo_rgb, pos, nrm, motion, extra_spec=0.0, instance_id=None):
    one = np.ones(diffuse_rgb.shape[:-1] + (1,))
    color = np.concatenate([albedo_rgb * diffuse_rgb + extra_spec, one], -1)
    return dict(color=color, diffuse=np.concatenate([diffuse_rgb, one], -1), albedo=np.concatenate([albedo_rgb, one], -1), normal=nrm, pos=pos,
                screen_motion=motion, instance_id=instance_id)


def _linear_scene(rng, w, h, layers=1):
    """Noisy channels that are an exact linear function of the ten features (hence of every block's scaled features)."""
    n = rng.normal(size=(layers, h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    pos = np.concatenate([rng.uniform(-3, 3, (layers, h, w, 3)), np.zeros((layers, h, w, 1))], -1)
    nn = M.octahedral_unpack(_oct_pack(n), np.float64)
    feat = np.concatenate([np.ones((layers, h, w, 1)), nn, pos[..., :3], pos[..., :3] ** 2], -1)
    dif = feat @ rng.uniform(0, 1, (10, 3))
    dif -= dif.min() - 0.1
    alb = rng.uniform(0.2, 1, (layers, h, w, 3))
    return _targets_from(dif, alb, pos, _oct_pack(n), _identity_motion(w, h, layers), extra_spec=0.05)


def test_block_offsets_cover_the_block():
    o = M.block_offsets()
    assert o.shape == (16, 2) and (o >= -16).all() and (o < 16).all() and (o % 2 == 0).all()
    assert len({tuple(x) for x in o.tolist()}) == 16
    assert len(set(o[:, 0].tolist())) == 16 and len(set(o[:, 1].tolist())) >= 8        # every even column once, rows spread


def test_model_reproduces_an_input_in_the_span_of_the_features():
    t = _linear_scene(np.random.default_rng(0), 70, 50)
    m = M.BmfrModel((70, 50), 1, 0, noise_amount=0.0)
    out = m.run(t, 3)
    assert np.abs(out - t["color"]).max() < 1e-9
    m6 = M.BmfrModel((70, 50), 1, 1, noise_amount=0.0)        # DIFFUSE_SPECULAR: the specular part (a constant) is in the span too
    assert np.abs(m6.run(t, 5) - t["color"]).max() < 1e-9


def test_model_history_is_the_running_mean():
    rng = np.random.default_rng(1)
    w = h = 16
    pos, nrm = _wall(w, h)
    m = M.BmfrModel((w, h), 1, 0)
    total = np.zeros((1, h, w, 3))
    for f in range(260):
        dif = rng.uniform(0, 2, (1, h, w, 3))
        m.run(_targets_from(dif, np.full((1, h, w, 3), 0.5), pos, nrm, _identity_motion(w, h)), f)
        total += dif
        n = f + 1
        assert (m.noisy[0][..., 3] == min(n, 255)).all()
        if n <= 100:          # alpha = 1 / n down to the clamp at 0.01
            assert np.abs(m.noisy[0][..., :3] - total / n).max() < 1e-12
    assert (m.filtered[0][..., 3] == 255).all()


def test_model_rejects_taps_outside_and_across_a_normal_change():
    w = h = 32
    pos, nrm = _wall(w, h)
    dif = np.full((1, h, w, 3), 1.0)
    alb = np.full((1, h, w, 3), 0.5)
    m = M.BmfrModel((w, h), 1, 0)
    m.run(_targets_from(dif, alb, pos, nrm, _identity_motion(w, h)), 0)
    assert (m.last["accept_bits"] == 0).all()                    # frame 0: no history
    # the whole frame reprojects half a pixel left and up of where it was: every interior pixel keeps four taps, column 0 and row 0 lose those outside
    mo = _identity_motion(w, h)
    mo[..., 0] -= 0.5 / w
    mo[..., 1] += 0.5 / h
    m.run(_targets_from(dif, alb, pos, nrm, mo), 1)
    b = m.last["accept_bits"][0]
    assert (b[1:, 1:] == 15).all() and (b[1:, 0] == 0b1010).all() and (b[0, 1:] == 0b1100).all() and b[0, 0] == 0b1000
    # 90 degrees: no tap survives, the history starts over
    _, turned = _wall(w, h, normal=(1.0, 0.0, 0.0))
    m.run(_targets_from(dif, alb, pos, turned, _identity_motion(w, h)), 2)
    assert (m.last["accept_bits"] == 0).all() and (m.noisy[0][..., 3] == 1).all()
    # no surface (instance id < 0): passes through, keeps nothing, and is no tap for the next frame
    ids = np.zeros((1, h, w), np.int32)
    ids[0, 8:16] = -1
    t = _targets_from(dif, alb, pos, turned, _identity_motion(w, h), instance_id=ids)
    t["color"][0, 8:16, :, :3] = 7.0
    out = m.run(t, 3)
    assert (m.last["accept_bits"][0, 8:16] == 16).all() and (out[0, 8:16, :, :3] == 7.0).all()
    m.run(_targets_from(dif, alb, pos, turned, _identity_motion(w, h)), 4)
    assert (m.last["accept_bits"][0, 9:15] == 0).all()


def test_mirrored_block_grid_pixels_equal_their_sources():
    w, h = 40, 24
    m = M.BmfrModel((w, h), 1, 0)
    img = np.arange(h * w, dtype=float).reshape(1, h, w, 1)
    for frame in range(16):
        ox, oy = m.offsets[frame]
        rows = m.gather_rows(img, frame)
        assert rows.shape == (m.bw * m.bh, 1, 1024)
        grid = rows.reshape(m.bh, m.bw, 32, 32).transpose(0, 2, 1, 3).reshape(m.bh * 32, m.bw * 32)
        for gy in range(0, m.bh * 32, 7):
            for gx in range(0, m.bw * 32, 5):
                x, y = gx - 16 + ox, gy - 16 + oy
                sx = -x - 1 if x < 0 else (2 * w - x - 1 if x >= w else x)
                sy = -y - 1 if y < 0 else (2 * h - y - 1 if y >= h else y)
                assert grid[gy, gx] == img[0, min(max(sy, 0), h - 1), min(max(sx, 0), w - 1), 0]
        inside = grid[16 - oy:16 - oy + h, 16 - ox:16 - ox + w]
        assert (inside == img[0, ..., 0]).all()                  # every image pixel is in the grid exactly where the shift puts it


def test_model_float32_householder_solves_least_squares():
    rng = np.random.default_rng(3)
    A = np.concatenate([np.ones((1024, 1)), rng.normal(size=(1024, 9))], 1)
    B = A @ rng.normal(size=(10, 3)) + 0.1 * rng.normal(size=(1024, 3))
    w32, w64 = M.householder_f32(A, B), M.lstsq_weights(A, B)
    assert np.abs(w32 - w64).max() < 1e-4


# ======================================================================================================================
# CPU: the boundary
BMFR_SYMBOLS = ("trhip_bmfr_create", "trhip_bmfr_destroy", "trhip_bmfr_run", "trhip_bmfr_reset_history", "trhip_bmfr_get_timings",
                "trhip_bmfr_fit_blocks", "trhip_bmfr_download")


def test_bmfr_symbols_resolve():
    from tauray_amd import _lib
    L = _lib.lib()
    for n in BMFR_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.BmfrOptionsC) == 8 and C.sizeof(_lib.BmfrFeaturesC) == 7 * 8 and C.sizeof(_lib.BmfrTimingsC) == 24


def test_bmfr_create_refuses_bad_arguments_and_a_missing_device():
    from tauray_amd import _lib
    L = _lib.lib()
    out = C.c_void_p()

    def err(opt, w, h, layers, dev=None):
        rc = L.trhip_bmfr_create(dev, C.byref(opt) if opt is not None else None, w, h, layers, C.byref(out))
        assert rc != 0 and not out.value
        return L.trhip_last_error().decode()
    assert "settings" in err(_lib.BmfrOptionsC(2, 0.0), 64, 64, 1)
    assert "settings" in err(_lib.BmfrOptionsC(-1, 0.0), 64, 64, 1)
    assert "noise_amount" in err(_lib.BmfrOptionsC(0, -1.0), 64, 64, 1)
    assert "noise_amount" in err(_lib.BmfrOptionsC(0, float("nan")), 64, 64, 1)
    assert "zero" in err(_lib.BmfrOptionsC(0, 0.0), 0, 64, 1)
    assert "zero" in err(_lib.BmfrOptionsC(0, 0.0), 64, 64, 0)
    assert "options" in err(None, 64, 64, 1)
    assert "device" in err(_lib.BmfrOptionsC(0, 0.0), 64, 64, 1)           # good arguments, no device: no CPU fallback
    assert L.trhip_bmfr_run(None, None, 0, None) != 0 and L.trhip_bmfr_reset_history(None) != 0
    assert L.trhip_bmfr_fit_blocks(None, 1, 3, None, None, None) != 0


def test_renderer_refuses_what_the_denoiser_cannot_do():
    from tauray_amd import renderer as R
    import torch
    with pytest.raises(ValueError, match="gathered and stitched"):
        R.RtRenderer(None, None, None, (64, 64), world_size=2, rank=0, denoiser="bmfr")
    with pytest.raises(ValueError, match="svgf is not built"):
        R.RtRenderer(None, None, None, (64, 64), denoiser="svgf")
    with pytest.raises(ValueError, match="fresh frame"):
        R.RtRenderer(None, None, None, (64, 64), denoiser="bmfr", accumulate=True)
    if not torch.cuda.is_available():
        with pytest.raises(R.TrhipError):
            R.BmfrStage(type("NoDevice", (), {"h": None})(), (64, 64))
        with pytest.raises(R.TrhipError):
            R.RtRenderer(R.Context(0), None, None, (64, 64), denoiser="bmfr")


def test_cli_knows_the_denoiser_option():
    exe = os.path.join(ROOT, "tauray_amd", "tauray_hip")
    h = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--denoiser" in h.stdout + h.stderr and "bmfr" in h.stdout + h.stderr
    r = subprocess.run([exe, os.path.join(GOLDEN, "test.glb"), "--denoiser=svgf", "--headless=/dev/null"], capture_output=True, text=True)
    assert r.returncode != 0 and "svgf" in r.stderr and "not built" in r.stderr
    r = subprocess.run([exe, os.path.join(GOLDEN, "test.glb"), "--denoiser=nonsense", "--headless=/dev/null"], capture_output=True, text=True)
    assert r.returncode != 0 and "denoiser" in r.stderr


def test_threshold_pixels_stay_under_the_cap_on_oracle_targets(oracle, test_glb_128, oracle_scene_128):
    """The condition of the 0.5 % allowance, checked without a GPU: the float32 model against the float64 model on the targets the
    oracle renders of test.glb (which tests/test_gpu_parity.py holds the library's targets to), fixed camera, four frames."""
    names = list(FEATURE_NAMES)
    opt = oracle.options_for_scene(test_glb_128, max_bounces=3)
    m64, m32 = M.BmfrModel((128, 128)), M.BmfrModel((128, 128), dtype=np.float32)
    for f in range(4):
        t = oracle_scene_128.render_pt_targets(opt, 128, 128, names, frame_counter=f, samples_accumulated=0)
        t = dict(t, instance_id=t["instance_id"][..., 0])
        m64.run(t, f)
        o32 = m32.run(t, f)
        share = float((m32.last["own_accept_bits"] != m64.last["own_accept_bits"]).mean())
        assert share <= LEFT_OUT_CAP, f"frame {f}: {share:.3%} of the pixels decide their taps differently at float32"
        assert np.isfinite(o32).all()
        if f:
            assert (m64.last["accept_bits"] & 15).astype(bool).mean() > 0.5       # a fixed camera keeps most of its history


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


def _alloc_targets(R, ctx, size, layers):
    w, h = size
    return {n: ctx.alloc(layers * w * h * R.PathTracerStage.TARGETS[n][0] * 4).zero() for n in FEATURE_NAMES}


def _download_targets(R, bufs, size, layers):
    w, h = size
    out = {}
    for n, b in bufs.items():
        ch, dt = R.PathTracerStage.TARGETS[n]
        out[n] = b.download((layers, h, w, ch), dt)
    out["instance_id"] = out["instance_id"][..., 0]
    return out


def _upload_targets(ctx, t):
    bufs = {}
    for n in FEATURE_NAMES:
        if t.get(n) is None:
            continue
        a = np.ascontiguousarray(t[n], dtype=np.int32 if n == "instance_id" else np.float32)
        bufs[n] = ctx.alloc(a.nbytes).upload(a)
    return bufs


def _render_frame(R, pt, bufs, layers):
    pt.reset_accumulated_samples()
    pt.run_targets(bufs, layers)


def _glb(name, size):
    from tauray_amd.gltf import load_glb
    return load_glb(os.path.join(GOLDEN, name), size[0], size[1])


def _sponza(size, tris=30000):
    from tauray_amd import scenes
    return scenes.sponza_class(seed=1, target_tris=tris, width=size[0], height=size[1])


def _orbit(cam0, angle):
    import copy
    c = copy.deepcopy(cam0)
    ca, sa = np.cos(angle), np.sin(angle)
    rot = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1.0]])
    c.transform = rot @ np.asarray(cam0.transform, float)
    return c


# ---- 1. the fit
def _family_matrices(R, ctx, family):
    rng = np.random.default_rng(11)
    if family == "random":
        out = []
        for c in (3, 6):
            A = np.concatenate([np.ones((6, 1, 1024)), rng.normal(size=(6, 9, 1024))], 1)
            B = np.einsum("bfr,bfc->bcr", A, rng.normal(size=(6, 10, c))) + 0.3 * rng.normal(size=(6, c, 1024))
            out.append(np.concatenate([A, B], 1).astype(np.float32))
        return out
    if family == "scenes":
        out = []
        for scene, size in ((_glb("test.glb", (128, 128)), (128, 128)), (_sponza((128, 72)), (128, 72))):
            ss = R.SceneStage(ctx, scene)
            pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=3), _dup(size))
            bufs = _alloc_targets(R, ctx, size, 1)
            for settings in (0, 1):
                stage = R.BmfrStage(ctx, size, 1, settings)
                _render_frame(R, pt, bufs, 1)
                stage.run(bufs, 5)
                rows = stage.download("feature_rows")
                m, _ = M.prepare_blocks(rows, stage.block_grid[0], stage.block_grid[1], 5, 1e-2, np.float64)
                out.append(m.astype(np.float32))
                stage.close()
            pt.close()
        return out
    # degenerate blocks, through the model's own preparation (scaling + the 1e-2 noise)
    ys, xs = np.mgrid[0:32, 0:32]
    ones, zeros = np.ones(1024), np.zeros(1024)
    wall = np.stack([ones, zeros, zeros, ones, xs.ravel() * 0.03, ys.ravel() * 0.03, ones * 2.0, (xs.ravel() * 0.03) ** 2, (ys.ravel() * 0.03) ** 2, ones * 4.0])
    noisy = rng.uniform(0, 1, (3, 1024))
    one_colour = np.repeat(np.array([[0.3], [0.55], [0.7]]), 1024, 1)
    bright = rng.uniform(0, 0.1, (3, 1024))
    bright[:, [5, 333, 777]] = 500.0
    rows = np.stack([np.concatenate([wall, b]) for b in (noisy, one_colour, bright, np.zeros((3, 1024)))] + [np.zeros((13, 1024))])
    m, _ = M.prepare_blocks(rows, rows.shape[0], 1, 2, 1e-2, np.float64)
    return [m.astype(np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["random", "scenes", "degenerate"])
def test_fit_is_least_squares(R, ctx, family):
    """|A (w - w*)| <= c |b| per block and channel, c = 4 x the model's float32 Householder's largest figure of the family (see the module
    docstring).  Measured on one MI355X (profiles/r10/bmfr.txt; the test prints them), largest |A (w - w*)| / |b| of the model's float32
    Householder -> bound -> the kernels': random 6.4e-7 -> 2.6e-6 -> 2.0e-7; scene blocks (test.glb 128 x 128, sponza_class 128 x 72, both
    settings) 4.5e-6 -> 1.8e-5 -> 2.6e-6; degenerate (flat wall with noisy / one-colour / few-bright-pixels / all-zero channels, an all-
    "no surface" block) 1.1e-5 (the one-colour block) -> 4.3e-5 -> 5.8e-7."""
    rng = np.random.default_rng(5)
    perm = rng.permutation(1024)
    cases = []
    for mats in _family_matrices(R, ctx, family):
        got = R.fit_blocks(ctx, mats)
        assert np.isfinite(got).all(), "weights must be finite"
        for blk in range(mats.shape[0]):
            A, B = mats[blk, :10].T.astype(np.float64), mats[blk, 10:].T.astype(np.float64)
            wstar = M.lstsq_weights(A, B)
            w32 = M.householder_f32(mats[blk, :10].T, mats[blk, 10:].T)
            w32p = M.householder_f32(mats[blk, :10].T[perm], mats[blk, 10:].T[perm])
            for c in range(B.shape[1]):
                nb = np.linalg.norm(B[:, c])
                model = max(np.linalg.norm(A @ (w32[c].astype(np.float64) - wstar[c])), np.linalg.norm(A @ (w32p[c].astype(np.float64) - wstar[c])))
                gpu = np.linalg.norm(A @ (got[blk, c].astype(np.float64) - wstar[c]))
                cases.append((blk, c, nb, model, gpu))
    ratios = [m / nb for _, _, nb, m, _ in cases if nb > 0]
    c_model = max(ratios)
    bound = 4 * c_model
    worst = max(g / nb for _, _, nb, _, g in cases if nb > 0)
    print(f"\nBMFR fit [{family}]: {len(cases)} block-channels, model float32 max |A(w32-w*)|/|b| = {c_model:.3e}, bound = {bound:.3e}, GPU max = {worst:.3e}")
    for blk, c, nb, model, gpu in cases:
        if nb == 0:
            assert gpu == 0.0, f"block {blk} channel {c}: an all-zero right-hand side must give fitted values of exactly 0"
        else:
            assert gpu <= bound * nb, f"block {blk} channel {c}: |A(w-w*)|/|b| = {gpu / nb:.3e} > {bound:.3e}"


# ---- 2. the stage is the model
def _compare_sequence(R, ctx, label, size, layers, settings, frames, render, use_id=True):
    """Runs `frames` frames: render(f) fills and returns the device targets; stage and models consume the same downloaded values."""
    stage = R.BmfrStage(ctx, size, layers, settings)
    m64, m32 = M.BmfrModel(size, layers, settings), M.BmfrModel(size, layers, settings, dtype=np.float32)
    worst = {}
    for f in range(frames):
        bufs = render(f)
        t = _download_targets(R, bufs, size, layers)
        feats = dict(bufs)
        if not use_id:
            feats["instance_id"] = None
            t["instance_id"] = None
        stage.run(feats, f)
        got = dict(color=bufs["color"].download((layers, size[1], size[0], 4)), noisy_diffuse=stage.download("noisy_diffuse"),
                   noisy_specular=stage.download("noisy_specular"), filtered_diffuse=stage.download("filtered_diffuse"))
        if settings == 1:
            got["filtered_specular"] = stage.download("filtered_specular")
        bits = stage.download("accept_bits")
        o64 = m64.run(t, f, accept_bits=bits)
        o32 = m32.run(t, f, accept_bits=bits)
        assert np.array_equal(bits & 16, m64.last["accept_bits"] & 16), f"{label} frame {f}: no-surface bits"
        left_out = bits != m64.last["own_accept_bits"]
        share = float(left_out.mean())
        assert share <= LEFT_OUT_CAP, f"{label} frame {f}: {share:.3%} of the pixels keep other taps than the model"
        keep = ~left_out
        ref = dict(color=(o64, o32), noisy_diffuse=(m64.noisy[0], m32.noisy[0]), noisy_specular=(m64.noisy[1], m32.noisy[1]),
                   filtered_diffuse=(m64.filtered[0], m32.filtered[0]))
        if settings == 1:
            ref["filtered_specular"] = (m64.filtered[1], m32.filtered[1])
        for q, (r64, r32) in ref.items():
            g = got[q]
            assert np.isfinite(g).all(), f"{label} frame {f}: {q} is not finite"
            model_dev = float(np.abs(r32[keep][:, :3].astype(np.float64) - r64[keep][:, :3]).max())
            gpu_dev = float(np.abs(g[keep][:, :3].astype(np.float64) - r64[keep][:, :3]).max())
            w = worst.setdefault(q, [0.0, 0.0, 0.0])
            w[0], w[1] = max(w[0], model_dev), max(w[1], gpu_dev)
            w[2] = max(w[2], gpu_dev / model_dev if model_dev > 0 else (0.0 if gpu_dev == 0 else np.inf))
            assert gpu_dev <= 4 * model_dev, f"{label} frame {f}: {q} deviates {gpu_dev:.3e} from the float64 model, the float32 model {model_dev:.3e}"
        for q in ("noisy_diffuse", "filtered_diffuse"):
            hl = got[q][..., 3][keep]
            assert np.abs(hl - ref[q][0][..., 3][keep]).max() <= 1e-4 * 255, f"{label} frame {f}: history length of {q}"
        worst["left_out"] = max(worst.get("left_out", 0.0), share)
    print(f"\nBMFR stage [{label}] {size[0]}x{size[1]}x{layers} settings {settings}, {frames} frames: left out max {worst['left_out']:.4%}; "
          + "; ".join(f"{q}: model32 {v[0]:.2e} gpu {v[1]:.2e} (worst ratio {v[2]:.2f})" for q, v in worst.items() if q != "left_out"))
    stage.close()
    return worst


def _scene_renderer(R, ctx, scene, size, layers, cameras_of_frame=None, animate=None, **opt_kw):
    ss = R.SceneStage(ctx, scene)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, **opt_kw), _dup(size))
    bufs = _alloc_targets(R, ctx, size, layers)
    state = {"prev": None}

    def render(f):
        if animate is not None:
            animate(ss, f)
        elif cameras_of_frame is not None:
            cams = cameras_of_frame(f)
            prev = state["prev"] or cams
            ss.update_cameras(cams)
            ss.set_previous_cameras(prev)
            state["prev"] = cams
        _render_frame(R, pt, bufs, layers)
        ctx.sync()
        return bufs
    return render, pt, ss


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["glb128-fixed-20", "glb128-specular", "glb200x120-grid", "glb128-orbit", "animated", "envmap-id", "envmap-no-id"])
def test_stage_is_the_model(R, ctx, case):
    """The whole pipeline against tests/bmfr_model.py on the same downloaded targets; bounds as the module docstring says.  Measured
    (profiles/r10/bmfr.txt): no pixel left out in any sequence; largest deviations from the float64 model between 6e-8 and 9.4e-6 for the
    float32 model and the kernels alike, worst per-frame ratio kernels / float32 model 2.5 (filtered diffuse, animated clip) of the 4 allowed."""
    from tauray_amd import scene as S
    if case in ("glb128-fixed-20", "glb128-specular"):
        size, layers, settings, frames = (128, 128), 1, (0 if case == "glb128-fixed-20" else 1), (20 if case == "glb128-fixed-20" else 6)
        scene = _glb("test.glb", size)
        render, pt, _ = _scene_renderer(R, ctx, scene, size, layers, max_bounces=3)
    elif case == "glb200x120-grid":
        size, layers, settings, frames = (200, 120), 2, 0, 5
        scene = _glb("test.glb", size)
        scene.cameras = S.generate_camera_grid(scene.cameras[0], 2, 1, 0.3, 0.3, 5.0)
        render, pt, _ = _scene_renderer(R, ctx, scene, size, layers, max_bounces=3)
    elif case == "glb128-orbit":
        size, layers, settings, frames = (128, 128), 1, 0, 8
        scene = _glb("test.glb", size)
        cam0 = scene.cameras[0]
        render, pt, _ = _scene_renderer(R, ctx, scene, size, layers, cameras_of_frame=lambda f: [_orbit(cam0, 0.02 * f)], max_bounces=3)
    elif case == "animated":
        from tauray_amd.animation import SceneAnimator
        size, layers, settings, frames = (128, 96), 1, 0, 6
        scene = _glb("animated.glb", size)
        holder = {}

        def animate(ss, f):
            if "a" not in holder:
                holder["a"] = SceneAnimator(ss.scene)
                holder["a"].play("", loop=True)
            ss.animate(holder["a"], 0 if f == 0 else round(1000000.0 / 24.0))
        render, pt, _ = _scene_renderer(R, ctx, scene, size, layers, animate=animate, max_bounces=3)
    else:
        size, layers, settings, frames = (128, 72), 1, 0, 5
        scene = _sponza(size)
        render, pt, _ = _scene_renderer(R, ctx, scene, size, layers, max_bounces=3)
    _compare_sequence(R, ctx, case, size, layers, settings, frames, render, use_id=(case != "envmap-no-id"))
    pt.close()


# ---- 3. properties that need no model
def _run_frames(R, ctx, stage, frames_targets, stream=None, first_frame=0):
    """Uploads each frame's targets, runs the stage on them, returns the denoised colours (bit patterns)."""
    outs = []
    for i, t in enumerate(frames_targets):
        bufs = _upload_targets(ctx, t)
        stage.run(bufs, first_frame + i, stream)
        ctx.sync(stream)
        shape = np.asarray(t["color"]).shape
        outs.append(bufs["color"].download(shape))
    return outs


def _capture_frames(R, ctx, scene, size, frames, layers=1, **kw):
    render, pt, ss = _scene_renderer(R, ctx, scene, size, layers, max_bounces=3, **kw)
    out = [_download_targets(R, render(f), size, layers) for f in range(frames)]
    pt.close()
    return out


@pytest.mark.gpu
def test_exact_in_span_input_is_reproduced(R, ctx):
    """3(i): per pixel within (the one-colour block's bound of the fit test) x (the largest channel value).  The noise of the fit is
    switched off (amplitude 1e-30: a fit on features with noise does not reproduce a function of the features without it, which is
    what the noise is for)."""
    t = _linear_scene(np.random.default_rng(0), 96, 64)
    stage = R.BmfrStage(ctx, (96, 64), 1, 1, noise_amount=1e-30)
    out = _run_frames(R, ctx, stage, [t])[0]
    # the bound of the one-colour block, measured as in test_fit_is_least_squares
    mats = _family_matrices(R, ctx, "degenerate")[0]
    A, B = mats[1, :10].T, mats[1, 10:].T
    wstar = M.lstsq_weights(A, B)
    perm = np.random.default_rng(5).permutation(1024)
    c = 4 * max((np.linalg.norm(A.astype(np.float64) @ (w.astype(np.float64) - wstar).T, axis=0) / np.linalg.norm(B.astype(np.float64), axis=0)).max()
                for w in (M.householder_f32(A, B), M.householder_f32(A[perm], B[perm])))
    err = np.abs(out[..., :3].astype(np.float64) - t["color"][..., :3])
    scale = float(np.abs(t["diffuse"][..., :3]).max())
    print(f"\nBMFR exact-in-span: max error {err.max():.3e}, bound {c * scale:.3e} (c = {c:.3e}, largest channel {scale:.3f})")
    assert err.max() <= c * scale
    stage.close()


@pytest.mark.gpu
def test_runs_are_bit_reproducible_and_reset_history_starts_over(R, ctx):
    """3(ii), 3(iii)."""
    size = (128, 128)
    frames = _capture_frames(R, ctx, _glb("test.glb", size), size, 4)
    a = R.BmfrStage(ctx, size, 1, 0)
    first = _run_frames(R, ctx, a, frames)
    b = R.BmfrStage(ctx, size, 1, 0)
    st = ctx.create_stream()
    second = _run_frames(R, ctx, b, frames, stream=st)
    ctx.destroy_stream(st)
    for x, y in zip(first, second):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not np.array_equal(first[0], first[3])
    a.reset_history()
    again = _run_frames(R, ctx, a, frames[:1])[0]
    assert np.array_equal(again.view(np.uint32), first[0].view(np.uint32)), "after reset_history the next frame is a new stage's first frame"
    t = a.timings()
    assert t["frames"] == 5 and t["total_ms"] > 0 and all(t[k] > 0 for k in ("preprocess_ms", "fit_ms", "weighted_sum_ms", "accumulate_output_ms"))
    a.close()
    b.close()


@pytest.mark.gpu
def test_no_surface_passes_through_and_nothing_is_ever_non_finite(R, ctx):
    """3(iv), 3(v)."""
    size = (128, 72)
    frames = _capture_frames(R, ctx, _sponza(size), size, 3)
    sky = frames[0]["instance_id"] < 0
    assert 0.01 < sky.mean() < 0.9, "the scene must show some sky"
    stage = R.BmfrStage(ctx, size, 1, 0)
    outs = _run_frames(R, ctx, stage, frames)
    for t, o in zip(frames, outs):
        s = t["instance_id"] < 0
        assert np.array_equal(o[s].view(np.uint32), t["color"][s].view(np.uint32)), "a pixel without a surface keeps its input colour bit for bit"
        assert np.isfinite(o).all()
    # one NaN sample: the damage stays in its block (and what reprojects from it) and is gone after reset_history
    poisoned = [dict(t) for t in frames]
    sy, sx = np.argwhere(~sky[0])[len(np.argwhere(~sky[0])) // 2]
    for n in ("color", "diffuse"):
        poisoned[1][n] = poisoned[1][n].copy()
        poisoned[1][n][0, sy, sx, :3] = np.nan
    stage.reset_history()
    outs2 = _run_frames(R, ctx, stage, poisoned)
    for o in outs2:
        assert np.isfinite(o).all()
    for n in ("noisy_diffuse", "noisy_specular", "filtered_diffuse", "weights", "min_max"):
        assert np.isfinite(stage.download(n)).all(), n
    changed = np.argwhere((outs2[1] != outs[1]).any(-1)[0])
    assert len(changed) and (np.abs(changed - [sy, sx]).max(0) < 32).all(), "the NaN sample changes its own block only"
    stage.reset_history()
    clean = _run_frames(R, ctx, stage, frames[:1])[0]
    assert np.array_equal(clean.view(np.uint32), outs[0].view(np.uint32))
    stage.close()


def _rms(a, b, mask):
    d = (a[..., :3].astype(np.float64) - b[..., :3])[mask]
    return float(np.sqrt((d * d).mean()))


def _denoising_figures(R, ctx, scene, size, last, spp_ref=1024):
    ss = R.SceneStage(ctx, scene)
    opt = R.options_for_scene(scene, max_bounces=3)
    w, h = size
    ref_pt = R.PathTracerStage(ctx, ss, opt, _dup(size))
    ref_buf = ctx.alloc(w * h * 16).zero()
    for _ in range(spp_ref):
        ref_pt.run(ref_buf)
    ref = ref_buf.download((1, h, w, 4))
    ref_pt.close()
    pt = R.PathTracerStage(ctx, ss, opt, _dup(size))
    bufs = _alloc_targets(R, ctx, size, 1)
    stage = R.BmfrStage(ctx, size, 1, 0)
    fig = {}
    for f in range(last + 1):
        _render_frame(R, pt, bufs, 1)
        noisy = bufs["color"].download((1, h, w, 4))
        surf = bufs["instance_id"].download((1, h, w, 1), np.int32)[..., 0] >= 0
        stage.run(bufs, f)
        den = bufs["color"].download((1, h, w, 4))
        assert np.isfinite(den).all()
        if f in (0, last):
            ok = surf & np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1)       # the path tracer's rare NaN sample
            fig[f] = (_rms(noisy, ref, ok), _rms(den, ref, ok))
    timings = stage.timings()
    stage.close()
    pt.close()
    return fig, timings


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["test.glb", "sponza_class"])
def test_it_denoises(R, ctx, which):
    """3(vi): RMS error against the same view at 1 024 spp; at frame 16 of a fixed camera the denoised frame beats its noisy input and the
    denoised frame 0.  The ratios are printed (profiles/r10/bmfr.txt), not asserted."""
    size = (128, 128) if which == "test.glb" else (160, 90)
    scene = _glb("test.glb", size) if which == "test.glb" else _sponza(size)
    fig, _ = _denoising_figures(R, ctx, scene, size, 16)
    (n0, d0), (n16, d16) = fig[0], fig[16]
    print(f"\nBMFR denoising [{which}] RMS vs 1024 spp: frame 0 noisy {n0:.4f} denoised {d0:.4f} (ratio {d0 / n0:.3f}); "
          f"frame 16 noisy {n16:.4f} denoised {d16:.4f} (ratio {d16 / n16:.3f}; vs denoised frame 0 {d16 / d0:.3f})")
    assert d16 < n16 and d16 < d0


# ---- 4. hosts
@pytest.mark.gpu
def test_renderer_with_denoiser_equals_the_stages_driven_by_hand(R, ctx):
    size = (128, 128)
    w, h = size
    scene = _glb("test.glb", size)
    opt = R.options_for_scene(scene, max_bounces=3)
    r = R.RtRenderer(ctx, scene, opt, size, denoiser="bmfr")
    assert not r.fused_tonemap and r.post.bmfr is not None
    frames = []
    for _ in range(4):
        r.render()
        frames.append(r.download("display").copy())
    r.close()
    ss = R.SceneStage(ctx, scene)
    pt = R.PathTracerStage(ctx, ss, opt, _dup(size))
    bufs = _alloc_targets(R, ctx, size, 1)
    stage, tm = R.BmfrStage(ctx, size, 1, 0), R.TonemapStage(ctx)
    display = ctx.alloc(w * h * 16)
    for f in range(4):
        ss.set_previous_camera_data(ss.camera_data)
        _render_frame(R, pt, bufs, 1)
        stage.run(bufs, f)
        tm.run(bufs["color"], display, w, h, 1)
        assert np.array_equal(display.download((1, h, w, 4)).view(np.uint32), frames[f].view(np.uint32)), f"frame {f}"
    assert not np.array_equal(frames[0], frames[3])
    stage.close()
    pt.close()
    # frames in flight: the same frames (the denoiser's history is one chain on the default stream)
    r2 = R.RtRenderer(ctx, scene, opt, size, denoiser="bmfr", frames_in_flight=2)
    for f in range(4):
        r2.render()
        assert np.array_equal(r2.download("display").view(np.uint32), frames[f].view(np.uint32)), f"two slots, frame {f}"
    r2.close()


@pytest.mark.gpu
def test_cli_denoises_the_animated_clip_like_the_python_host(R, ctx, tmp_path):
    """`tauray_hip animated.glb --denoiser=bmfr --animation --headless=...`, three frames, against RtRenderer(denoiser="bmfr") playing the
    same file: the criterion of tests/test_cpp_host.py's animated comparison (the two animators differ in the last bits of a matrix)."""
    from tauray_amd.animation import SceneAnimator
    W, H = 160, 120
    glb = os.path.join(GOLDEN, "animated.glb")
    prefix = str(tmp_path / "dn")
    exe = os.path.join(ROOT, "tauray_amd", "tauray_hip")
    subprocess.check_call([exe, glb, f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--filetype=raw", "--animation", "--framerate=24", "--frames=3",
                           "--denoiser=bmfr", f"--headless={prefix}"])
    plain = str(tmp_path / "plain")
    subprocess.check_call([exe, glb, f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--filetype=raw", "--animation", "--framerate=24", "--frames=3",
                           f"--headless={plain}"])
    scene = _glb("animated.glb", (W, H))
    r = R.RtRenderer(ctx, scene, R.options_for_scene(scene, max_bounces=3), (W, H), denoiser="bmfr")
    an = SceneAnimator(scene)
    an.play("")
    for frame in range(3):
        r.scene_update.animate(an, 0 if frame == 0 else round(1000000.0 / 24.0), refit=(frame % 3 != 2))
        r.render()
        ref = r.download("display")[0]
        got = np.fromfile(f"{prefix}{frame}.raw", dtype=np.float32).reshape(H, W, 4)
        differing = float((np.abs(got - ref).max(-1) > 1e-3).mean())
        assert differing < 2e-3 and abs(float(got.mean()) - float(ref.mean())) < 1e-4, f"frame {frame}: {differing:.4%} of the pixels differ"
        noisy = np.fromfile(f"{plain}{frame}.raw", dtype=np.float32).reshape(H, W, 4)
        assert float((np.abs(got - noisy).max(-1) > 1e-3).mean()) > 0.2, "the denoiser did not run"
    r.close()


# ---- 5. full size
@pytest.mark.gpu
def test_full_size_sequence(R, ctx):
    size = (1920, 1080)
    scene = _sponza(size, tris=260_000)
    fig, t = _denoising_figures(R, ctx, scene, size, 4)
    (n0, d0), (n4, d4) = fig[0], fig[4]
    print(f"\nBMFR 1920x1080 sponza_class: RMS vs 1024 spp frame 0 noisy {n0:.4f} denoised {d0:.4f}; frame 4 noisy {n4:.4f} denoised {d4:.4f}; timings {t}")
    assert d4 < n4 and d4 < d0
    assert t["frames"] == 5 and t["total_ms"] > 0
