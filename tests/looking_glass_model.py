"""numpy model of the Looking Glass composition stage (trhip_lkg_*, tauray_amd/csrc/looking_glass.hip), written from the rule of
include/trhip.h at float64; with dtype=np.float32 it repeats the pinned order of operations of tauray_amd/csrc/looking_glass.h - every
product, sum and quotient rounded on its own - and is then the stage bit for bit.

Per output pixel p: calibration = (pitch, tilt * pitch, pitch / (3 * out_w), -center), negated under invert; uv = (p + 0.5) / out_size;
uvf = (uv.x, 1 - uv.y); per channel c: d = ((uvf.x * cal.x + uvf.y * cal.y) + c * cal.z) + cal.w, view = clamp(int(floor(fract(d) * N)),
0, N - 1); out[c] = channel c of that view, bilinear with clamp to edge at the unflipped uv; alpha = 1."""
import numpy as np


def calibration_vector(pitch, tilt, center, invert, out_w, dtype=np.float64):
    """The host's calibration vector from the stage's float32 options."""
    t = dtype
    pitch, tilt, center = (t(np.float32(v)) for v in (pitch, tilt, center))
    cal = np.array([pitch, tilt * pitch, pitch / (t(3.0) * t(out_w)), -center], dtype=t)
    return -cal if invert else cal


def _uv(out_size, dtype):
    W, H = out_size
    t = dtype
    uvx = (np.arange(W, dtype=t) + t(0.5)) / t(W)
    uvy = (np.arange(H, dtype=t) + t(0.5)) / t(H)
    return uvx, uvy


def view_indices(out_size, viewports, pitch, tilt, center, invert, dtype=np.float64):
    """uint8 [H][W][4]: the view of r, g, b; 0."""
    W, H = out_size
    t = dtype
    cal = calibration_vector(pitch, tilt, center, invert, W, t)
    uvx, uvy = _uv(out_size, t)
    uvfy = t(1.0) - uvy
    base = (uvx * cal[0])[None, :] + (uvfy * cal[1])[:, None]
    out = np.zeros((H, W, 4), np.uint8)
    for c in range(3):
        d = (base + t(c) * cal[2]) + cal[3]
        hh = d - np.floor(d)
        out[..., c] = np.clip(np.floor(hh * t(viewports)).astype(np.int64), 0, viewports - 1)
    return out


def bilinear_taps(out_size, view_size, dtype):
    """(x0, x1, wx) per output column and (y0, y1, wy) per output row."""
    t = dtype
    res = []
    for uv, n in zip(_uv(out_size, t), view_size):
        p = uv * t(n) - t(0.5)
        f = np.floor(p)
        w = p - f
        i = f.astype(np.int64)
        res.append((np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), w))
    return res


def compose(views, out_size, viewports, pitch, tilt, center, invert, dtype=np.float64):
    """views: [N][h][w][4].  Returns (out [H][W][4] of dtype, indices uint8 [H][W][4])."""
    t = dtype
    views = np.asarray(views)
    assert views.shape[0] == viewports
    h, w = views.shape[1:3]
    W, H = out_size
    idx = view_indices(out_size, viewports, pitch, tilt, center, invert, t)
    (x0, x1, wx), (y0, y1, wy) = bilinear_taps(out_size, (w, h), t)
    wx, wy = wx[None, :], wy[:, None]
    out = np.ones((H, W, 4), t)
    one = t(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            v = idx[..., c].astype(np.int64)
            ch = views[..., c].astype(t)
            t00 = ch[v, y0[:, None], x0[None, :]]
            t10 = ch[v, y0[:, None], x1[None, :]]
            t01 = ch[v, y1[:, None], x0[None, :]]
            t11 = ch[v, y1[:, None], x1[None, :]]
            top = t00 * (one - wx) + t10 * wx
            bottom = t01 * (one - wx) + t11 * wx
            out[..., c] = top * (one - wy) + bottom * wy
    return out, idx


def quantise(dst):
    """dst_rgba8 of a float32 dst: uint8(clamp(c, 0, 1) * 255 + 0.5) per channel (a NaN gives 0), 255 for alpha."""
    c = np.asarray(dst, np.float32)[..., :3]
    with np.errstate(invalid="ignore"):
        cc = np.where(c > 0, np.where(c < 1, c, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    q = (cc * np.float32(255.0) + np.float32(0.5)).astype(np.float32)
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = q.astype(np.uint8)
    return out


def resample(view, out_size, dtype=np.float64):
    """One view resampled bilinearly with clamp to edge to out_size (what the stage does with one view)."""
    t = dtype
    h, w = view.shape[:2]
    (x0, x1, wx), (y0, y1, wy) = bilinear_taps(out_size, (w, h), t)
    wx, wy = wx[None, :, None], wy[:, None, None]
    v = view.astype(t)
    top = v[y0[:, None], x0[None, :]] * (1 - wx) + v[y0[:, None], x1[None, :]] * wx
    bottom = v[y1[:, None], x0[None, :]] * (1 - wx) + v[y1[:, None], x1[None, :]] * wx
    return top * (1 - wy) + bottom * wy
