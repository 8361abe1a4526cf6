"""A numpy model of the temporal antialiasing stage (csrc/taa.hip; include/trhip.h), written from the description of
the algorithm, with a dtype switch: float64 is the reference the tests compare against; float32 evaluates every expression in the order
csrc/taa.h pins (which is the order the kernel uses) and measures what float32 rounding does to it.  A second float32 variant
(pow="power") takes the colour map's powers with numpy.power instead of exp2(gamma * log2(c)): another equally valid float32 evaluation.

Per output pixel p of a layer (camera pair cur / prev, both packed camera_data records):
  1. col = src[p]; m = map(col.rgb): c <= 0 ? 0 : c^gamma; under anti_shimmer then c > 1e-5 ? log(c) : -10
  2. lo / hi [11]: min / max over the 3 x 3 window (clamped to the edge) of dot(m, axis) -/+ 1e-5
  3. edge dilation: offset of the window pixel with the smallest depth dot(pos - origin, forward) under a strict <, x outer, y inner,
     starting from (+inf, offset 0); pixels outside the image or with instance_id < 0 have depth +inf.  The depth is defined as the float32
     value of that expression (three differences, three products, two sums from the left), like the float32 content of the reference's
     depth target: on a wall that faces the camera the depths of a window differ by rounding only, and a comparison at another precision
     would pick other neighbours
  4. motion = screen_motion[p + offset]; where that pixel has no surface (instance_id < 0; without ids: a NaN motion) and the camera is
     perspective: prev.view_proj * (primary ray direction through the centre of p, 0) -> xy / w * 0.5 + 0.5
  5. motion += (prev.pan.zw - cur.pan.zw) * 0.5; uv = (motion.x, 1 - motion.y) - offset / size; outside [0, 1 + 2 / size] (or NaN):
     out = col
  6. prev colour = the bicubic filter of the history at uv (twelve clamped texels), max(., 0)
  7. delta = map(prev) - m; t = k-DOP intersection from m along delta (fmin / fmax drop a NaN axis); clipped = m + clamp(t, 0, 1) * delta;
     out.rgb = unmap(mix(clipped, m, alpha)); out.a = col.a
The decision byte: bits 0-3 (ox + 1) * 3 + (oy + 1), bit 4 outside, bit 5 no surface.
"""
import numpy as np

DILATION = 1e-5
OUTSIDE, NO_SURFACE = 16, 32
# the 22-DOP of shader/taa.comp:46-56, as the float32 values the kernel holds
AXES = np.array([
    [1.000000, 0.000000, 0.000000], [-0.098489, 0.184576, -0.977871], [0.752374, -0.312087, 0.580116], [-0.098489, -0.969577, -0.224098],
    [0.330653, 0.717910, -0.612596], [0.752374, 0.656636, -0.052553], [0.591354, 0.440953, 0.675174], [0.698983, -0.670755, -0.248014],
    [0.176950, -0.538181, -0.824045], [-0.698983, -0.042551, 0.713871], [0.330652, -0.849517, 0.411084]], np.float32)


def _pow(c, g, dt, pow_mode):
    """c <= 0 ? 0 : c^g, per element."""
    pos = c > 0
    safe = np.where(pos, c, dt(1))
    with np.errstate(all="ignore"):
        r = np.power(safe, dt(g)) if pow_mode == "power" else np.exp2(dt(g) * np.log2(safe))
    return np.where(pos, r, dt(0)).astype(dt)


def map_color(c, gamma, anti_shimmer, dt=np.float64, pow_mode="exp2"):
    c = np.asarray(c).astype(dt)
    r = _pow(c, dt(np.float32(gamma)), dt, pow_mode)
    if anti_shimmer:
        big = r > dt(np.float32(1e-5))
        r = np.where(big, np.log(np.where(big, r, dt(1))), dt(-10)).astype(dt)
    return r


def unmap_color(c, gamma, anti_shimmer, dt=np.float64, pow_mode="exp2"):
    c = np.asarray(c).astype(dt)
    if anti_shimmer:
        c = np.exp(c).astype(dt)
    inv_gamma = dt(1) / dt(np.float32(gamma))
    return _pow(c, inv_gamma, dt, pow_mode)


def _dot3(v, axis, dt):
    a = axis.astype(dt)
    return v[..., 0] * a[0] + v[..., 1] * a[1] + v[..., 2] * a[2]


def _mat(rec, name, dt):
    """A matrix of a camera_data record as [column][row]."""
    return np.asarray(rec[name]).reshape(4, 4).astype(dt)


def _mul(m, x, y, z, w):
    """M * (x, y, z, w): col0 * x + col1 * y + col2 * z + col3 * w from the left; returns the four rows."""
    return [m[0][r] * x + m[1][r] * y + m[2][r] * z + m[3][r] * w for r in range(4)]


def _mix(a, b, t, dt):
    return a * (dt(1) - t) + b * t


def window_ranges(m, dt):
    """lo, hi [11][h][w] of the mapped image m [h][w][3]."""
    pad = np.pad(m, ((1, 1), (1, 1), (0, 0)), mode="edge")
    h, w = m.shape[:2]
    lo = np.empty((len(AXES), h, w), dt)
    hi = np.empty((len(AXES), h, w), dt)
    for a, axis in enumerate(AXES):
        r = _dot3(pad, axis, dt)
        rl, rh = r - dt(DILATION), r + dt(DILATION)
        l = h_ = None
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                sl = (slice(1 + dy, 1 + dy + h), slice(1 + dx, 1 + dx + w))
                l = rl[sl] if l is None else np.fmin(rl[sl], l)
                h_ = rh[sl] if h_ is None else np.fmax(rh[sl], h_)
        lo[a], hi[a] = l, h_
    return lo, hi


def closest_offsets(pos, ids, cur, dt=None):
    """ox, oy [h][w]: the edge dilation's choice.  The depth is a float32 quantity with a pinned formula (csrc/taa.h), as the reference's is
    the float32 content of a depth target: every model variant compares the same float32 depths, whatever it evaluates colours at."""
    dt = np.float32
    h, w = pos.shape[:2]
    o = np.asarray(cur["origin"]).reshape(4).astype(dt)
    vi = _mat(cur, "view_inverse", dt)
    fwd = [-vi[2][0], -vi[2][1], -vi[2][2]]
    p = pos.astype(dt)
    with np.errstate(all="ignore"):
        depth = (p[..., 0] - o[0]) * fwd[0] + (p[..., 1] - o[1]) * fwd[1] + (p[..., 2] - o[2]) * fwd[2]
    if ids is not None:
        depth = np.where(ids < 0, dt(np.inf), depth)
    pad = np.pad(depth, 1, mode="constant", constant_values=np.inf)
    best = np.full((h, w), np.inf, dt)
    ox = np.zeros((h, w), np.int64)
    oy = np.zeros((h, w), np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            d = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            take = d < best
            best = np.where(take, d, best)
            ox = np.where(take, dx, ox)
            oy = np.where(take, dy, oy)
    return ox, oy


def miss_motion(w, h, cur, prev, dt):
    """The previous camera's projection of the primary ray directions through the pixel centres (perspective), [h][w][2]."""
    ys, xs = np.mgrid[0:h, 0:w]
    u = ((xs.astype(dt) + dt(0.5)) / dt(w)) * dt(2) - dt(1)
    v = ((dt(h) - (ys.astype(dt) + dt(0.5))) / dt(h)) * dt(2) - dt(1)
    one = np.ones_like(u)
    t = _mul(_mat(cur, "proj_inverse", dt), u, v, one, one)
    d = _mul(_mat(cur, "view_inverse", dt), t[0], t[1], t[2], dt(0))
    length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    d = [d[0] / length, d[1] / length, d[2] / length]
    c = _mul(_mat(prev, "view_proj", dt), d[0], d[1], d[2], dt(0))
    with np.errstate(all="ignore"):
        return np.stack([(c[0] / c[3]) * dt(0.5) + dt(0.5), (c[1] / c[3]) * dt(0.5) + dt(0.5)], -1)


def reprojected_uv(motion, pos, ids, cur, prev, edge_dilation, perspective, dt=np.float64):
    """Steps 3-5 for one layer: uv [h][w][2] (x right, y down, in [0, 1] over the image), ox, oy, no-surface mask."""
    h, w = motion.shape[:2]
    if edge_dilation:
        ox, oy = closest_offsets(pos, ids, cur, dt)
    else:
        ox = np.zeros((h, w), np.int64)
        oy = np.zeros((h, w), np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    qy, qx = ys + oy, xs + ox
    mo = motion[qy, qx].astype(dt)
    nosurf = (ids[qy, qx] < 0) if ids is not None else np.isnan(motion[qy, qx]).any(-1)
    if perspective and nosurf.any():
        mo = np.where(nosurf[..., None], miss_motion(w, h, cur, prev, dt), mo)
    pc = np.asarray(cur["pan"]).reshape(4).astype(dt)
    pp = np.asarray(prev["pan"]).reshape(4).astype(dt)
    mx = mo[..., 0] + (pp[2] - pc[2]) * dt(0.5)
    my = mo[..., 1] + (pp[3] - pc[3]) * dt(0.5)
    psx, psy = dt(1) / dt(w), dt(1) / dt(h)
    uvx = mx - ox.astype(dt) * psx
    uvy = (dt(1) - my) - oy.astype(dt) * psy
    return np.stack([uvx, uvy], -1), ox, oy, nosurf


def bicubic(hist, uvx, uvy, dt):
    """The reference's Catmull-Rom filter of hist [h][w][3+] at uv (arrays of N positions), as twelve clamped texels -> [N][3]."""
    h, w = hist.shape[:2]
    hist = hist[..., :3].astype(dt)
    posx, posy = uvx * dt(w), uvy * dt(h)
    cxf, cyf = np.floor(posx - dt(0.5)), np.floor(posy - dt(0.5))
    fx, fy = posx - (cxf + dt(0.5)), posy - (cyf + dt(0.5))
    cx, cy = cxf.astype(np.int64), cyf.astype(np.int64)

    def weights(f):
        f2 = f * f
        f3 = f * f2
        w0 = (dt(-0.5) * f3 + f2) - dt(0.5) * f
        w1 = (dt(1.5) * f3 - dt(2.5) * f2) + dt(1)
        w2 = (dt(-1.5) * f3 + dt(2) * f2) + dt(0.5) * f
        w3 = dt(0.5) * f3 - dt(0.5) * f2
        return w0, w1 + w2, w2 / (w1 + w2), w3
    w0x, w12x, qx, w3x = weights(fx)
    w0y, w12y, qy, w3y = weights(fy)

    def T(i, j):
        return hist[np.clip(cy + j, 0, h - 1), np.clip(cx + i, 0, w - 1)]
    qx3, qy3 = qx[:, None], qy[:, None]
    A = _mix(T(0, -1), T(1, -1), qx3, dt)
    B = _mix(T(-1, 0), T(-1, 1), qy3, dt)
    Cc = _mix(_mix(T(0, 0), T(1, 0), qx3, dt), _mix(T(0, 1), T(1, 1), qx3, dt), qy3, dt)
    D = _mix(T(2, 0), T(2, 1), qy3, dt)
    E = _mix(T(0, 2), T(1, 2), qx3, dt)
    wa, wb, wc, wd, we = w12x * w0y, w0x * w12y, w12x * w12y, w3x * w12y, w12x * w3y
    total = (((wa + wb) + wc) + wd) + we
    s = (((A * wa[:, None] + B * wb[:, None]) + Cc * wc[:, None]) + D * wd[:, None]) + E * we[:, None]
    return np.maximum(s / total[:, None], dt(0))


def kdop_clip(m, mp, lo, hi, dt):
    """m, mp [N][3], lo, hi [11][N]: map(prev) clipped towards m; returns (clipped [N][3], len [N])."""
    delta = mp - m
    near = np.full(m.shape[0], -1e9, dt)
    far = np.full(m.shape[0], 1e9, dt)
    with np.errstate(all="ignore"):
        for a, axis in enumerate(AXES):
            inv = dt(1) / _dot3(delta, axis, dt)
            pp = _dot3(m, axis, dt)
            t0, t1 = (lo[a] - pp) * inv, (hi[a] - pp) * inv
            near = np.fmax(near, np.fmin(t0, t1))
            far = np.fmin(far, np.fmax(t0, t1))
    t = np.where((near <= far) & ((near > 0) | (far > 0)), np.where(near > 0, near, far), dt(-1))
    length = np.minimum(np.maximum(t, dt(0)), dt(1))
    return m + length[:, None] * delta, length


def run_layer(src, history, motion, pos, ids, cur, prev, alpha, gamma, edge_dilation=True, anti_shimmer=False, perspective=True,
              dtype=np.float64, pow_mode="exp2"):
    """One layer of one frame.  src, history [h][w][4]; motion [h][w][2]; pos [h][w][4] (edge dilation); ids [h][w] or None; cur / prev:
    camera_data records.  Returns (out [h][w][4] of dtype - dst and the new history -, decisions uint8 [h][w])."""
    dt = dtype
    h, w = src.shape[:2]
    alpha = dt(np.float32(alpha))
    m = map_color(src[..., :3], gamma, anti_shimmer, dt, pow_mode)
    lo, hi = window_ranges(m, dt)
    uv, ox, oy, nosurf = reprojected_uv(motion, pos, ids, cur, prev, edge_dilation, perspective, dt)
    uvx, uvy = uv[..., 0], uv[..., 1]
    psx, psy = dt(1) / dt(w), dt(1) / dt(h)
    with np.errstate(all="ignore"):
        outside = ~(uvx >= 0) | ~(uvy >= 0) | (uvx > dt(1) + dt(2) * psx) | (uvy > dt(1) + dt(2) * psy)
    decisions = ((ox + 1) * 3 + (oy + 1)).astype(np.uint8) | np.where(nosurf, NO_SURFACE, 0).astype(np.uint8) | np.where(outside, OUTSIDE, 0).astype(np.uint8)
    out = src.astype(dt).copy()
    inside = ~outside
    if inside.any():
        prev_col = bicubic(history, uvx[inside], uvy[inside], dt)
        mi = m[inside]
        clipped, _ = kdop_clip(mi, map_color(prev_col, gamma, anti_shimmer, dt, pow_mode), lo[:, inside], hi[:, inside], dt)
        mixed = _mix(clipped, mi, alpha, dt)
        rgb = unmap_color(mixed, gamma, anti_shimmer, dt, pow_mode)
        o = out[inside]
        o[:, :3] = rgb
        out[inside] = o
    return out, decisions


class TaaModel:
    """The stage: a history per layer, alpha = 1 while there is none."""

    def __init__(self, size, layers=1, alpha=0.125, gamma=2.2, edge_dilation=True, anti_shimmer=False, perspective=True, base_camera_index=0,
                 dtype=np.float64, pow_mode="exp2"):
        self.size, self.layers = (int(size[0]), int(size[1])), int(layers)
        self.alpha, self.gamma, self.edge_dilation, self.anti_shimmer, self.perspective = alpha, gamma, edge_dilation, anti_shimmer, perspective
        self.base, self.dtype, self.pow_mode = base_camera_index, dtype, pow_mode
        self.history = None
        self.decisions = None

    def reset_history(self):
        self.history = None

    def run(self, src, motion, pos, ids, cameras, prev_cameras, history=None, have_history=None):
        """src [L][h][w][4], motion [L][h][w][2], pos [L][h][w][4] or None, ids [L][h][w] or None; cameras / prev_cameras: camera_data arrays.
        `history`: the history to read instead of the model's own (the stage's, downloaded), with `have_history`."""
        w, h = self.size
        hist = self.history if history is None else history
        have = (self.history is not None) if have_history is None else have_history
        if hist is None:
            hist = np.zeros((self.layers, h, w, 4), np.float32)
        out = np.empty((self.layers, h, w, 4), self.dtype)
        dec = np.empty((self.layers, h, w), np.uint8)
        for z in range(self.layers):
            out[z], dec[z] = run_layer(src[z], hist[z], motion[z], None if pos is None else pos[z], None if ids is None else ids[z],
                                       cameras[self.base + z], prev_cameras[self.base + z], self.alpha if have else 1.0, self.gamma,
                                       self.edge_dilation, self.anti_shimmer, self.perspective, self.dtype, self.pow_mode)
        self.history, self.decisions = out, dec
        return out
