"""A numpy model of the spatial and temporal reprojection stages (csrc/reprojection.hip; include/trhip.h), written
from the description of the algorithm, with a dtype switch: float64 is the reference the tests compare against, float32 evaluates every
expression in the order the description gives (which is the order the kernels use) and measures what float32 rounding does to it.

Per output pixel of the spatial stage:
  source viewport          its colour
  destination, surface     project pos with every source's view_proj; candidate = smallest z/w below 1 (w > 0; ties: the first); a try of
                           source s: taps at floor(uv * size - 0.5), uv = (xy/w * 0.5 + 0.5, y -> 1 - y); a tap is kept when inside, a
                           surface, dot(n_tap, n) > 0.99 and |pos - pos_tap|^2 < 0.01; weights bilinear, renormalised over the kept taps;
                           success when the kept weight exceeds 1e-5.  Candidate first; if it fails the others in order, each only if its
                           depth is below the best accepted so far (1 while none is).  Nothing accepted: default_value.
  destination, no surface  the same pixel of the first source without a surface there, else default_value
"no surface": a NaN pos or instance_id < 0.  The temporal stage uses the same taps at screen_motion in its own history.

A model can be told the decisions (kind, slot, keep bits, tap origin) instead of making them: `decisions=` of run().  The value under given
decisions has no thresholds left in it, so float32 and float64 evaluations of it differ by rounding only.
"""
import numpy as np

NONE, REPROJECTED, SKY_COPY = 0, 1, 2
NORMAL_COS, DISTANCE_SQ, MIN_WEIGHT = 0.99, 0.01, 1e-5
CANONICAL_WEIGHT = 1e-3
TIE_FRACTION = 2.0 ** -24      # see _taps
RECORD = np.dtype([("kind", "u1"), ("slot", "u1"), ("bits", "u1"), ("zero", "u1"), ("ox", "<i2"), ("oy", "<i2")])


def octahedral_pack(n):
    n = np.asarray(n, np.float64)
    n = n / np.abs(n).sum(-1, keepdims=True)
    return np.where(n[..., 2:3] >= 0, n[..., :2], (1 - np.abs(n[..., 1::-1])) * (np.where(n[..., :2] >= 0, 1.0, 0.0) * 2 - 1))


def octahedral_unpack(o, dt):
    o = np.asarray(o).astype(dt)
    one = dt(1)
    x, y = o[..., 0], o[..., 1]
    z = one - np.abs(x) - np.abs(y)
    t = np.minimum(np.maximum(z, dt(-1)), dt(0))
    x = x + t * (np.where(x >= 0, one, dt(0)) * dt(2) - one)
    y = y + t * (np.where(y >= 0, one, dt(0)) * dt(2) - one)
    length = np.sqrt(x * x + y * y + z * z)
    return np.stack([x / length, y / length, z / length], -1)


def no_surface(pos, instance_id):
    ns = np.isnan(np.asarray(pos)[..., :3]).any(-1)
    if instance_id is not None:
        ns = ns | (np.asarray(instance_id) < 0)
    return ns


def project(view_proj, p, dt):
    """view_proj: [4 columns][4 rows] (the layout of CAMERA_DATA); p: [N, 3].  Returns w, z / w and uv = xy / w * 0.5 + 0.5."""
    m = np.asarray(view_proj).astype(dt)
    c = m[0][None] * p[:, 0:1] + m[1][None] * p[:, 1:2] + m[2][None] * p[:, 2:3] + m[3][None]
    with np.errstate(all="ignore"):
        depth = c[:, 2] / c[:, 3]
        u = (c[:, 0] / c[:, 3]) * dt(0.5) + dt(0.5)
        v = (c[:, 1] / c[:, 3]) * dt(0.5) + dt(0.5)
    return c[:, 3], depth, u, v


def tap_position(u, v, w, h, dt):
    """The continuous tap position: y -> 1 - y, * size, - 0.5, clamped to [-2, size + 1]."""
    with np.errstate(all="ignore"):
        fx = u * dt(w) - dt(0.5)
        fy = (dt(1) - v) * dt(h) - dt(0.5)
    # the kernels' min / max: a NaN position becomes -2 (outside)
    fx = np.where(np.isnan(fx), dt(-2), np.minimum(np.maximum(fx, dt(-2)), dt(w + 1)))
    fy = np.where(np.isnan(fy), dt(-2), np.minimum(np.maximum(fy, dt(-2)), dt(h + 1)))
    return fx, fy


def _taps(fx, fy, tx, ty, src_pos, src_normal, src_nosurf, n, p, w, h, dt, bits=None):
    """Keep bits (unless given) and normalised weights of the four taps at (tx, ty) for N pixels; src_* are one layer [h, w, ...].

    With given bits the whole decision is given - the origin, the kept set and that the try succeeded - so no threshold is left: the kept
    weights are normalised whatever their sum.  The origin then need not be this model's own floor(): where the position lies on a pixel
    centre within rounding, the fraction towards a given origin may come out as 1 + 1e-7 or as exactly 1, and a kept set in the column
    (row) that weighs ~0 would have a sum of zero or below.  The fractions are therefore held inside [2^-24, 1 - 2^-24], half a float32
    step at 1: the normalised weights are then the limit they have at the tie, and move by less than a float32 rounding elsewhere."""
    qx, qy = fx - tx.astype(dt), fy - ty.astype(dt)
    if bits is not None:
        qx, qy = np.clip(qx, dt(TIE_FRACTION), dt(1) - dt(TIE_FRACTION)), np.clip(qy, dt(TIE_FRACTION), dt(1) - dt(TIE_FRACTION))
    sx, sy = (dt(1) - qx, qx), (dt(1) - qy, qy)
    own = np.zeros(len(fx), np.uint8)
    cw = np.zeros((len(fx), 4), dt)
    for k in range(4):
        x, y = tx + (k & 1), ty + (k >> 1)
        inside = (x >= 0) & (y >= 0) & (x < w) & (y < h)
        xc, yc = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
        pp = src_pos[yc, xc, :3].astype(dt)
        d = p - pp
        with np.errstate(all="ignore"):
            nt =octahedral_unpack(src_normal[yc, xc], dt)
            cosn = nt[:, 0] * n[:, 0] + nt[:, 1] * n[:, 1] + nt[:, 2] * n[:, 2]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            keep = inside & ~src_nosurf[yc, xc] & (cosn > dt(NORMAL_COS)) & (d2 < dt(DISTANCE_SQ))
        own |= (keep.astype(np.uint8) << k)
    use = own if bits is None else bits
    total = np.zeros(len(fx), dt)
    for k in range(4):
        cw[:, k] = np.where((use >> k) & 1, sx[k & 1] * sy[k >> 1], dt(0))
        total = total + cw[:, k]
    ok = total > dt(MIN_WEIGHT) if bits is None else use != 0
    with np.errstate(all="ignore"):
        cw = np.where(ok[:, None], cw / total[:, None], cw)
    return own, cw, ok


def _blend(color, tx, ty, bits, cw, w, h, dt):
    out = np.zeros((len(tx), 4), dt)
    for k in range(4):
        xc, yc = np.clip(tx + (k & 1), 0, w - 1), np.clip(ty + (k >> 1), 0, h - 1)
        t = np.where(((bits >> k) & 1).astype(bool)[:, None], color[yc, xc].astype(dt), dt(0))
        out = out + t * cw[:, k:k + 1]
    return out


class SpatialModel:
    def __init__(self, size, total_viewports, source_viewports, default_value=(np.nan,) * 4, dtype=np.float64):
        self.w, self.h = int(size[0]), int(size[1])
        self.total, self.sources = int(total_viewports), [int(v) for v in source_viewports]
        self.destinations = [v for v in range(self.total) if v not in self.sources]
        self.default = np.asarray(default_value, np.float64)
        self.dt = np.dtype(dtype).type
        self.last = {}

    def run(self, view_proj, src, dst, decisions=None):
        """view_proj [total][4][4]; src: color, normal, pos, instance_id as [S, h, w(, c)]; dst: normal, pos, instance_id as [D, h, w(, c)].
        Returns the colour of every viewport [total, h, w, 4] in this model's dtype; self.last holds "decisions" (the ones used),
        "own_decisions" (the ones this model makes; equal unless decisions were given) and "weights" (normalised, of the decisions used)."""
        dt, w, h = self.dt, self.w, self.h
        N = w * h
        ys, xs = np.divmod(np.arange(N), w)
        out = np.zeros((self.total, h, w, 4), dt)
        D = len(self.destinations)
        own_rec = np.zeros((D, h, w), RECORD)
        weights = np.zeros((D, h, w, 4), dt)
        src_ns = [no_surface(src["pos"][s], src["instance_id"][s]) for s in range(len(self.sources))]
        for s, v in enumerate(self.sources):
            out[v] = src["color"][s].astype(dt)
        for d, v in enumerate(self.destinations):
            pos = np.asarray(dst["pos"][d]).reshape(N, -1)[:, :3]
            p = pos.astype(dt)
            n = octahedral_unpack(np.asarray(dst["normal"][d]).reshape(N, 2), dt)
            ns = no_surface(pos, np.asarray(dst["instance_id"][d]).reshape(N))
            surf = ~ns
            proj = []
            for s, sv in enumerate(self.sources):
                cw_, depth, u, vv = project(view_proj[sv], p, dt)
                with np.errstate(all="ignore"):
                    ok = surf & (cw_ > 0) & (depth < dt(1))
                fx, fy = tap_position(u, vv, w, h, dt)
                proj.append((ok, depth, fx, fy))
            # ---- this model's own decisions
            rec = np.zeros(N, RECORD)
            wts = np.zeros((N, 4), dt)
            col = np.broadcast_to(self.default.astype(dt), (N, 4)).copy()
            cand = np.full(N, -1)
            cand_depth = np.full(N, dt(1))
            for s, (ok, depth, _, _) in enumerate(proj):
                better = ok & (depth < cand_depth)
                cand[better] = s
                cand_depth[better] = depth[better]
            best = np.full(N, dt(1))
            done = np.zeros(N, bool)
            for phase in (0, 1):
                for s, (ok, depth, fx, fy) in enumerate(proj):
                    m = ((cand == s) if phase == 0 else (~done & (cand != s) & ok & (depth < best)))
                    idx = np.nonzero(m)[0]
                    if not len(idx):
                        continue
                    tx, ty = np.floor(fx[idx]).astype(np.int64), np.floor(fy[idx]).astype(np.int64)
                    bits, cw, good = _taps(fx[idx], fy[idx], tx, ty, src["pos"][s], src["normal"][s], src_ns[s], n[idx], p[idx], w, h, dt)
                    c = _blend(src["color"][s], tx, ty, bits, cw, w, h, dt)
                    g = idx[good]
                    col[g] = c[good]
                    best[g] = depth[g]
                    wts[g] = cw[good]
                    rec["kind"][g], rec["slot"][g], rec["bits"][g] = REPROJECTED, s, bits[good]
                    rec["ox"][g], rec["oy"][g] = tx[good], ty[good]
                    if phase == 0:
                        done[g] = True
            sky_done = np.zeros(N, bool)
            for s in range(len(self.sources)):
                m = ns & ~sky_done & src_ns[s].reshape(N)
                col[m] = src["color"][s].reshape(N, 4)[m].astype(dt)
                rec["kind"][m], rec["slot"][m] = SKY_COPY, s
                sky_done |= m
            own_rec[d] = rec.reshape(h, w)
            # ---- the value under given decisions
            if decisions is not None:
                given = np.asarray(decisions[d]).reshape(N)
                col = np.broadcast_to(self.default.astype(dt), (N, 4)).copy()
                wts = np.zeros((N, 4), dt)
                for s in range(len(self.sources)):
                    idx = np.nonzero((given["kind"] == REPROJECTED) & (given["slot"] == s))[0]
                    if len(idx):
                        _, _, fx, fy = proj[s]
                        tx, ty = given["ox"][idx].astype(np.int64), given["oy"][idx].astype(np.int64)
                        bits = given["bits"][idx]
                        _, cw, good = _taps(fx[idx], fy[idx], tx, ty, src["pos"][s], src["normal"][s], src_ns[s], n[idx], p[idx], w, h, dt, bits=bits)
                        c = _blend(src["color"][s], tx, ty, bits, cw, w, h, dt)
                        c[~good] = np.nan              # a decision nobody can make: reprojected without a kept tap
                        col[idx] = c
                        wts[idx] = cw
                    m = (given["kind"] == SKY_COPY) & (given["slot"] == s)
                    col[m] = src["color"][s].reshape(N, 4)[m].astype(dt)
            out[v] = col.reshape(h, w, 4)
            weights[d] = wts.reshape(h, w, 4)
        self.last = {"own_decisions": own_rec, "decisions": own_rec if decisions is None else np.asarray(decisions), "weights": weights}
        return out


def canonical(decisions, weights):
    """The decision without the ties of floor(): per pixel (kind, slot, the absolute tap pixels that are kept and carry a normalised weight
    above 1e-3, sorted).  A projection that lands on a pixel centre may take either neighbouring origin; the tap that differs then weighs ~0."""
    dec = np.asarray(decisions)
    out = np.full(dec.shape + (6,), -1, np.int64)
    out[..., 0], out[..., 1] = dec["kind"], np.where(dec["kind"] == NONE, 0, dec["slot"])
    taps = np.full(dec.shape + (4,), np.iinfo(np.int64).max, np.int64)
    for k in range(4):
        x, y = dec["ox"].astype(np.int64) + (k & 1), dec["oy"].astype(np.int64) + (k >> 1)
        keep = (dec["kind"] == REPROJECTED) & (((dec["bits"] >> k) & 1) == 1) & (np.asarray(weights)[..., k] > CANONICAL_WEIGHT)
        taps[..., k] = np.where(keep, y * 65536 + x, taps[..., k])
    taps.sort(-1)
    out[..., 2:] = np.where(taps == np.iinfo(np.int64).max, -1, taps)
    return out


def differing_share(a, b):
    """Share of pixels (per leading layer) whose canonical decisions differ."""
    diff = (a != b).any(-1)
    return diff.reshape(diff.shape[0], -1).mean(-1)


class TemporalModel:
    def __init__(self, size, layers, ratio, dtype=np.float64):
        self.w, self.h, self.layers = int(size[0]), int(size[1]), int(layers)
        self.dt = np.dtype(dtype).type
        self.ratio = self.dt(np.float32(ratio))
        self.history = None          # (colour, packed normal, pos, no-surface) of the last frame
        self.last = {}

    def reset_history(self):
        self.history = None

    def run(self, images, decisions=None):
        """images: color, normal, pos, screen_motion [L, h, w, c], instance_id [L, h, w] or None.  Returns the blended colour [L, h, w, 4]."""
        dt, w, h, L = self.dt, self.w, self.h, self.layers
        N = w * h
        color = np.asarray(images["color"]).astype(dt).copy()
        ids = images.get("instance_id")
        ns_all = no_surface(images["pos"], ids)
        own_rec = np.zeros((L, h, w), RECORD)
        weights = np.zeros((L, h, w, 4), dt)
        if self.history is not None:
            pc, pn, pp, pns = self.history
            for l in range(L):
                p = np.asarray(images["pos"][l]).reshape(N, -1)[:, :3].astype(dt)
                n = octahedral_unpack(np.asarray(images["normal"][l]).reshape(N, 2), dt)
                mo = np.asarray(images["screen_motion"][l]).reshape(N, 2).astype(dt)
                surf = ~ns_all[l].reshape(N)
                fx, fy = tap_position(mo[:, 0], mo[:, 1], w, h, dt)
                cur = color[l].reshape(N, 4)
                idx = np.nonzero(surf)[0]
                tx, ty = np.floor(fx[idx]).astype(np.int64), np.floor(fy[idx]).astype(np.int64)
                bits, cw, good = _taps(fx[idx], fy[idx], tx, ty, pp[l], pn[l], pns[l], n[idx], p[idx], w, h, dt)
                c = _blend(pc[l], tx, ty, bits, cw, w, h, dt)
                blended = cur[idx] * (dt(1) - self.ratio) + c * self.ratio
                good = good & ~np.isnan(blended).any(-1)
                rec = np.zeros(N, RECORD)
                g = idx[good]
                rec["kind"][g], rec["bits"][g], rec["ox"][g], rec["oy"][g] = REPROJECTED, bits[good], tx[good], ty[good]
                own_rec[l] = rec.reshape(h, w)
                wts = np.zeros((N, 4), dt)
                wts[g] = cw[good]
                new = cur.copy()
                new[g] = blended[good]
                if decisions is not None:
                    given = np.asarray(decisions[l]).reshape(N)
                    idx = np.nonzero(given["kind"] == REPROJECTED)[0]
                    tx, ty, bits = given["ox"][idx].astype(np.int64), given["oy"][idx].astype(np.int64), given["bits"][idx]
                    _, cw, good = _taps(fx[idx], fy[idx], tx, ty, pp[l], pn[l], pns[l], n[idx], p[idx], w, h, dt, bits=bits)
                    c = _blend(pc[l], tx, ty, bits, cw, w, h, dt)
                    c[~good] = np.nan
                    new = cur.copy()
                    new[idx] = cur[idx] * (dt(1) - self.ratio) + c * self.ratio
                    wts = np.zeros((N, 4), dt)
                    wts[idx] = cw
                color[l] = new.reshape(h, w, 4)
                weights[l] = wts.reshape(h, w, 4)
        self.history = (color.copy(), np.asarray(images["normal"]).copy(), np.asarray(images["pos"]).copy(), ns_all.copy())
        self.last = {"own_decisions": own_rec, "decisions": own_rec if decisions is None else np.asarray(decisions), "weights": weights}
        return color
