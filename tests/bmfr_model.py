"""A numpy model of the BMFR stage (trhip_bmfr_*, include/trhip.h), written from the algorithm and not from csrc/bmfr.hip's layout:
per-pixel steps as array expressions over whole images, the fit as numpy.linalg.lstsq per block.  float64 by default; `dtype=np.float32`
evaluates the same expressions at the kernels' precision (and fits with the model's own float32 Householder QR), which is what the
tolerances of tests/test_bmfr.py are measured with.

The steps, per frame (w x h pixels, L layers; images are [L][h][w][c]):
 (a) preprocess   noisy diffuse = `diffuse`, noisy specular = max(0, color - albedo * diffuse); four bilinear taps of the history of
                  noisy values at the position `screen_motion` points to, a tap kept when it is inside the image, had a surface, its normal
                  agrees (cos > 0.9) and the position test passes; exponential average with alpha = clamp(1 / history length, 0.01, 1).
                  Feature row 1, n, p, p^2 and the accumulated channels; all zero where the pixel has no surface.
 (b) fit          per 32 x 32 block of a grid shifted by -16 + offset[frame % 16] (pixels outside mirrored): features 4-9 scaled to the
                  block's min / max, noise on features 1-9, least squares of the ten features against each channel.
 (c) weighted sum the features without noise times the block's weights, clamped at 0.
 (d) accumulate   the same taps of the history of filtered values, alpha from the history length before the increment;
                  colour = albedo * diffuse + specular unless the pixel has no surface.
"""
import numpy as np

FEATURES = 10
INV_UINT32_MAX = np.float32(2.3283064365386963e-10)


def block_offsets():
    """The stage's 16 block offsets: Halton points (bases 2 and 3) of index 0..15 as even numbers of [-16, 16)."""
    out = np.zeros((16, 2), np.int32)
    for i in range(16):
        rev = int(format(i, "04b")[::-1], 2)
        num = (i % 3) * 9 + ((i // 3) % 3) * 3 + ((i // 9) % 3)
        out[i] = (2 * rev - 16, 2 * (num * 16 // 27) - 16)
    return out


def pcg4d(x, y, z, w):
    """pcg4d of csrc/rng.h on uint32 arrays; returns the first component."""
    v = [np.asarray(a, dtype=np.uint64) & 0xFFFFFFFF for a in np.broadcast_arrays(x, y, z, w)]
    m = np.uint64(0xFFFFFFFF)
    v = [(a * np.uint64(1664525) + np.uint64(1013904223)) & m for a in v]

    def mix(s):
        return [(s[0] + s[1] * s[3]) & m, (s[1] + s[2] * s[0]) & m, (s[2] + s[0] * s[1]) & m, (s[3] + s[1] * s[2]) & m]
    v = mix(v)
    v = [a ^ (a >> np.uint64(16)) for a in v]
    v = mix(v)
    return v[0].astype(np.uint32)


def noise_unit(x, y, layer, feature, frame):
    """u in [0, 1] of the fit's noise: float32(pcg4d(x, y, layer * 16 + feature, frame).x) * 2^-32 (float32 by definition)."""
    return pcg4d(x, y, np.uint64(layer) * np.uint64(16) + np.uint64(feature), frame).astype(np.float32) * INV_UINT32_MAX


def octahedral_unpack(o, T):
    o = np.asarray(o, dtype=T)
    x, y = o[..., 0], o[..., 1]
    z = T(1) - np.abs(x) - np.abs(y)
    t = np.clip(z, T(-1), T(0))
    x = x + t * (np.where(x >= 0, T(1), T(0)) * T(2) - T(1))
    y = y + t * (np.where(y >= 0, T(1), T(0)) * T(2) - T(1))
    ln = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / ln, y / ln, z / ln], -1)


def mirror(i, size):
    i = np.where(i < 0, -i - 1, np.where(i >= size, 2 * size - i - 1, i))
    return np.clip(i, 0, size - 1)


def tap_position(motion, w, h):
    """Top-left tap and fractions of the reprojected position.  float32 in the kernel's operation order whatever the model's precision:
    a floor that went the other way would move all four taps."""
    m = np.asarray(motion, dtype=np.float32)
    fx = m[..., 0] * np.float32(w) - np.float32(0.5)
    fy = (np.float32(1) - m[..., 1]) * np.float32(h) - np.float32(0.5)
    fx = np.where(np.isnan(fx), np.float32(-2), fx)
    fy = np.where(np.isnan(fy), np.float32(-2), fy)
    fx = np.minimum(np.maximum(np.float32(-2), fx), np.float32(w) + np.float32(1))
    fy = np.minimum(np.maximum(np.float32(-2), fy), np.float32(h) + np.float32(1))
    flx, fly = np.floor(fx), np.floor(fy)
    return flx.astype(np.int64), fly.astype(np.int64), (fx - flx), (fy - fly)


def scale_feature(v, lo, hi):
    rng = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.abs(rng) > 1, (v - lo) / np.where(rng == 0, 1, rng), v - lo)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def householder_f32(A, B):
    """Least squares by Householder QR in float32, the textbook form on the whole matrix: A [rows][10], B [rows][channels] ->
    weights [channels][10].  A zero pivot column leaves its weight 0."""
    M = np.concatenate([A, B], 1).astype(np.float32)
    n = A.shape[1]
    for k in range(n):
        x = M[k:, k]
        norm = np.sqrt(np.sum(x * x, dtype=np.float32))
        if not norm > 0:
            continue
        alpha = -norm if x[0] > 0 else norm
        v = x.copy()
        v[0] = v[0] - alpha
        vv = np.sum(v * v, dtype=np.float32)
        if not vv > 0:
            continue
        tau = (np.float32(2) / vv) * (v @ M[k:, k:])
        M[k:, k:] -= np.outer(v, tau).astype(np.float32)
        M[k, k] = alpha
        M[k + 1:, k] = 0
    R, Q = M[:n, :n], M[:n, n:]
    W = np.zeros((B.shape[1], n), np.float32)
    for c in range(B.shape[1]):
        for i in range(n - 1, -1, -1):
            s = Q[i, c] - np.sum(R[i, i + 1:] * W[c, i + 1:], dtype=np.float32)
            W[c, i] = s / R[i, i] if R[i, i] != 0 else 0
            if not np.isfinite(W[c, i]):
                W[c, i] = 0
    return W


def lstsq_weights(A, B):
    """The float64 least-squares solution (minimum norm where the matrix is rank deficient): weights [channels][10]."""
    return np.linalg.lstsq(A.astype(np.float64), B.astype(np.float64), rcond=None)[0].T


def prepare_blocks(rows, bw, bh, frame, noise_amount=1e-2, dtype=np.float64):
    """Step (b) before the fit: `rows` [blocks][10 + C][1024] unscaled and without noise (row = y * 32 + x inside the block, blocks in
    layer, y, x order) -> (matrix with features 4-9 scaled and noise on features 1-9 of the rows with a surface, min / max [blocks][6][2])."""
    T = dtype
    M = np.array(rows, dtype=T)
    nb = M.shape[0]
    minmax = np.zeros((nb, 6, 2), T)
    r = np.arange(1024)
    for b in range(nb):
        layer, inb = divmod(b, bw * bh)
        by, bx = divmod(inb, bw)
        surf = M[b, 0] != 0
        if not surf.any():
            continue
        for f in range(6):
            lo, hi = M[b, 4 + f][surf].min(), M[b, 4 + f][surf].max()
            minmax[b, f] = (lo, hi)
            M[b, 4 + f] = np.where(surf, scale_feature(M[b, 4 + f], lo, hi), M[b, 4 + f])
        if noise_amount:
            amp = T(np.float32(noise_amount)) * T(2)
            for c in range(1, FEATURES):
                u = noise_unit(bx * 32 + (r & 31), by * 32 + (r >> 5), layer, c, frame).astype(T)
                M[b, c] = np.where(surf, M[b, c] + amp * (u - T(0.5)), M[b, c])
    return M, minmax


class BmfrModel:
    def __init__(self, size, layers=1, settings=0, noise_amount=1e-2, dtype=np.float64):
        self.w, self.h, self.layers = int(size[0]), int(size[1]), int(layers)
        self.channels = 3 if settings == 0 else 6
        self.noise = noise_amount
        self.T = dtype
        self.bw, self.bh = (self.w + 31) // 32 + 1, (self.h + 31) // 32 + 1
        self.offsets = block_offsets()
        self.reset_history()

    def reset_history(self):
        self.have_history = False
        shp = (self.layers, self.h, self.w)
        self.noisy = [np.zeros(shp + (4,), self.T), np.zeros(shp + (4,), self.T)]
        self.filtered = [np.zeros(shp + (4,), self.T), np.zeros(shp + (4,), self.T)]
        self.prev_normal = np.zeros(shp + (2,), self.T)
        self.prev_pos = np.zeros(shp + (4,), self.T)

    # ---- taps
    def _taps(self, motion, n, p, nosurf):
        """accept bits [L][h][w] and the tap positions."""
        T, w, h = self.T, self.w, self.h
        tx, ty, qx, qy = tap_position(motion, w, h)
        bits = np.zeros(tx.shape, np.uint8)
        if self.have_history:
            lz = np.arange(self.layers)[:, None, None]
            prev_n = octahedral_unpack(self.prev_normal, T)
            for k in range(4):
                x, y = tx + (k & 1), ty + (k >> 1)
                inside = (x >= 0) & (y >= 0) & (x < w) & (y < h)
                xc, yc = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
                pp = self.prev_pos[lz, yc, xc]
                npv = prev_n[lz, yc, xc]
                d = p - pp[..., :3]
                cosn = dot3(npv, n)
                d2 = dot3(d, d)
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = d / np.sqrt(d2)[..., None]
                    wgt = np.clip(T(1) - np.abs(dot3(t, n)), T(0), T(1)) * np.clip(cosn, T(0), T(1))
                    wgt = np.where(d2 < T(np.float32(0.001)), T(1), wgt)
                    keep = inside & (pp[..., 3] == 0) & (cosn > T(np.float32(0.9))) & (wgt > T(0.5)) & ~nosurf
                bits |= (keep.astype(np.uint8) << k)
        return bits, tx, ty, qx.astype(T), qy.astype(T)

    def _tap_weights(self, bits, qx, qy):
        T = self.T
        sx, sy = [T(1) - qx, qx], [T(1) - qy, qy]
        cw = [np.where((bits >> k) & 1, sx[k & 1] * sy[k >> 1], T(0)) for k in range(4)]
        s = ((cw[0] + cw[1]) + cw[2]) + cw[3]
        big = s > T(np.float32(1e-5))
        cw = [np.where(big, c / np.where(big, s, T(1)), c) for c in cw]
        return s, cw

    def _blend(self, img, bits, tx, ty, cw):
        lz = np.arange(self.layers)[:, None, None]
        r = np.zeros(img.shape, self.T)
        for k in range(4):
            x, y = np.clip(tx + (k & 1), 0, self.w - 1), np.clip(ty + (k >> 1), 0, self.h - 1)
            t = np.where(((bits >> k) & 1).astype(bool)[..., None], img[lz, y, x], self.T(0))
            r = r + t * cw[k][..., None]
        return r

    def _mix(self, a, b, t):
        return a * (self.T(1) - t) + b * t

    def features(self, n, p, nosurf):
        f = np.concatenate([np.ones(n.shape[:-1] + (1,), self.T), n, p, p * p], -1)
        f = np.where(np.isnan(f), self.T(0), f)
        return np.where(nosurf[..., None], self.T(0), f)

    def gather_rows(self, per_pixel, frame):
        """[L][h][w][c] -> [blocks][c][1024] over the shifted, mirrored block grid of `frame`."""
        ox, oy = self.offsets[frame % 16]
        px = mirror(np.arange(self.bw * 32) - 16 + ox, self.w)
        py = mirror(np.arange(self.bh * 32) - 16 + oy, self.h)
        g = per_pixel[:, py[:, None], px[None, :]]                                   # [L][bh*32][bw*32][c]
        c = g.shape[-1]
        g = g.reshape(self.layers, self.bh, 32, self.bw, 32, c).transpose(0, 1, 3, 5, 2, 4)
        return g.reshape(self.layers * self.bh * self.bw, c, 1024)

    def run(self, targets, frame, fit=None, accept_bits=None):
        """One frame; returns the denoised colour [L][h][w][4].  `fit`: None = lstsq at float64 / the model's Householder at float32,
        or a function (A [1024][10], B [1024][C]) -> weights [C][10].  `accept_bits`: the tap decisions of another implementation
        ([L][h][w], bits 0-3) to continue with instead of the model's own (a tap at a threshold can be kept by one and dropped by the
        other; the model's own decisions stay in self.last["own_accept_bits"], so the caller can count where they differ).
        What the frame computed stays in self.last."""
        T, w, h = self.T, self.w, self.h
        col = np.asarray(targets["color"], T).reshape(self.layers, h, w, 4)
        dif = np.asarray(targets["diffuse"], T).reshape(self.layers, h, w, 4)
        alb = np.asarray(targets["albedo"], T).reshape(self.layers, h, w, 4)
        pos = np.asarray(targets["pos"], T).reshape(self.layers, h, w, 4)
        nrm_packed = np.asarray(targets["normal"], T).reshape(self.layers, h, w, 2)
        motion = np.asarray(targets["screen_motion"], np.float32).reshape(self.layers, h, w, 2)
        n = octahedral_unpack(nrm_packed, T)
        p = pos[..., :3]
        nosurf = np.isnan(p).any(-1)
        if targets.get("instance_id") is not None:
            nosurf = nosurf | (np.asarray(targets["instance_id"]).reshape(self.layers, h, w) < 0)
        with np.errstate(invalid="ignore"):
            x = col[..., :3] - alb[..., :3] * dif[..., :3]
            spec = np.where(x > 0, x, T(0))
        diffuse = dif[..., :3].copy()
        hist_len = np.ones((self.layers, h, w), T)

        # (a)
        bits, tx, ty, qx, qy = self._taps(motion, n, p, nosurf)
        own_bits = bits
        if accept_bits is not None:
            bits = (np.asarray(accept_bits).reshape(bits.shape) & 15).astype(np.uint8)
        sum_w, cw = self._tap_weights(bits, qx, qy)
        if self.have_history:
            dprev = self._blend(self.noisy[0], bits, tx, ty, cw)
            sprev = self._blend(self.noisy[1], bits, tx, ty, cw)
            use = (sum_w > T(np.float32(0.001))) & ~np.isnan(dprev).any(-1)
            hl = np.minimum(dprev[..., 3] + T(1), T(255))
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = np.clip(T(1) / hl, T(np.float32(0.01)), T(1))
            diffuse = np.where(use[..., None], self._mix(dprev[..., :3], diffuse, alpha[..., None]), diffuse)
            spec = np.where(use[..., None], self._mix(sprev[..., :3], spec, alpha[..., None]), spec)
            hist_len = np.where(use, hl, hist_len)
        diffuse = np.where(np.isnan(diffuse), T(0), diffuse)
        spec = np.where(np.isnan(spec), T(0), spec)
        noisy_new = [np.concatenate([diffuse, hist_len[..., None]], -1), np.concatenate([spec, np.ones_like(hist_len)[..., None]], -1)]

        feat = self.features(n, p, nosurf)
        chans = np.concatenate([diffuse, spec], -1)[..., :self.channels]
        chans = np.where(nosurf[..., None], T(0), chans)
        rows = self.gather_rows(np.concatenate([feat, chans], -1), frame)

        # (b)
        M, minmax = prepare_blocks(rows, self.bw, self.bh, frame, self.noise, T)
        weights = np.zeros((rows.shape[0], self.channels, FEATURES), T)
        for b in range(rows.shape[0]):
            A, B = M[b, :FEATURES].T, M[b, FEATURES:].T
            if not A.any():
                continue
            if fit is not None:
                weights[b] = fit(A, B)
            elif T == np.float32:
                weights[b] = householder_f32(A, B)
            else:
                weights[b] = lstsq_weights(A, B)

        # (c)
        ox, oy = self.offsets[frame % 16]
        bx = (np.arange(w) + 16 - ox) >> 5
        by = (np.arange(h) + 16 - oy) >> 5
        blk = (np.arange(self.layers)[:, None, None] * self.bh + by[None, :, None]) * self.bw + bx[None, None, :]
        f = feat.copy()
        for k in range(6):
            f[..., 4 + k] = np.where(nosurf, T(0), scale_feature(feat[..., 4 + k], minmax[blk, k, 0], minmax[blk, k, 1]))
        wsum = []
        for s in range(self.channels // 3):
            acc = np.zeros((self.layers, h, w, 3), T)
            for k in range(FEATURES):
                acc = acc + weights[blk, s * 3:s * 3 + 3, k] * f[..., k:k + 1]
            wsum.append(np.where(acc > 0, acc, T(0)))

        # (d)
        dcur = np.concatenate([wsum[0], np.ones((self.layers, h, w, 1), T)], -1)
        scur = np.concatenate([wsum[1], np.ones((self.layers, h, w, 1), T)], -1) if self.channels == 6 else noisy_new[1].copy()
        if self.have_history:
            dprev = self._blend(self.filtered[0], bits, tx, ty, cw)
            use = (bits != 0) & (sum_w > T(np.float32(0.001))) & ~np.isnan(dprev).any(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = np.clip(T(1) / dprev[..., 3], T(np.float32(0.01)), T(1))
            mixed = self._mix(dprev[..., :3], dcur[..., :3], alpha[..., None])
            dcur = np.where(use[..., None], np.concatenate([mixed, np.minimum(dprev[..., 3] + T(1), T(255))[..., None]], -1), dcur)
            if self.channels == 6:
                sprev = self._blend(self.filtered[1], bits, tx, ty, cw)
                scur = np.where(use[..., None], np.concatenate([self._mix(sprev[..., :3], scur[..., :3], alpha[..., None]), scur[..., 3:]], -1), scur)
        dcur[..., :3] = np.where(np.isnan(dcur[..., :3]), T(0), dcur[..., :3])
        scur[..., :3] = np.where(np.isnan(scur[..., :3]), T(0), scur[..., :3])
        out = np.concatenate([alb[..., :3] * dcur[..., :3] + scur[..., :3], np.ones((self.layers, h, w, 1), T)], -1)
        out = np.where(nosurf[..., None], col, out)

        self.last = dict(accept_bits=bits | (nosurf.astype(np.uint8) << 4), own_accept_bits=own_bits | (nosurf.astype(np.uint8) << 4), tap_x=tx, tap_y=ty, rows=rows, matrix=M, min_max=minmax,
                         weights=weights, weighted=wsum, hist_len=hist_len, nosurf=nosurf)
        self.noisy = noisy_new
        self.filtered = [dcur, scur if self.channels == 6 else self.filtered[1]]
        self.prev_normal = nrm_packed.copy()
        self.prev_pos = np.concatenate([p, nosurf.astype(T)[..., None]], -1)
        self.have_history = True
        return out
