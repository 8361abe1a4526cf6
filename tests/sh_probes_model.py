"""numpy model of the SH probe-grid baking stage (tauray_amd/csrc/sh_probes.h; include/trhip.h "sh_path_tracer_stage"), written from the
rule: at float32 in the pinned order of operations - every product, sum, quotient and square root rounded on its own; sin, cos and pow
evaluated at double and rounded once - and at float64, where the same expressions stand for the rule itself.

The radiance of a ray comes from a callable, so the model knows no scene: `BoxScene` below is the analytic one of the deterministic test (an
axis-aligned box seen from inside, one emitter material per face, max_bounces = 1 and no light sampling)."""
from __future__ import annotations

import numpy as np

SH_BLOCK = 256
GOLDEN = 0.38196601125
SQRT3 = 3.0 ** 0.5


# ---------------------------------------------------------------------------------------------------
# hashes and the sampler (shader/math.glsl:75-123, shader/random_sampler.glsl:11-19), uint32 and wrapping
def pcg(seed):
    """Returns the new seed, which is also the value (GLSL `inout`)."""
    with np.errstate(over="ignore"):
        s = np.asarray(seed, dtype=np.uint32) * np.uint32(747796405) + np.uint32(2891336453)
        s = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
        return (s >> np.uint32(22)) ^ s


def pcg4d(v):
    """v: uint32 [..., 4]; returns the new seed, which is also the value."""
    with np.errstate(over="ignore"):
        v = np.asarray(v, dtype=np.uint32) * np.uint32(1664525) + np.uint32(1013904223)
        for rnd in range(2):
            x, y, z, w = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
            v = np.stack([x + y * w, y + z * x, z + x * y, w + y * z], axis=-1)
            if rnd == 0:
                v = v ^ (v >> np.uint32(16))
        return v


def init_sampler(coord, sample_counter, rng_seed):
    """init_local_sampler(uvec4(x, y, z, s)) of the uniform-random sampler: coord uint32 [..., 4]."""
    with np.errstate(over="ignore"):
        c = np.array(coord, dtype=np.uint32)
        c[..., 3] = c[..., 3] + np.uint32(sample_counter)
        c[..., 2] = c[..., 2] + np.uint32(rng_seed)
        x = pcg(c[..., 0])
        y = c[..., 1] ^ x
        yy = pcg(y)
        z = c[..., 2] ^ yy
        zz = pcg(z)
        w = c[..., 3] ^ zz
        return np.stack([x, yy, zz, w], axis=-1)


def seed_rule(rng_seed):
    """src/rt_stage.cc:82."""
    return int(pcg(rng_seed)) if rng_seed != 0 else 0


# ---------------------------------------------------------------------------------------------------
def _sin(x, dt):
    return np.sin(x.astype(np.float64)).astype(dt)


def _cos(x, dt):
    return np.cos(x.astype(np.float64)).astype(dt)


def _pow(x, y, dt):
    return np.power(x.astype(np.float64), np.float64(dt(y))).astype(dt)


def sample_sphere_phi(cos_theta, phi, dt):
    sin_theta = np.sqrt(dt(1) - cos_theta * cos_theta)
    return np.stack([_cos(phi, dt) * sin_theta, _sin(phi, dt) * sin_theta, cos_theta], axis=-1)


def local_dirs(s, n, rotation_x, rotation_y, dt=np.float32):
    """even_sample_sphere(s, N, (rotation_x, rotation_y)) for an array of sample indices."""
    sf = np.asarray(s).astype(dt)
    o = (sf + dt(rotation_x)) * dt(GOLDEN)
    u = (sf + dt(rotation_y)) / dt(n)
    cos_theta = dt(2) * u - dt(1)
    phi = (o * dt(2)) * dt(np.pi)
    return sample_sphere_phi(cos_theta, phi, dt)


def sh_basis(d, order, dt=np.float32):
    """sh_basis (shader/spherical_harmonics.glsl:31-69) in the order it is written: d [..., 3] -> [..., C]."""
    d = np.asarray(d, dtype=dt)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    x2, y2, z2 = x * x, y * y, z * z
    c = lambda v: dt(v)
    out = [np.full(x.shape, c(0.2820947917738781), dtype=dt)]
    if order >= 1:
        out += [c(0.4886025119029199) * y, c(0.4886025119029199) * z, c(0.4886025119029199) * x]
    if order >= 2:
        out += [c(1.0925484305920792) * x * y, c(1.0925484305920792) * y * z, c(0.3153915652525201) * (c(3) * z2 - c(1)),
                c(1.0925484305920792) * x * z, c(0.5462742152960396) * (x2 - y2)]
    if order >= 3:
        out += [c(0.5900435899266435) * y * (c(3) * x2 - y2), c(2.8906114426405543) * x * y * z, c(0.4570457994644658) * y * (c(5) * z2 - c(1)),
                c(0.3731763325901155) * z * (c(5) * z2 - c(3)), c(0.4570457994644658) * x * (c(5) * z2 - c(1)),
                c(1.4453057213202771) * z * (x2 - y2), c(0.5900435899266435) * x * (x2 - c(3) * y2)]
    if order >= 4:
        out += [c(2.503342941796705) * x * y * (x2 - y2), c(1.770130769779931) * y * z * (c(3) * x2 - y2),
                c(0.9461746957575602) * x * y * (c(7) * z2 - c(1)), c(0.6690465435572893) * y * z * (c(7) * z2 - c(3)),
                c(0.1057855469152043) * ((c(35) * z2 * z2 - c(30) * z2) + c(3)), c(0.6690465435572893) * x * z * (c(7) * z2 - c(3)),
                c(0.4730873478787801) * (x2 - y2) * (c(7) * z2 - c(1)), c(1.770130769779931) * x * z * (x2 - c(3) * y2),
                c(0.6258357354491763) * ((x2 * x2 - c(6) * x2 * y2) + y2 * y2)]
    return np.stack(out, axis=-1)


def matrix_orientation(transform, dt=np.float32):
    """mat3(get_matrix_orientation(transform)) (src/math.cc:44-52): the columns normalized, through glm's quaternion and back.  `transform`
    is a mathematical 4x4; the result a mathematical 3x3."""
    t = np.asarray(transform, dtype=dt)
    m = np.zeros((3, 3), dtype=dt)      # m[column][row], as glm indexes
    for c in range(3):
        v = t[:, c]
        ln = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
        m[c] = v[:3] / ln
    fx, fy = m[0][0] - m[1][1] - m[2][2], m[1][1] - m[0][0] - m[2][2]
    fz, fw = m[2][2] - m[0][0] - m[1][1], m[0][0] + m[1][1] + m[2][2]
    big, fbig = 0, fw
    for k, f in ((1, fx), (2, fy), (3, fz)):
        if f > fbig:
            big, fbig = k, f
    bv = np.sqrt(fbig + dt(1)) * dt(0.5)
    mult = dt(0.25) / bv
    if big == 0:
        qw, qx, qy, qz = bv, (m[1][2] - m[2][1]) * mult, (m[2][0] - m[0][2]) * mult, (m[0][1] - m[1][0]) * mult
    elif big == 1:
        qw, qx, qy, qz = (m[1][2] - m[2][1]) * mult, bv, (m[0][1] + m[1][0]) * mult, (m[2][0] + m[0][2]) * mult
    elif big == 2:
        qw, qx, qy, qz = (m[2][0] - m[0][2]) * mult, (m[0][1] + m[1][0]) * mult, bv, (m[1][2] + m[2][1]) * mult
    else:
        qw, qx, qy, qz = (m[0][1] - m[1][0]) * mult, (m[2][0] + m[0][2]) * mult, (m[1][2] + m[2][1]) * mult, bv
    qxx, qyy, qzz, qxz, qxy, qyz, qwx, qwy, qwz = qx * qx, qy * qy, qz * qz, qx * qz, qx * qy, qy * qz, qw * qx, qw * qy, qw * qz
    one, two = dt(1), dt(2)
    cols = [[one - two * (qyy + qzz), two * (qxy + qwz), two * (qxz - qwy)],
            [two * (qxy - qwz), one - two * (qxx + qzz), two * (qyz + qwx)],
            [two * (qxz + qwy), two * (qyz - qwx), one - two * (qxx + qyy)]]
    return np.array(cols, dtype=dt).T


def grid_data(transform, scaling, resolution, samples, frame_counter, history_length, temporal_ratio, dt=np.float32):
    """grid_data_buffer of render number `history_length` (1 = the first since creation or reset) at frame `frame_counter`
    (src/sh_path_tracer_stage.cc:115-137).  The inputs are the float32 values the stage is given, whatever `dt`."""
    t = np.asarray(transform, dtype=np.float32).astype(dt)
    counter = (int(frame_counter) * int(samples)) & 0xFFFFFFFF
    denom = dt(np.float32(0xFFFFFFFF))      # float(0xFFFFFFFFu) in the reference's host code
    inv = dt(1) / dt(history_length)
    return dict(transform=t, normal_transform=matrix_orientation(t, dt), resolution=tuple(int(r) for r in resolution),
                mix_ratio=max(inv, dt(np.float32(temporal_ratio))),
                cell_scale=(dt(0.5) * np.asarray(resolution).astype(dt)) / np.asarray(scaling, dtype=np.float32).astype(dt),
                rotation_x=dt(int(pcg(counter))) / denom, rotation_y=dt(int(pcg((counter + 1) & 0xFFFFFFFF))) / denom,
                sample_counter=counter)


def blackman_harris(u, dt):
    flip = u > dt(0.5)
    u = np.where(flip, dt(1) - u, u)
    s = ((((dt(0.29627329) * u + dt(-0.33518669) * _pow(u, 0.5, dt)) + dt(-0.51620529) * _pow(u, 0.3333333333, dt)) + dt(1.87406934) * _pow(u, 0.25, dt)) +
         dt(-0.66315464) * _pow(u, 0.2, dt))
    return np.where(flip, dt(1) - s, s)


def probe_rays(g, probe, samples, rng_seed=0, film=0, film_radius=1.0, dt=np.float32):
    """Origins [N, 3], world directions [N, 3] and probe-space directions [N, 3] of one probe (x, y, z)."""
    n = int(samples)
    s = np.arange(n)
    offset = np.zeros((n, 3), dtype=dt)
    if film != 0:
        coord = np.stack([np.full(n, probe[0]), np.full(n, probe[1]), np.full(n, probe[2]), s], axis=-1).astype(np.uint32)
        rs = pcg4d(init_sampler(coord, g["sample_counter"], seed_rule(rng_seed)))
        r = rs.astype(np.float32).astype(dt) * dt(np.float32(2.3283064365386963e-10))
        if film == 1:
            offset = r[:, :3] * dt(2) - dt(1)
        else:
            v = sample_sphere_phi(dt(2) * r[:, 0] - dt(1), (r[:, 1] * dt(2)) * dt(np.pi), dt)
            rad = _pow(np.abs(dt(2) * blackman_harris(r[:, 2], dt) - dt(1)), np.float32(1.0) / np.float32(3.0), dt)
            offset = v * rad[:, None]
    res = np.asarray(g["resolution"]).astype(dt)
    local = (((np.asarray(probe).astype(dt) + offset * dt(np.float32(film_radius))) + dt(0.5)) / res) * dt(2) - dt(1)
    t = g["transform"]
    origin = ((t[:3, 0] * local[:, 0:1] + t[:3, 1] * local[:, 1:2]) + t[:3, 2] * local[:, 2:3]) + t[:3, 3] * dt(1)
    ldir = local_dirs(s, n, g["rotation_x"], g["rotation_y"], dt)
    nt = g["normal_transform"]
    gd = (nt[:, 0] * ldir[:, 0:1] + nt[:, 1] * ldir[:, 1:2]) + nt[:, 2] * ldir[:, 2:3]
    ln = np.sqrt((gd[:, 0] * gd[:, 0] + gd[:, 1] * gd[:, 1]) + gd[:, 2] * gd[:, 2])
    return origin.astype(dt), (gd / ln[:, None]).astype(dt), ldir


def project(value, first_dist, ldir, g, order, dt=np.float32):
    """One probe: value [N, 3], first_dist [N], ldir [N, 3] -> the new coefficients [C, 4], summed in the tree of sh_probes.h."""
    n = len(ldir)
    sc = ldir * g["cell_scale"]
    ln = np.sqrt((sc[:, 0] * sc[:, 0] + sc[:, 1] * sc[:, 1]) + sc[:, 2] * sc[:, 2])
    dist = np.minimum(np.maximum(first_dist * ln, dt(0)), np.sqrt(dt(3)))
    coef_mult = (dt(4) * dt(np.pi)) / dt(n)
    coefs = np.concatenate([value, dist[:, None]], axis=1).astype(dt) * coef_mult
    terms = coefs[:, None, :] * sh_basis(ldir, order, dt)[:, :, None]      # [N, C, 4]
    acc = np.zeros((SH_BLOCK,) + terms.shape[1:], dtype=dt)
    for base in range(0, n, SH_BLOCK):
        chunk = terms[base:base + SH_BLOCK]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    waves = acc.reshape(SH_BLOCK // 64, 64, *terms.shape[1:])
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ off]
    w = waves[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


def bake(radiance, transform, scaling, resolution, order, samples, frame_counter=0, history_length=1, temporal_ratio=0.0, rng_seed=0,
         film=0, film_radius=1.0, previous=None, dt=np.float32):
    """One render of the stage: the volume [rz][ry * C][rx][4].  radiance(origin [N, 3], direction [N, 3], dt) -> (value [N, 3],
    first_dist [N]).  `previous`: the volume before this render (read when mix_ratio < 1)."""
    g = grid_data(transform, scaling, resolution, samples, frame_counter, history_length, temporal_ratio, dt)
    rx, ry, rz = g["resolution"]
    c = (order + 1) ** 2
    out = np.zeros((rz, ry * c, rx, 4), dtype=dt)
    for z in range(rz):
        for y in range(ry):
            for x in range(rx):
                origin, gdir, ldir = probe_rays(g, (x, y, z), samples, rng_seed, film, film_radius, dt)
                value, first_dist = radiance(origin, gdir, dt)
                out[z, y + ry * np.arange(c), x] = project(value, first_dist, ldir, g, order, dt)
    ratio = g["mix_ratio"]
    if ratio < 1:
        out = previous.astype(dt) * (dt(1) - dt(ratio)) + out * dt(ratio)
    return out


# ---------------------------------------------------------------------------------------------------
def modulate_color(albedo, metallic, diffuse, reflection, dt=np.float32):
    """modulate_color (shader/material.glsl:57-65)."""
    albedo, diffuse, reflection = (np.asarray(a, dtype=dt) for a in (albedo, diffuse, reflection))
    metallic = np.asarray(metallic, dtype=dt)[..., None]
    f = dt(0.02)
    dd = diffuse * albedo * (dt(1) - metallic)
    rr = reflection * (f * (dt(1) - metallic) + albedo * metallic) / (f * (dt(1) - metallic) + dt(1) * metallic)
    return dd + rr


class BoxScene:
    """An axis-aligned box [lo, hi] seen from inside; face f = 2 * axis + (0: the lo side, 1: the hi side) has emission[f] (rgb), albedo[f]
    (rgb) and metallic[f].  radiance() is evaluate_ray at max_bounces = 1 without light sampling, HIDE_LIGHTS and
    INDIRECT_CLAMP_FIRST_BOUNCE: the first hit's emission, clamped, through modulate_color with primary_lobes = (0, 0, 0, 1)."""

    def __init__(self, lo, hi, emission, albedo, metallic, indirect_clamping):
        self.lo, self.hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
        self.emission, self.albedo = np.asarray(emission, dtype=np.float32), np.asarray(albedo, dtype=np.float32)
        self.metallic = np.asarray(metallic, dtype=np.float32)
        self.clamp = np.float32(indirect_clamping)

    def hit(self, origin, direction, dt):
        lo, hi = self.lo.astype(dt), self.hi.astype(dt)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (np.where(direction > 0, hi, lo) - origin) / direction
        t = np.where(direction == 0, np.inf, t)
        axis = np.argmin(t, axis=1)
        rows = np.arange(len(origin))
        face = 2 * axis + (direction[rows, axis] > 0)
        return face, t[rows, axis].astype(dt)

    def radiance(self, origin, direction, dt=np.float32):
        face, t = self.hit(origin, direction, dt)
        pos = origin + direction * t[:, None]
        d = pos - origin
        first_dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        light = self.emission.astype(dt)[face]
        if self.clamp > 0:
            lum = (light[:, 0] * dt(np.float32(0.2126)) + light[:, 1] * dt(np.float32(0.7152))) + light[:, 2] * dt(np.float32(0.0722))
            clamp = dt(self.clamp)
            mul = np.where(lum > clamp, clamp / np.where(lum > 0, lum, dt(1)), dt(1))
            light = light * mul[:, None]
        reflection = np.zeros_like(light) + light * dt(1)
        diffuse = np.zeros_like(light) + light * dt(0)
        return modulate_color(self.albedo.astype(dt)[face], self.metallic.astype(dt)[face], diffuse, reflection, dt), first_dist
