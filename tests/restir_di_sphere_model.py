"""numpy model of ReSTIR DI's sphere lights as area lights (tauray_amd/csrc/restir_di.h `sphere lights`, restir_di_sphere.h), on top of
restir_di_model.py: the same operations in the same order at float32 or float64.  `with area_mode(): ...` puts the area mode's
sample_canonical and light_contribution in restir_di_model's place, around whatever is there (the uniform or the power selection's
sampler), so that a frame model written for the point mode models an area frame."""
from __future__ import annotations

import numpy as np

import restir_di_model as M
from restir_di_model import PI, create_tangent_space, dot, fmax2, ggx_lobes, mulT_tbn, normalize, sample_cone, unit


def oct_encode(n, dt):
    """`sphere lights` 1: unit vectors (..., 3) to (..., 2)"""
    n = np.asarray(n, dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs(n[..., 0]) + np.abs(n[..., 1]) + np.abs(n[..., 2])
        px, py = n[..., 0] / s, n[..., 1] / s
    sx, sy = np.where(px >= 0, dt(1), dt(-1)), np.where(py >= 0, dt(1), dt(-1))
    fx, fy = (dt(1) - np.abs(py)) * sx, (dt(1) - np.abs(px)) * sy
    lower = n[..., 2] < 0
    return np.stack([np.where(lower, fx, px), np.where(lower, fy, py)], -1).astype(dt)


def oct_decode(p, dt):
    p = np.asarray(p, dtype=dt)
    z = (dt(1) - np.abs(p[..., 0])) - np.abs(p[..., 1])
    t = fmax2(-z, dt(0))
    x = p[..., 0] + np.where(p[..., 0] >= 0, -t, t)
    y = p[..., 1] + np.where(p[..., 1] >= 0, -t, t)
    return normalize(np.stack([x, y, z], -1).astype(dt))


def _with_radius(L, typ, idx):
    """The type-0 samples whose light has radius != 0 (a NaN radius is != 0, as in the kernel)"""
    m = (typ == 0) & (idx < L.n_point)
    if m.any() and "radius" in (L.point.dtype.names or ()):
        radius = np.zeros(len(typ), dtype=np.float32)
        radius[m] = L.point["radius"][idx[m]]
        return m & (radius != 0)
    return np.zeros(len(typ), dtype=bool)


def sphere_cone(pl, pos, dt):
    """d, dist2 and the cutoff of the cone the spheres `pl` subtend at `pos` (sample_point_light's head)"""
    r = pl["radius"].astype(dt)
    d = pos.astype(dt) - pl["pos"].astype(dt)
    dist2 = dot(d, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = dt(1) - r * r / dist2
        cutoff = np.where(k > 0, np.sqrt(np.where(k > 0, k, dt(0))), dt(-1)).astype(dt)
    return d, dist2, cutoff


def sphere_point(pl, pos, u, min_ray_dist, dt):
    """`sphere lights` 2 for lights `pl` (records with a radius), receivers `pos` and the two free unit numbers `u` (N, 2): the outward
    normal of the drawn point, solid_pdf with its guard, the cone's direction and the distance along it."""
    r = pl["radius"].astype(dt)
    pos = pos.astype(dt)
    d, dist2, cutoff = sphere_cone(pl, pos, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        direction = sample_cone(u.astype(dt), -normalize(d), cutoff, dt)
        b = dot(d, direction)
        length = -b - np.sqrt(fmax2(b * b - dist2 + r * r, dt(0)))
        x = pos + direction * length[..., None]
        n = normalize(x - pl["pos"].astype(dt))
        solid_pdf = dt(1) / (dt(2) * dt(PI) * (dt(1) - cutoff))
        bad = np.isnan(n).any(-1) | (length <= dt(min_ray_dist))
    return n, np.where(bad, dt(1e9), solid_pdf).astype(dt), direction, length


def sphere_draw(L, words, pos, typ, idx, data, pdf, min_ray_dist, dt):
    """restir_sphere_draw behind either sampler: data and pdf of the type-0 samples whose light has a radius are replaced."""
    data, pdf = data.copy(), pdf.copy()
    m = _with_radius(L, typ, idx)
    if m.any():
        n, solid_pdf, _, _ = sphere_point(L.point[idx[m]], pos[m], unit(words[m], dt)[:, 1:3], min_ray_dist, dt)
        data[m] = oct_encode(n, dt)
        pdf[m] = pdf[m] * solid_pdf
    return data, pdf


def sample_canonical(L, words, pos, min_ray_dist, dt, base=None):
    """base: the sampler the helper runs behind (restir_di_model's uniform one, or the power selection's)"""
    typ, idx, data, pdf = (base or _POINT_SAMPLE_CANONICAL)(L, words, pos, min_ray_dist, dt)
    data, pdf = sphere_draw(L, words, pos, typ, idx, data, pdf, min_ray_dist, dt)
    return typ, idx, data, pdf


def light_contribution(L, typ, idx, data, dom, dt):
    """restir_contribution<true>: restir_di_model's for every sample but those on a light with a radius (`sphere lights` 3)"""
    typ, idx = np.asarray(typ), np.asarray(idx)
    value, direction, dist2, normal = _POINT_LIGHT_CONTRIBUTION(L, typ, idx, data, dom, dt)
    m = _with_radius(L, typ, idx)
    if not m.any():
        return value, direction, dist2, normal
    value, direction, dist2, normal = value.copy(), direction.copy(), dist2.copy(), normal.copy()
    pl = L.point[idx[m]]
    s = dom[m]
    sd = np.asarray(data)[m].astype(dt)
    pos = s["pos"].astype(dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = pl["radius"].astype(dt)
        n = oct_decode(sd, dt)
        p = (pl["pos"].astype(dt) + r[:, None] * n) - pos
        d = normalize(p)
        to = normalize(pl["pos"].astype(dt) - pos)
        fall = pl["dir_falloff"].astype(dt)
        cut = dot(to, -pl["dir"].astype(dt))
        inner = dt(1) - np.power((fmax2(dt(1) - cut, dt(0)) / (dt(1) - pl["dir_cutoff"].astype(dt))).astype(np.float64), fall.astype(np.float64)).astype(dt)
        spot = np.where(fall > 0, np.where(cut > pl["dir_cutoff"].astype(dt), inner, dt(0)), dt(1)).astype(dt)
        colour = (pl["color"].astype(dt) * spot[:, None]) / (r * r * dt(PI))[:, None]
        colour = np.where(~(dot(n, d) < 0)[:, None], dt(0), colour)      # >= 0 or NaN
        flat = s["flat_normal"].astype(dt)
        facing = ~(dot(d, flat) < dt(1e-6))
        tbn = create_tangent_space(s["mapped_normal"].astype(dt), dt)
        tview = mulT_tbn(-s["view"].astype(dt), tbn)
        tview = np.where((tview[..., 2] < dt(1e-5))[..., None], np.stack([tview[..., 0], tview[..., 1], fmax2(tview[..., 2], dt(1e-5))], -1), tview)
        diffuse, dielectric, metal = ggx_lobes(mulT_tbn(d, tbn), normalize(tview), s, dt)
        albedo = s["albedo"].astype(dt)[..., :3]
        v = (albedo * ((metal + dt(0)) + diffuse)[..., None] + dielectric[..., None]) * colour
    v = np.where((facing & ~np.isnan(sd).any(-1))[..., None], v, dt(0))
    value[m], direction[m], dist2[m], normal[m] = v, d, dot(p, p), n
    return value, direction, dist2, normal


_POINT_SAMPLE_CANONICAL = M.sample_canonical
_POINT_LIGHT_CONTRIBUTION = M.light_contribution


class area_mode:
    """`with area_mode(): ...` - inside, M.sample_canonical and M.light_contribution are the area mode's.  The sampler wraps the one that
    is there on entry, so that inside restir_di_selection_model.power_selection the helper runs behind the power selection's draw."""

    def __enter__(self):
        self.before = M.sample_canonical
        base = self.before
        M.sample_canonical = lambda L, words, pos, min_ray_dist, dt: sample_canonical(L, words, pos, min_ray_dist, dt, base)
        M.light_contribution = light_contribution

    def __exit__(self, *exc):
        M.sample_canonical = self.before
        M.light_contribution = _POINT_LIGHT_CONTRIBUTION
