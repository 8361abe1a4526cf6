"""numpy model of ReSTIR DI's power-proportional light selection (tauray_amd/csrc/restir_di.h `light selection`, restir_di_power.h,
include/tauray_alias.hh) on top of restir_di_model.py: the lights' weights in float32 in the kernel's order of
operations, the probabilities and the alias table in the host builder's double steps, and sample_canonical with the point and the
triangle class drawn through the table.  Shares no code with the library."""
from __future__ import annotations

import math

import numpy as np

import restir_di_model as M

UNIFORM, POWER = 0, 1
MODES = {"uniform": UNIFORM, "power": POWER}
ENTRY = np.dtype([("alias_id", "<u4"), ("probability", "<u4"), ("pdf", "<f4"), ("alias_pdf", "<f4")])
f32, f64 = np.float32, np.float64
_UNIFORM_SAMPLE_CANONICAL = M.sample_canonical      # the uniform selection's, whatever power_selection puts in its place


# ---------------------------------------------------------------------------------------------------------------- weights
def clean(w):
    """A weight that is negative, NaN or infinite is 0."""
    w = np.asarray(w, dtype=f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(w) & (w > 0), w, f32(0)).astype(f32)


def light_weights(point, tri):
    """k_restir_light_weights: float32 [n_point + n_tri].  point: POINT_LIGHT records (luminance of the colour; the cone and the radius
    are ignored), tri: TRI_LIGHT records (luminance of the decoded emission times the area; the texture is ignored)."""
    out = []
    if point is not None and len(point):
        out.append(M.luminance(point["color"].astype(f32), f32))
    if tri is not None and len(tri):
        P = tri["pos"].astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            area = f32(0.5) * M.length(M.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
            out.append(M.luminance(M.rgb9e5(tri["emission_factor"], f32), f32) * area)
    return clean(np.concatenate(out)) if out else np.zeros(0, dtype=f32)


# ---------------------------------------------------------------------------------------------------------------- the table
def probabilities(weights, uniform_fraction):
    """p_i = (1 - f) * w_i / sum(w) + f / n in double, the sum one running double sum in slot order; 1 / n when it is 0."""
    w = clean(weights).astype(f64)
    n = len(w)
    total = float(np.cumsum(w)[-1]) if n else 0.0
    f = f64(f32(uniform_fraction))
    if total > 0:
        return (f64(1) - f) * (w / f64(total)) + f / f64(n)
    return np.full(n, f64(1) / f64(n)) if n else np.zeros(0)


def _fixed32(v):
    r = math.ldexp(float(v), 32)
    return int(min(max(r, 0.0), 4294967295.0))


def alias_table(weights, uniform_fraction):
    """build_light_alias_table (tauray_alias.hh): one class's table over its n slots."""
    p = probabilities(weights, uniform_fraction)
    n = len(p)
    imp = [float(f64(n) * v) for v in p]
    table = np.zeros(n, dtype=ENTRY)
    alias = list(range(n))
    prob = [0xFFFFFFFF] * n
    i = j = 0
    while i < n and imp[i] > 1.0:
        i += 1
    while j < n and imp[j] <= 1.0:
        j += 1
    weight = imp[j] if j < n else 0.0
    while j < n:
        if weight > 1.0:
            if i >= n:
                break
            prob[i] = _fixed32(imp[i])
            alias[i] = j
            weight = (weight + imp[i]) - 1.0
            i += 1
            while i < n and imp[i] > 1.0:
                i += 1
        else:
            prob[j] = _fixed32(weight)
            old_j = j
            j += 1
            while j < n and imp[j] <= 1.0:
                j += 1
            if j < n:
                alias[old_j] = j
                weight = (weight + imp[j]) - 1.0
    table["alias_id"], table["probability"] = alias, prob
    table["pdf"] = p.astype(f32)
    table["alias_pdf"] = p[np.asarray(alias, dtype=np.int64)].astype(f32) if n else []
    return table


def selection_table(weights, n_point, n_tri, uniform_fraction):
    """The stage's table: the point lights' class, then the triangle lights'."""
    w = np.asarray(weights, dtype=f32)
    assert len(w) == n_point + n_tri
    return np.concatenate([alias_table(w[:n_point], uniform_fraction), alias_table(w[n_point:], uniform_fraction)])


def reconstructed_probabilities(table):
    """The probability with which the draw takes each light of one class's table, exactly, from the thresholds and the aliases: a slot is
    kept when the 32-bit word is <= its threshold."""
    from fractions import Fraction
    n = len(table)
    q = [Fraction(0)] * n
    for k in range(n):
        keep = Fraction(int(table["probability"][k]) + 1, 1 << 32)
        q[k] += keep / n
        q[int(table["alias_id"][k])] += (1 - keep) / n
    return np.array([float(v) for v in q])


# ---------------------------------------------------------------------------------------------------------------- the draw
def draw(table, words):
    """The draw of restir_sample_canonical_power for one class: words uint32 (N); returns the index and the float32 pdf."""
    n = len(table)
    p = words.astype(np.uint64) * np.uint64(n)
    slot = (p >> np.uint64(32)).astype(np.int64)
    low = (p & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    e = table[slot]
    take_alias = low > e["probability"].astype(np.uint64)
    idx = np.where(take_alias, e["alias_id"].astype(np.int64), slot)
    return np.clip(idx, 0, n - 1), np.where(take_alias, e["alias_pdf"], e["pdf"]).astype(f32)


def sample_canonical(L: M.Lights, table, words, pos, min_ray_dist, dt):
    """M.sample_canonical with the point and the triangle class through `table` ([n_point + n_tri] entries): the class is picked as
    there, the directional and the environment class are drawn as there, and so is the point on a triangle."""
    typ, idx, data, pdf = _UNIFORM_SAMPLE_CANONICAL(L, words, pos, min_ray_dist, dt)
    null = (typ == 0) & (idx == M.NULL_INDEX)
    m = (typ == 0) & ~null
    if m.any():
        i, p = draw(table[:L.n_point], words[m, 0])
        idx[m] = i
        pdf[m] = p.astype(dt) * dt(L.prob_point)
    m = typ == 1
    if m.any():
        u = M.unit(words, dt)
        i, p = draw(table[L.n_point:], words[m, 2])
        idx[m] = i
        P = L.tri["pos"][i].astype(dt)
        q = pos[m].astype(dt)
        A, B, C = P[:, 0] - q, P[:, 1] - q, P[:, 2] - q
        out_dir, tri_pdf = M.spherical_triangle(u[m, :2], A, B, C, dt)
        out_len = M.ray_plane_distance(out_dir, A, B, C)
        with np.errstate(invalid="ignore"):
            bad = np.isinf(tri_pdf) | (tri_pdf <= 0) | (out_len <= dt(min_ray_dist)) | np.isnan(out_dir).any(-1)
        tri_pdf = np.where(bad, dt(1e9), tri_pdf)
        data[m] = M.barycentric(out_dir * out_len[:, None], A, B, C, dt)[:, :2]
        pdf[m] = (tri_pdf * p.astype(dt)) * dt(L.prob_tri)
    return typ, idx, data, pdf


class power_selection:
    """`with power_selection(table): ...` - inside, M.sample_canonical is the power mode's, so that a frame model written for the uniform
    selection (tests/test_restir_di.py _model_frame) models a power frame from the downloaded table."""

    def __init__(self, table):
        self.table = table

    def __enter__(self):
        table = self.table
        M.sample_canonical = lambda L, words, pos, min_ray_dist, dt: sample_canonical(L, table, words, pos, min_ray_dist, dt)

    def __exit__(self, *exc):
        M.sample_canonical = _UNIFORM_SAMPLE_CANONICAL


# ---------------------------------------------------------------------------------------------------------------- the estimator
def ris_one_candidate(L: M.Lights, surface, table, seed, dt=f64):
    """RIS with one candidate and no reuse over point lights at `surface` (n records), every light visible: the estimate
    contribution * uc_weight (n, 3).  table None: the uniform selection."""
    n = len(surface)
    rs = M.pcg4d(M.init_sampler(np.arange(n) % 200, np.arange(n) // 200, 0, 0, seed))
    if table is None:
        typ, idx, data, pdf = _UNIFORM_SAMPLE_CANONICAL(L, rs, surface["pos"], 1e-4, dt)
    else:
        typ, idx, data, pdf = sample_canonical(L, table, rs, surface["pos"], 1e-4, dt)
    contrib = M.light_contribution(L, typ, idx, data, surface, dt)[0]
    t = M.luminance(contrib, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = M.nan_to_zero(t / pdf)
    rs = M.pcg4d(rs)
    wsum, take = M.update_reservoir(np.zeros(n, dtype=dt), w, M.unit(rs, dt)[:, 0])
    ucw = M.uc_weight(wsum, np.where(take, t, dt(0)), dt)
    return np.where(take[:, None], contrib, dt(0)) * ucw[:, None], idx
