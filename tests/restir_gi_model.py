"""numpy model of ReSTIR GI (tauray_amd/csrc/restir_gi.h, restir_gi.hip): what the stage adds to ReSTIR DI's rule, in the same operations
in the same order at float32 or float64, vectorised over pixels.  Everything the two stages share - the random numbers, the vector layer,
the BSDF lobes, sample_canonical, light_contribution, update_reservoir, the Jacobian, the MIS terms and the screen-space decisions - is
tests/restir_di_model.py's and is imported from there, unchanged.  float32 repeats the kernels bit for bit, float64 is the yardstick the
tests' bounds are taken from."""
from __future__ import annotations

import numpy as np

import restir_di_model as M

SAMPLER_W = 0x80000000      # RESTIR_GI_SAMPLER_W: the fourth sampler coordinate of the stage's streams
PASS_INITIAL, PASS_TEMPORAL, PASS_SPATIAL = 0, 1, 2


def sampler(px, py, viewport, frame, pass_index, rng_seed):
    """init_local_sampler((px, py, viewport, 0x80000000), 3 * frame + pass, pcg(rng_seed) or 0, uniform).rs"""
    return M.init_sampler(px, py, viewport, (SAMPLER_W + 3 * int(frame) + int(pass_index)) & 0xFFFFFFFF, rng_seed)


def di_sampler_w(frame, pass_index):
    """The fourth coordinate of ReSTIR DI's two streams (restir_di.h)."""
    return (2 * int(frame) + int(pass_index)) & 0xFFFFFFFF


def gi_sampler_w(frame, pass_index):
    return (SAMPLER_W + 3 * int(frame) + int(pass_index)) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- the initial direction
def concentric_disk(u, dt):
    """sample_concentric_disk<RoundedMath> (math.glsl:205-218)"""
    uo = dt(2) * u - dt(1)
    a = np.abs(uo)
    zero = (a[..., 0] < dt(0.0001)) & (a[..., 1] < dt(0.0001))
    first = a[..., 0] > a[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(first, uo[..., 0], uo[..., 1])
        t = np.where(first, dt(M.PI) / dt(4) * (uo[..., 1] / uo[..., 0]), dt(M.PI) / dt(2) - dt(M.PI) / dt(4) * (uo[..., 0] / uo[..., 1]))
        out = np.stack([r * M.cos(t, dt), r * M.sin(t, dt)], -1).astype(dt)
    return np.where(zero[..., None], dt(0), out)


def cosine_hemisphere(u, dt):
    """sample_cosine_hemisphere<RoundedMath> and pdf_cosine_hemisphere: the local direction (z up) and its pdf"""
    d = concentric_disk(u, dt)
    z = np.sqrt(M.fmax2(dt(0), dt(1) - (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])))
    local = np.stack([d[..., 0], d[..., 1], z], -1).astype(dt)
    return local, M.fmax2(z, dt(0)) * (dt(1) / dt(M.PI))


def initial_direction(u, dom, dt):
    """`initial` of restir_gi.h up to the ray: dir, pdf and whether the ray is cast"""
    local, pdf = cosine_hemisphere(u.astype(dt), dt)
    direction = M.mul_tbn(M.create_tangent_space(dom["mapped_normal"].astype(dt), dt), local)
    cast = ~((M.dot(direction, dom["flat_normal"].astype(dt)) < dt(1e-6)) | (pdf <= 0))
    return direction, pdf, cast


# ---------------------------------------------------------------------------------------------------------------- a sample at a surface
def is_null(n_s, L_o):
    return (np.asarray(n_s) == 0).all(-1) & (np.asarray(L_o) == 0).all(-1)


def contribution(x_s, n_s, L_o, dom, dt, bits=None):
    """restir_gi_contribution: value (N, 3), dir (N, 3), dist2 (N) of samples at surface records `dom` (arrays by field name).  `bits`,
    a dict, receives the three discrete tests (alive: not null and dist2 > 0; above: the direction clears the flat normal; facing: n_s
    faces the surface)."""
    x_s, n_s, L_o = x_s.astype(dt), n_s.astype(dt), L_o.astype(dt)
    null = is_null(n_s, L_o)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        to = x_s - dom["pos"].astype(dt)
        dist2 = M.dot(to, to)
        direction = M.normalize(to)
        alive = ~null & (dist2 > 0)
        flat = dom["flat_normal"].astype(dt)
        above = ~(M.dot(direction, flat) < dt(1e-6))
        facing = ~(M.dot(n_s, -direction) < dt(1e-6))
        tbn = M.create_tangent_space(dom["mapped_normal"].astype(dt), dt)
        tview = M.mulT_tbn(-dom["view"].astype(dt), tbn)
        tview = np.where((tview[..., 2] < dt(1e-5))[..., None], np.stack([tview[..., 0], tview[..., 1], M.fmax2(tview[..., 2], dt(1e-5))], -1), tview)
        shading_view = M.normalize(tview)
        shading_light = M.mulT_tbn(direction, tbn)
        diffuse, dielectric, metal = M.ggx_lobes(shading_light, shading_view, dom, dt)
        albedo = dom["albedo"].astype(dt)[..., :3]
        value = (albedo * ((metal + dt(0)) + diffuse)[..., None] + dielectric[..., None]) * L_o
    if bits is not None:
        bits.update(alive=alive, above=above & alive, facing=facing & above & alive)
    value = np.where((alive & above & facing)[..., None], value, dt(0))
    return value, np.where(null[..., None], dt(0), direction), np.where(null, dt(0), dist2)


def radiance(light_contribution, visibility, light_pdf, dt):
    """L_o = (contribution * visibility) / light_pdf per component, 0 if any component is NaN or inf"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L = (light_contribution.astype(dt) * visibility.astype(dt)[..., None]) / light_pdf.astype(dt)[..., None]
    return np.where(np.isfinite(L).all(-1)[..., None], L, dt(0))


def casts(c):
    return (c > 0).any(-1)


def initial_weight(target, pdf, prev_confidence, dt):
    """(1 / (1 + prev_confidence)) * target / pdf, NaN -> 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return M.nan_to_zero((dt(1) / (dt(1) + prev_confidence)) * target / pdf)


def temporal_merge(target, pdf, prev, reuse, max_confidence, u_initial, u_merge, dt, temporal=True):
    """k_restir_gi_temporal behind its reprojection: the initial sample (target, pdf) enters an empty reservoir with DI's one-candidate
    weight, then - where `reuse` - the history reservoir `prev` = (its sample's target at this surface, uc_weight, confidence) is merged
    by confidence.  Returns a dict: weight (initial), take_initial, weight_prev, take_prev, target_function, uc_weight, confidence."""
    t_prev, w_prev, c_prev = (np.asarray(x).astype(dt) for x in prev)
    prev_confidence = np.where(reuse, c_prev, dt(0)).astype(dt)
    weight = initial_weight(target.astype(dt), pdf.astype(dt), prev_confidence, dt)
    wsum, take = M.update_reservoir(np.zeros_like(weight), weight, u_initial)
    tf = np.where(take, target.astype(dt), dt(0))
    confidence = np.ones_like(weight)
    ucw = M.uc_weight(wsum, tf, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        weight_prev = M.nan_to_zero(((c_prev / (confidence + c_prev)) * t_prev) * w_prev)
    wsum2, take_prev = M.update_reservoir(wsum, weight_prev, u_merge)
    take_prev = take_prev & reuse
    wsum = np.where(reuse, wsum2, wsum)
    tf = np.where(take_prev, t_prev, tf)
    confidence = np.where(reuse, confidence + c_prev, confidence)
    ucw = np.where(reuse, M.uc_weight(wsum, tf, dt), ucw)
    if temporal:
        confidence = M.fmin2(confidence, dt(max_confidence))
    return dict(weight=weight, take_initial=take, weight_prev=np.where(reuse, weight_prev, dt(0)), take_prev=take_prev, target_function=tf, uc_weight=ucw,
                confidence=confidence)


def spatial_merge(canonical, neighbours, draws, u_canonical, dt):
    """k_restir_gi_spatial's merge at one surface.  `canonical` = (target_function, uc_weight, confidence); every neighbour a dict of
    arrays: target_function, uc_weight, confidence (its reservoir), target_n (its sample here, shadowed), jacobian_n, target_c (the
    canonical sample there, shadowed), jacobian_c, held, live (held and its sample not null), canonical_live (held and the canonical
    sample not null).  Returns a dict: per slot m, wi, take, mis_canonical; canonical_m, final_wi, take_canonical, chosen (-1 none, k a
    slot, len(neighbours) the canonical sample), target_function, uc_weight, confidence."""
    c_t, c_w, c_c = (np.asarray(x).astype(dt) for x in canonical)
    total = c_c
    for n in neighbours:
        total = np.where(n["held"], total + n["confidence"].astype(dt), total)
    with np.errstate(invalid="ignore", divide="ignore"):
        canonical_m = c_c / total
    wsum = np.zeros_like(c_t)
    tf = np.zeros_like(c_t)
    chosen = np.full(c_t.shape, -1)
    confidence = np.zeros_like(c_t)
    out = dict(m=[], wi=[], take=[], mis_canonical=[])
    for k, n in enumerate(neighbours):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            m = M.mis_noncanonical(c_c, n["confidence"].astype(dt), total, n["target_function"].astype(dt), n["target_n"].astype(dt), n["jacobian_n"].astype(dt), dt)
            wi = M.nan_to_zero(((n["target_n"].astype(dt) * m) * n["uc_weight"].astype(dt)) * n["jacobian_n"].astype(dt))
            mc = M.mis_canonical(c_c, n["confidence"].astype(dt), total, c_t, n["target_c"].astype(dt), n["jacobian_c"].astype(dt), dt)
        wsum2, take = M.update_reservoir(wsum, wi, draws[k])
        take = take & n["live"]
        wsum = np.where(n["live"], wsum2, wsum)
        chosen, tf = np.where(take, k, chosen), np.where(take, n["target_n"].astype(dt), tf)
        confidence = np.where(n["held"], confidence + n["confidence"].astype(dt), confidence)
        canonical_m = np.where(n["canonical_live"], canonical_m + mc, canonical_m)
        for key, val, mask in (("m", m, n["live"]), ("wi", wi, n["live"]), ("take", take, n["live"]), ("mis_canonical", mc, n["canonical_live"])):
            out[key].append(np.where(mask, val, np.zeros_like(val)))
    with np.errstate(invalid="ignore"):
        final_wi = M.nan_to_zero((canonical_m * c_t) * c_w)
    wsum, take = M.update_reservoir(wsum, final_wi, u_canonical)
    chosen, tf = np.where(take, len(neighbours), chosen), np.where(take, c_t, tf)
    confidence = confidence + c_c
    out.update(canonical_m=canonical_m, final_wi=final_wi, take_canonical=take, chosen=chosen, target_function=tf, uc_weight=M.uc_weight(wsum, tf, dt),
               confidence=confidence)
    return out
