"""numpy model of `path` of tauray_amd/csrc/restir_gi.h (k_restir_gi_initial_path, restir_gi_path.hip): the radiance L_o of a ReSTIR GI
sample as that of a path continued from x_s, in the same operations in the same order at float32 or float64, vectorised over paths.
Everything below the path - the random numbers, the cosine-hemisphere direction, the contribution of a sample at a surface, the radiance of
a light sample - is tests/restir_gi_model.py's and tests/restir_di_model.py's, imported and unchanged.  float32 repeats the kernel bit for
bit, float64 is the yardstick the tests' bounds are taken from."""
from __future__ import annotations

import numpy as np

import restir_di_model as M
import restir_gi_model as G

MAX_BOUNCES = 8     # RESTIR_GI_MAX_BOUNCES


def factor(x_next, n_next, dom, pdf, dt, bits=None):
    """f_k: the contribution of the sample (x_{k+1}, n_{k+1}, (1, 1, 1)) at the surface records `dom` of x_k, / pdf_k per component"""
    one = np.ones(np.shape(x_next), dtype=dt)
    c = G.contribution(x_next, n_next, one, dom, dt, bits)[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return c / np.asarray(pdf).astype(dt)[..., None]


def survives(T):
    """a throughput with a NaN or inf component or without a positive one ends the lane"""
    return np.isfinite(T).all(-1) & G.casts(T)


def advance(T, L_o, f, nee, reached, dt):
    """One vertex of the forward form: T' = T * f where the vertex was `reached` (the lane was alive, its ray was cast and hit), 0
    elsewhere; where T' survives, L_o' = L_o + T' * nee.  Returns T', L_o' and the lanes alive behind the vertex."""
    with np.errstate(invalid="ignore", over="ignore"):
        T2 = np.where(reached[..., None], T.astype(dt) * f.astype(dt), dt(0))
        alive = reached & survives(T2)
        L2 = np.where(alive[..., None], L_o.astype(dt) + T2 * nee.astype(dt), L_o.astype(dt))
    return T2, L2, alive


def forward(nee, factors, reached, dt):
    """L_o = NEE_1 + sum over k of T_{k+1} * NEE_{k+1}, T_{k+1} = T_k * f_k: `nee` = [NEE_1, ..., NEE_B], `factors` = [f_1, ..., f_{B-1}],
    `reached` = per extra vertex the paths whose ray from the vertex before was cast and hit.  Returns L_o, the throughputs [T_2, ...] and
    the running sums behind every extra vertex."""
    L_o = np.asarray(nee[0]).astype(dt)
    T = np.ones(L_o.shape, dtype=dt)
    alive = np.ones(L_o.shape[:-1], dtype=bool)
    Ts, sums = [], []
    for f, n, r in zip(factors, nee[1:], reached):
        T, L_o, alive = advance(T, L_o, f, n, alive & r, dt)
        Ts.append(T), sums.append(L_o)
    return L_o, Ts, sums


def backward(nee, vertices, doms, pdfs, dt):
    """The recursion the forward form unrolls, for paths that reached every vertex: L_o(x_k) = NEE_k + contribution(x_{k+1} carrying
    L_o(x_{k+1})) at x_k / pdf_k, from the last vertex to x_1.  `nee` = [NEE_1, ..., NEE_B], `vertices` = [(x_2, n_2), ..., (x_B, n_B)],
    `doms` = the surface records of x_1 ... x_{B-1}, `pdfs` = [pdf_1, ..., pdf_{B-1}].  The recursion has no throughput to test; it
    equals the forward form wherever every factor is finite: a throughput's components are products of non-negative factors, so one
    without a positive component makes every later term 0, which is what ending the lane makes them."""
    L = np.asarray(nee[-1]).astype(dt)
    for k in range(len(vertices) - 1, -1, -1):
        x, n = vertices[k]
        c = G.contribution(x, n, L, doms[k], dt)[0]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            L = np.asarray(nee[k]).astype(dt) + c / np.asarray(pdfs[k]).astype(dt)[..., None]
    return L


def initial_sample(x_1, n_1, L_o):
    """The sample the initial pass leaves: (x_1, n_1, L_o), or the null sample where the final sum has no positive component"""
    keep = G.casts(L_o)[..., None]
    return tuple(np.where(keep, a, a.dtype.type(0)) for a in (np.asarray(x_1), np.asarray(n_1), np.asarray(L_o)))


def draws(rs, steps):
    """The stream behind the initial pass's two draws: `rs` = the sampler state behind them (behind the first where x_s was not hit, no
    matter: such a path takes no further draw), `steps` = per extra vertex (took_direction, took_light), the paths that took the draw.
    Returns per extra vertex the state of the direction draw and of the light draw (the four words are the state itself)."""
    out = []
    for took_direction, took_light in steps:
        rs = np.where(took_direction[..., None], M.pcg4d(rs), rs)
        d = rs
        rs = np.where(took_light[..., None], M.pcg4d(rs), rs)
        out.append((d, rs))
    return out
