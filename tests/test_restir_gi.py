"""ReSTIR GI (trhip_restir_gi_*, tauray_amd/csrc/restir_gi.{h,hip}).

CPU: the ABI, the refusals of create and of the command line, the host sanitizers' program, and the numpy model of restir_gi.h
(tests/restir_gi_model.py on top of tests/restir_di_model.py) held to closed forms that need no GPU.  GPU: the stage against that model -
exactly where the model can be exact (the surface record, the secondary rays, the light sample at x_s, the replay of the reservoir
updates from the decision records, the random draws), within 4 |float32 model - float64 model| + one float32 ulp where it cannot (DI's
bound) - against the path tracer for its expectation, against itself for reuse and layout, and both hosts against each other."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import restir_di_model as M
import restir_gi_model as G
from conftest import GOLDEN, ROOT
from test_restir_di import _room, _lights_of, _plane_surface, _synthetic_records, _bits, _ulp32, _bounded, scene_min_ray_dist, _raw

f32, f64 = np.float32, np.float64
SIZES = ((13, 7), (37, 19))
CLI = os.path.join(ROOT, "tauray_amd", "tauray_hip")


@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


# =========================================================================================================================== CPU
def test_symbols_resolve_and_sizes_agree_with_the_header(tmp_path):
    from tauray_amd import _lib
    L = _lib.lib()
    for name in ("create", "destroy", "reset", "render", "get_timings", "download"):
        assert hasattr(L, "trhip_restir_gi_" + name) and "trhip_restir_gi_" + name in _lib.SYMBOLS
    structs = ["options", "reservoir", "initial", "timings"]
    codes = ["SURFACE", "CANONICAL", "HISTORY", "INITIAL", "SECONDARY", "LIGHT", "TEMPORAL", "SPATIAL", "FINAL"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "trhip.h"\nint main(void) {\n' +
                   "".join(f'    printf("%zu\\n", sizeof(trhip_restir_gi_{s}));\n' for s in structs) +
                   '    printf("' + " ".join(["%d"] * len(codes)) + '\\n", ' + ", ".join("TRHIP_RESTIR_GI_" + c for c in codes) + ");\n    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    header = dict(zip(structs, (int(v) for v in out[:len(structs)])))
    assert header == dict(options=28, reservoir=48, initial=96, timings=212)
    assert C.sizeof(_lib.RestirGiOptionsC) == header["options"] and C.sizeof(_lib.RestirGiTimingsC) == header["timings"]
    assert np.dtype(_lib.RESTIR_GI_RESERVOIR_DTYPE).itemsize == header["reservoir"] and np.dtype(_lib.RESTIR_GI_INITIAL_DTYPE).itemsize == header["initial"]
    assert [int(v) for v in out[len(structs)].split()] == [getattr(_lib, "RESTIR_GI_" + c) for c in codes] == list(range(9))
    assert _lib.RESTIR_GI_SAMPLER_W == G.SAMPLER_W


@pytest.mark.parametrize("size, layers, options, text", [
    ((16, 16), 1, {}, "no CPU fallback"),
    ((0, 16), 1, {}, "zero width, height or layer count"),
    ((16, 16), 0, {}, "zero width, height or layer count"),
    ((16385, 16), 1, {}, "image too large"),
    ((16, 16), 4097, {}, "image too large"),
    ((16, 16), 1, dict(spatial_samples=5), "spatial_samples 5 is outside 0..4"),
    ((16, 16), 1, dict(search_radius=0.0), "search_radius must be in (0, 1024]"),
    ((16, 16), 1, dict(search_radius=float("nan")), "search_radius must be in (0, 1024]"),
    ((16, 16), 1, dict(search_radius=2000.0), "search_radius must be in (0, 1024]"),
    ((16, 16), 1, dict(max_confidence=0.5), "max_confidence must be finite and at least 1"),
    ((16, 16), 1, dict(max_confidence=float("inf")), "max_confidence must be finite and at least 1"),
    ((16, 16), 1, dict(temporal_reuse=2), "temporal_reuse must be 0 or 1"),
    ((16, 16), 1, dict(min_ray_dist=0.0), "min_ray_dist must be finite and positive"),
    ((16, 16), 1, dict(record=3), "record must be 0 or 1"),
])
def test_create_refuses(R, size, layers, options, text):
    with pytest.raises(R.TrhipError) as e:
        R.RestirGiStage(None, None, size, layers, options)
    assert "trhip_restir_gi_create" in str(e.value) and text in str(e.value)
    with pytest.raises(AttributeError):
        R.restir_gi_options(candidates=3)


@pytest.mark.parametrize("args, text", [
    (["--renderer=restir-gi", "--denoiser=bmfr"], "--renderer=restir-gi: no --denoiser"),
    (["--renderer=restir-gi", "--taa=4"], "--renderer=restir-gi: no --taa"),
    (["--renderer=restir-gi", "--temporal-reprojection=0.5"], "--renderer=restir-gi: no --spatial-reprojection or --temporal-reprojection"),
    (["--renderer=restir-gi", "--camera-grid=2,1,0.1,0.1", "--spatial-reprojection=0"], "--renderer=restir-gi: no --spatial-reprojection or --temporal-reprojection"),
    (["--renderer=restir-gi", "--display=looking-glass"], "--renderer=restir-gi: no --display=looking-glass"),
    (["--renderer=restir-gi", "--samples-per-pixel=2"], "--renderer=restir-gi: one pass per frame, --samples-per-pixel must be 1"),
    (["--renderer=restir-gi", "--devices=0,1"], "--renderer=restir-gi runs on one device"),
    (["--renderer=restir-gi", "--process-count=2", "--process-rank=0"], "--renderer=restir-gi runs in one process"),
    (["--renderer=restir-gi", "--restir-gi=5"], "--restir-gi: spatial_samples must be a whole number in 0..4"),
    (["--renderer=restir-gi", "--restir-gi=2,-1"], "search_radius must be in (0, 1024]"),
    (["--renderer=restir-gi", "--restir-gi=2,8,0"], "max_confidence must be finite and at least 1"),
    (["--renderer=restir-gi", "--restir-gi=temporal_reuse=maybe"], "temporal_reuse=maybe is neither on nor off"),
    (["--renderer=restir-gi", "--restir-gi=radius=3"], "--restir-gi: radius is not one of its fields"),
    (["--renderer=restir-gi", "--restir=0"], "--restir: candidates must be a whole number in 1..32"),
    (["--restir-gi=2"], "--restir-gi sets the options of --renderer=restir-gi"),
    (["--renderer=restir-di", "--restir-gi=2"], "--restir-gi sets the options of --renderer=restir-gi"),
    (["--restir=4"], "--restir sets the options of --renderer=restir-di"),
    (["--renderer=dshgi", "--restir=4"], "--restir sets the options of --renderer=restir-di"),
    (["--renderer=restir"], "unknown renderer restir "),
    (["--renderer=restir-gi", "--denoiser=svgf"], "svgf"),
])
def test_cli_refuses(args, text):
    p = subprocess.run([CLI] + args + [os.path.join(GOLDEN, "test.glb"), "--width=16", "--height=16", "--filetype=none"], capture_output=True, text=True)
    assert p.returncode != 0 and text in p.stderr, p.stderr
    assert "--renderer=restir-gi [--restir-gi=spatial_samples,search_radius,max_confidence,temporal_reuse]" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout


def test_host_option_checks_under_the_sanitizers(tmp_path):
    """tests/restir_gi_check.cc: --restir-gi= parsing and the C++ renderer's option checks, built with address and undefined-behaviour
    sanitizers, no device."""
    exe = str(tmp_path / "restir_gi_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "restir_gi_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)

    def run(*a):
        p = subprocess.run([exe] + list(a), capture_output=True, text=True)
        return p.returncode, p.stdout.strip(), p.stderr.strip()
    assert run("parse", "") == (0, "2 32 16 1", "")
    assert run("parse", "3,12.5,20,off") == (0, "3 12.5 20 0", "")
    assert run("parse", "temporal_reuse=false,spatial_samples=0") == (0, "0 32 16 0", "")
    assert run("parse", "1,max_confidence=4") == (0, "1 32 4 1", "")
    for text, why in (("5", "spatial_samples must be a whole number in 0..4"), ("2.5", "spatial_samples must be a whole number"), ("2,8,16,on,1", "more than 4 values"),
                      ("spatial_samples=", "spatial_samples has no value"), ("x", "spatial_samples=x is not a number"), ("2,0", "search_radius must be in (0, 1024]"),
                      ("2,nan", "search_radius must be in (0, 1024]"), ("bogus=1", "bogus is not one of its fields"), ("candidates=4", "candidates is not one of its fields")):
        rc, out, err = run("parse", text)
        assert rc == 1 and why in err, (text, err)
    assert run("check", "2", "32", "16", "1e-4") == (0, "ok", "")
    for a, why in ((("5", "32", "16", "1e-4"), "spatial_samples 5 is outside 0..4"), (("2", "32", "0.5", "1e-4"), "max_confidence"), (("2", "32", "16", "0"), "min_ray_dist"),
                   (("2", "2000", "16", "1e-4"), "search_radius")):
        rc, out, err = run("check", *a)
        assert rc == 1 and why in err, (a, err)


# ---- the model against closed forms
def test_cosine_hemisphere_integrates_to_pi():
    """Over 10^5 seeded draws the mean of local.z / pdf is pi within 4 standard errors (it is pi for every draw up to rounding: the pdf
    is z / pi - so the spread is rounding alone), every direction is unit and in the upper hemisphere; the mean of z itself, whose
    expectation under the cosine density is 2 / 3, is held to 4 standard errors as well: that one has a spread."""
    n = 100_000
    rs = M.pcg4d(M.init_sampler(np.arange(n) % 400, np.arange(n) // 400, 0, G.gi_sampler_w(0, 0), 25))
    for dt, tol in ((f32, 2e-6), (f64, 1e-12)):
        local, pdf = G.cosine_hemisphere(M.unit(rs, dt)[:, :2], dt)
        assert (np.abs(np.linalg.norm(local.astype(f64), axis=-1) - 1) < tol).all() and (local[:, 2] >= 0).all()
        ok = pdf > 0
        assert ok.mean() > 0.999
        ratio = local[ok, 2].astype(f64) / pdf[ok].astype(f64)
        se = ratio.std(ddof=1) / math.sqrt(ok.sum())
        assert abs(ratio.mean() - math.pi) <= 4 * se + 1e-6 * math.pi, (dt, ratio.mean(), se)
        z = local[:, 2].astype(f64)
        assert abs(z.mean() - 2 / 3) <= 4 * z.std(ddof=1) / math.sqrt(n)
        # the direction about a normal is unit and above it
        nrm = np.tile(np.array([[0.3, 0.9, -0.2]]) / np.linalg.norm([0.3, 0.9, -0.2]), (n, 1)).astype(dt)
        d, p, cast = G.initial_direction(M.unit(rs, dt)[:, :2], dict(mapped_normal=nrm, flat_normal=nrm), dt)
        assert (np.abs(np.linalg.norm(d.astype(f64), axis=-1) - 1) < 4 * tol).all() and (M.dot(d, nrm)[cast] > 0).all() and cast.mean() > 0.99


def test_contribution_is_the_triangle_light_sample_of_the_same_point():
    """A GI sample (x_s, n_s, L_o) at a surface against restir_di_model's light_contribution of a triangle light whose first vertex is x_s,
    sampled at barycentrics (1, 0), with the same normal and with L_o as its emission (a value rgb9e5 holds exactly): the same float32
    bits wherever both are non-zero, the same direction and squared distance everywhere."""
    from tauray_amd import scene as S
    n = 512
    s, _, eye = _synthetic_records(n, seed=9)
    rng = np.random.default_rng(4)
    x = np.stack([rng.uniform(-2, 2, n), rng.uniform(0.3, 2.5, n), rng.uniform(-2, 2, n)], -1).astype(f32)
    emission = (200 << 0) | (120 << 9) | (60 << 18) | (17 << 27)
    L_o = np.tile(M.rgb9e5(np.array([emission]), f32), (n, 1))
    tri = np.zeros(n, dtype=S.TRI_LIGHT)
    e1 = np.array([0.25, 0.0, 0.0], dtype=f32)
    e2 = np.array([0.0, 0.0, 0.25], dtype=f32)
    tri["pos"][:, 0], tri["pos"][:, 1], tri["pos"][:, 2] = x, x + e2, x + e1      # normalize(cross(P2 - P0, P1 - P0)) = -y: facing down
    tri["emission_factor"], tri["emission_tex_id"] = emission, -1
    n_s = np.tile(np.array([[0.0, -1.0, 0.0]], dtype=f32), (n, 1))
    L = M.Lights(tri=tri)
    data = np.tile(np.array([[1.0, 0.0]], dtype=f32), (n, 1))
    both = 0
    for dt in (f32, f64):
        want, wdir, wd2, wn = M.light_contribution(L, np.ones(n, dtype=np.int64), np.arange(n), data, s, dt)
        got, gdir, gd2 = G.contribution(x, n_s, L_o, s, dt)
        assert (wn == n_s.astype(dt)).all()
        assert got.tobytes() == np.where((want != 0).any(-1, keepdims=True) & (got != 0).any(-1, keepdims=True), want, got).tobytes()
        assert gdir.tobytes() == wdir.tobytes() and gd2.tobytes() == wd2.tobytes()
        nz = (want != 0).any(-1) & (got != 0).any(-1)
        both += int(nz.sum())
        # one is zero without the other only through the two facing rules (DI: |cos| < 0.001 at the light; GI: cos < 1e-6 at x_s)
        assert ((want != 0).any(-1) == (got != 0).any(-1)).mean() > 0.98
    assert both > n
    # the null sample, a sample below the flat normal and one that faces away give nothing
    p = _plane_surface(3)
    xs = np.array([[0, 1, 0], [0.5, -1, 0], [0, 1, 0]], dtype=f32)
    ns = np.array([[0, 0, 0], [0, 1, 0], [0, 1, 0]], dtype=f32)
    Ls = np.array([[0, 0, 0], [1, 1, 1], [1, 1, 1]], dtype=f32)
    v, d, d2 = G.contribution(xs, ns, Ls, p, f32)
    assert (v == 0).all() and (d[0] == 0).all() and d2[0] == 0 and d2[1] > 0
    assert (G.contribution(xs[2:], np.array([[0, -1, 0]], dtype=f32), Ls[2:], p[:1], f32)[0] > 0).all()
    assert G.is_null(ns, Ls).tolist() == [True, False, False]


def test_jacobian_of_a_sample_reused_at_the_same_position_is_one():
    rng = np.random.default_rng(8)
    pos, x = rng.uniform(-2, 2, (256, 3)), rng.uniform(-2, 2, (256, 3))
    n = rng.normal(size=(256, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    for dt in (f32, f64):
        assert (M.jacobian(pos.astype(dt), pos.astype(dt), x.astype(dt), n.astype(dt), dt) == 1).all()
    # and moving the receiver towards x_s along the normal by half the distance: (1 / d^2 ratio) = 4 the other way round
    j = M.jacobian(np.array([[0.0, 2.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]), np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]]), f64)[0]
    assert abs(j - 4.0) < 1e-12


def test_merging_reservoirs_that_hold_one_sample_keeps_its_weight():
    """K reservoirs with the same sample (same target, same unbiased contribution weight W) and confidences c_k: the pairwise-MIS merge of
    the spatial kernel gives uc_weight W (to rounding) and confidence sum c_k whichever is chosen; the temporal merge of an initial
    sample with a history reservoir holding it gives W = 1 / pdf and min(1 + c, max_confidence)."""
    rng = np.random.default_rng(12)
    for dt, tol in ((f32, 2e-6), (f64, 1e-14)):
        for K in (2, 3, 5):
            n = 64
            conf = rng.integers(1, 17, (K, n)).astype(dt)
            t, W = rng.uniform(0.1, 3.0, n).astype(dt), rng.uniform(0.2, 5.0, n).astype(dt)
            yes = np.ones(n, dtype=bool)
            neighbours = [dict(target_function=t, uc_weight=W, confidence=conf[k], target_n=t, jacobian_n=np.ones(n, dtype=dt), target_c=t, jacobian_c=np.ones(n, dtype=dt),
                               held=yes, live=yes, canonical_live=yes) for k in range(1, K)]
            draws = [rng.random(n).astype(dt) for _ in range(K - 1)]
            out = G.spatial_merge((t, W, conf[0]), neighbours, draws, rng.random(n).astype(dt), dt)
            assert (np.abs(out["uc_weight"].astype(f64) / W.astype(f64) - 1) < tol * K).all()
            assert (out["confidence"] == conf.sum(0)).all() and (out["chosen"] >= 0).all() and (out["target_function"] == t).all()
            total = sum(x.astype(f64) for x in out["m"]) + out["canonical_m"].astype(f64)
            assert (np.abs(total - 1) < tol * K).all()
        n = 64
        t, pdf, c = rng.uniform(0.1, 3.0, n).astype(dt), rng.uniform(0.05, 1.0, n).astype(dt), rng.integers(1, 30, n).astype(dt)
        out = G.temporal_merge(t, pdf, (t, dt(1) / pdf, c), np.ones(n, dtype=bool), 16.0, rng.random(n).astype(dt), rng.random(n).astype(dt), dt)
        assert (np.abs(out["uc_weight"].astype(f64) * pdf.astype(f64) - 1) < tol).all()
        assert (out["confidence"] == np.minimum(1 + c, 16)).all() and (out["take_initial"]).all()
        alone = G.temporal_merge(t, pdf, (t, dt(1) / pdf, c), np.zeros(n, dtype=bool), 16.0, rng.random(n).astype(dt), rng.random(n).astype(dt), dt)
        assert (np.abs(alone["uc_weight"].astype(f64) * pdf.astype(f64) - 1) < tol).all() and (alone["confidence"] == 1).all() and not alone["take_prev"].any()


def test_model_float32_against_float64(capsys):
    """The model's own steps at both precisions on 4096 seeded synthetic records: the initial direction and its pdf, the contribution of
    a sample one metre or so above each record, a temporal merge with a history sample and a spatial merge with the record three places
    on.  No discrete decision of ReSTIR GI's own - ray cast or not, the three tests of the contribution, every update_reservoir - differs;
    the largest relative difference of each continuous quantity is printed and held to 2^-12 of the largest value of its kind, as DI's.
    (The neighbour offsets and the good / bad bits are DI's decisions, compared in tests/test_restir_di.py with DI's cap.)"""
    n = 4096
    s, L, eye = _synthetic_records(n)
    rng = np.random.default_rng(21)
    x = (s["pos"].astype(f64) + np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.4, 2.0, n), rng.uniform(-1.5, 1.5, n)], -1)).astype(f32)
    nrm = np.stack([rng.normal(0, 0.4, n), -np.ones(n), rng.normal(0, 0.4, n)], -1)
    n_s = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(f32)
    L_o = rng.uniform(0.0, 4.0, (n, 3)).astype(f32)
    prev_c, prev_w = rng.integers(1, 17, n).astype(f32), rng.uniform(0.5, 6.0, n).astype(f32)
    reuse = rng.random(n) < 0.7
    out = {}
    for dt in (f32, f64):
        rs = M.pcg4d(G.sampler(np.arange(n) % 64, np.arange(n) // 64, 0, 2, G.PASS_INITIAL, 0))
        direction, pdf, cast = G.initial_direction(M.unit(rs, dt)[:, :2], s, dt)
        bits = {}
        contrib, cdir, d2 = G.contribution(x, n_s, L_o, s, dt, bits)
        target = M.luminance(contrib, dt)
        other = np.roll(s, 3)
        bits_o = {}
        contrib_o = G.contribution(x, n_s, L_o, other, dt, bits_o)[0]
        target_o = M.luminance(contrib_o, dt)
        rs = G.sampler(np.arange(n) % 64, np.arange(n) // 64, 0, 2, G.PASS_TEMPORAL, 0)
        rs = M.pcg4d(rs)
        u0 = M.unit(rs, dt)[:, 0]
        rs = M.pcg4d(rs)
        u1 = M.unit(rs, dt)[:, 0]
        x_prev = np.roll(x, 5, 0)
        t_prev = M.luminance(G.contribution(x_prev, np.roll(n_s, 5, 0), np.roll(L_o, 5, 0), s, dt)[0], dt)
        tm = G.temporal_merge(target, pdf, (t_prev, prev_w, prev_c), reuse, 16.0, u0, u1, dt)
        j_n = M.jacobian(other["pos"].astype(dt), s["pos"].astype(dt), x_prev.astype(dt), np.roll(n_s, 5, 0).astype(dt), dt)
        j_c = M.jacobian(s["pos"].astype(dt), other["pos"].astype(dt), x.astype(dt), n_s.astype(dt), dt)
        yes = np.ones(n, dtype=bool)
        rs = M.pcg4d(rs)
        u2 = M.unit(rs, dt)[:, 0]
        rs = M.pcg4d(rs)
        u3 = M.unit(rs, dt)[:, 0]
        sm = G.spatial_merge((target, prev_w, prev_c), [dict(target_function=np.roll(target, 5), uc_weight=np.roll(prev_w, 2), confidence=np.roll(prev_c, 2), target_n=t_prev,
                                                               jacobian_n=j_n, target_c=target_o, jacobian_c=j_c, held=yes, live=yes, canonical_live=yes)], [u2], u3, dt)
        cont = dict(dir=direction, pdf=pdf, contribution=contrib, initial_weight=tm["weight"], temporal_weight=tm["weight_prev"], temporal_uc_weight=tm["uc_weight"],
                    jacobian_n=j_n, jacobian_c=j_c, m=sm["m"][0], wi=sm["wi"][0], canonical_m=sm["canonical_m"], final_wi=sm["final_wi"], spatial_uc_weight=sm["uc_weight"])
        disc = dict(cast=cast, alive=bits["alive"], above=bits["above"], facing=bits["facing"], above_o=bits_o["above"], facing_o=bits_o["facing"], take_initial=tm["take_initial"],
                    take_prev=tm["take_prev"], take_n=sm["take"][0], take_canonical=sm["take_canonical"], chosen=sm["chosen"])
        out[dt] = cont, disc
    (c32, d32), (c64, d64) = out[f32], out[f64]
    report = {}
    for k in c32:
        finite = np.isfinite(c64[k]) & np.isfinite(c32[k].astype(f64))
        report[k] = np.abs(c32[k].astype(f64) - c64[k])[finite].max() / np.abs(c64[k][finite]).max()
    differ = {k: int((d32[k] != d64[k]).sum()) for k in d32}
    with capsys.disabled():
        print(f"\nrestir gi model, float32 against float64 over {n} records: " + ", ".join(f"{k} {v:.2e}" for k, v in report.items()) +
              f"; discrete decisions that differ: {sum(differ.values())}")
    assert d32["cast"].any() and d32["facing"].any() and not d32["facing"].all() and d32["take_prev"].any() and not d32["take_prev"].all()
    assert d32["take_n"].any() and d32["take_canonical"].any()
    assert not any(differ.values()), differ
    for k, rel in report.items():
        assert rel <= 2.0 ** -12, (k, rel)


# =========================================================================================================================== GPU
class _Run:
    """`frames` frames of a recording stage over both viewports of the room: per frame `in`, the colour and every download."""
    NAMES = ("surface", "canonical", "history", "initial", "secondary", "light", "temporal", "final")

    def __init__(self, R, ctx, ss, size, frames=3, viewports=(0, 1), with_in=True, **options):
        self.size, self.viewports, self.options = size, tuple(viewports), R.restir_gi_options(record=True, **options)
        st = R.RestirGiStage(ctx, ss, size, len(self.viewports), self.options)
        shape = (len(self.viewports), size[1], size[0], 4)
        out = ctx.alloc(int(np.prod(shape)) * 4).zero()
        inp = ctx.alloc(int(np.prod(shape)) * 4).zero() if with_in else None
        rng = np.random.default_rng(77)
        self.frames = []
        for _ in range(frames):
            host_in = rng.uniform(0.0, 2.0, shape).astype(f32)
            if with_in:
                inp.upload(host_in)
            st.run(self.viewports, inp, out)
            f = {n: st.download(n) for n in self.NAMES}
            if self.options["spatial_samples"]:
                f["spatial"] = st.download("spatial")
            f["color"] = out.download(shape)
            f["in"] = host_in if with_in else np.broadcast_to(np.array([0, 0, 0, 1], dtype=f32), shape)
            self.frames.append(f)
        self.timings = st.timings()
        st.close()
        out.free()
        if inp is not None:
            inp.free()


@pytest.fixture(scope="module")
def rooms(R, ctx):
    """The room at the sizes of this file, uploaded on demand (one scene lives on the device at a time)."""
    from tauray_amd import scene as S
    scenes = {size: _room(S, size) for size in SIZES + ((64, 64),)}
    current = {}

    def get(size, as_strategy=0):
        if current.get("key") != (size, as_strategy):
            current["ss"] = R.SceneStage(ctx, scenes[size], as_strategy=as_strategy)
            current["key"] = (size, as_strategy)
        return scenes[size], current["ss"]
    return get


RUN_CASES = [((13, 7), dict(spatial_samples=0, temporal_reuse=False)), ((13, 7), dict(spatial_samples=2, temporal_reuse=True, search_radius=4.0)),
             ((37, 19), dict(spatial_samples=4, temporal_reuse=False, search_radius=6.0)), ((37, 19), dict(spatial_samples=0, temporal_reuse=True)),
             ((37, 19), dict(spatial_samples=3, temporal_reuse=True, search_radius=4.0, max_confidence=6.0))]
CASES = tuple(range(len(RUN_CASES)))


@pytest.fixture(scope="module")
def runs(R, ctx, rooms):
    """Every case of RUN_CASES rendered once; the tests below share the downloads and leave them unchanged."""
    cache = {}

    def get(i):
        if i not in cache:
            size, options = RUN_CASES[i]
            scene, ss = rooms(size)
            cache[i] = _Run(R, ctx, ss, size, rng_seed=31 + i, **options)
        return cache[i]
    return get


def _sample_of(rec):
    return rec["x_s"], rec["n_s"], rec["L_o"]


@pytest.mark.gpu
def test_surface_record_is_restir_di_s_and_miss_pixels_copy_in(R, ctx, rooms):
    """The surface record of a frame is RestirDiStage's of the same frame, byte for byte; a pixel without a surface has null reservoirs in
    both buffers and `in` as its colour; `in` = null counts as (0, 0, 0, 1)."""
    for size in SIZES:
        scene, ss = rooms(size)
        run = _Run(R, ctx, ss, size, frames=2, spatial_samples=1, temporal_reuse=True)
        di = R.RestirDiStage(ctx, ss, size, 2, R.restir_di_options(candidates=1, spatial_samples=0))
        sink = ctx.alloc(size[0] * size[1] * 16 * 2).zero()
        for f in run.frames:
            di.run((0, 1), sink)
            assert di.download("surface").tobytes() == f["surface"].tobytes()
            miss = f["surface"]["instance_id"] < 0
            assert miss.any() and not miss.all()
            assert (_bits(f["color"][miss]) == _bits(f["in"][miss])).all() and (_bits(f["color"][..., 3]) == _bits(f["in"][..., 3])).all()
            for name in ("canonical", "history"):
                assert (f[name][miss].view(np.uint32) == 0).all()
            assert (f["initial"]["traced"][miss] == 0).all() and (f["secondary"]["instance_id"][miss] == -1).all()
            assert np.isfinite(f["color"]).all() and (f["color"][..., :3][~miss] >= f["in"][..., :3][~miss]).all()
            assert (f["color"][..., :3][~miss] > f["in"][..., :3][~miss]).any()
        di.close()
        sink.free()
        bare = _Run(R, ctx, ss, size, frames=1, with_in=False, spatial_samples=1, temporal_reuse=True)
        f = bare.frames[0]
        miss = f["surface"]["instance_id"] < 0
        assert (f["color"][miss] == np.array([0, 0, 0, 1], dtype=f32)).all() and (f["color"][..., 3] == 1).all() and f["color"][..., :3].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", (0, 4))
def test_secondary_rays_hit_what_the_closest_hit_query_finds(rooms, runs, case):
    """The recorded secondary rays, given to trhip_trace_closest, return the recorded instance, primitive, u, v and t bit for bit; n_s is
    the normal of that quad on the side the ray arrived from and x_s lies on its plane to a few ulps of its coordinates."""
    run = runs(case)
    scene, ss = rooms(run.size)
    quad = scene.vertices["pos"].astype(f64).reshape(-1, 4, 3)
    face = np.cross(quad[:, 1] - quad[:, 0], quad[:, 3] - quad[:, 0])
    face /= np.linalg.norm(face, axis=-1, keepdims=True)
    hits = 0
    for f in run.frames:
        init, sec, surf = f["initial"], f["secondary"], f["surface"]
        traced = init["traced"] != 0
        assert traced.any() and (traced <= (surf["instance_id"] >= 0)).all()
        rays = np.zeros((int(traced.sum()), 8), dtype=f32)
        rays[:, :3], rays[:, 3], rays[:, 4:7], rays[:, 7] = surf["pos"][traced], run.options["min_ray_dist"], init["dir"][traced], np.inf
        got = ss.trace_closest(rays, None)
        rec = init[traced]
        assert (got["instance_id"] == rec["instance_id"]).all() and (got["primitive_id"] == rec["primitive_id"]).all()
        hit = rec["instance_id"] >= 0
        for a, b in (("bary_u", "u"), ("bary_v", "v"), ("t", "t")):
            assert (_bits(got[a][hit]) == _bits(rec[b][hit])).all(), a
        assert (init["instance_id"][~traced] == -1).all() and (sec["instance_id"] == init["instance_id"]).all()
        s2, ids = sec[traced][hit], rec["instance_id"][hit]
        hits += int(hit.sum())
        n_s = s2["flat_normal"].astype(f64)
        along = (n_s * face[ids]).sum(-1)
        assert (np.abs(np.abs(along) - 1) < 1e-6).all()
        assert ((n_s * rec["dir"][hit].astype(f64)).sum(-1) < 0).all(), "n_s faces away from the ray"
        off = np.abs(((s2["pos"].astype(f64) - quad[ids, 0]) * face[ids]).sum(-1))
        assert (off <= 8 * _ulp32(np.abs(s2["pos"]).max(-1))).all(), off.max()
        # the record's view is the ray, its position the ray's end
        want = surf["pos"][traced][hit].astype(f64) + rec["dir"][hit].astype(f64) * rec["t"][hit].astype(f64)[:, None]
        assert (np.abs(s2["pos"].astype(f64) - want) <= 1e-5 * (1 + np.abs(want))).all()
        assert (np.abs((s2["view"].astype(f64) * rec["dir"][hit].astype(f64)).sum(-1) - 1) < 1e-5).all()
    assert hits > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_the_light_sample_at_the_secondary_hit_is_restir_di_s(rooms, runs, case):
    """restir_di_model's sample_canonical and light_contribution on the recorded x_s record and the recorded draw give the recorded
    candidate bit for bit - class, index, light_data, pdf and the unshadowed contribution -, L_o follows from it and the recorded
    visibility, and the initial sample in the record is (x_s.pos, x_s.flat_normal, L_o) or null."""
    from tauray_amd import scene as S
    run = runs(case)
    scene, ss = rooms(run.size)
    L = _lights_of(S, scene, ss)
    classes = set()
    for f in run.frames:
        init, sec, light = f["initial"], f["secondary"], f["light"]
        hit = sec["instance_id"] >= 0
        s2, rec = sec[hit], light[hit]
        typ, idx, data, pdf = M.sample_canonical(L, init["light_draw"][hit], s2["pos"], run.options["min_ray_dist"], f32)
        assert ((rec["light"] >> 30) == typ).all() and ((rec["light"] & 0x3FFFFFFF) == idx).all()
        classes |= set(np.unique(typ).tolist())
        # an x_s in the plane of an emissive triangle has NaN light_data on both sides (the spherical triangle is degenerate; the
        # contribution of such a sample is 0): a NaN has no bits to compare, every other value is compared bit for bit
        nan = np.isnan(data)
        assert (np.isnan(rec["light_data"]) == nan).all() and (typ[nan.any(-1)] == 1).all() and not nan.all()
        assert (_bits(rec["light_data"])[~nan] == _bits(data)[~nan]).all() and (_bits(rec["pdf"]) == _bits(pdf)).all()
        contrib = M.light_contribution(L, typ, idx, data, s2, f32)[0]
        assert (_bits(rec["contribution"]) == _bits(contrib)).all()
        assert ((rec["visibility"] == 0) | (rec["visibility"] == 1)).all() and (rec["visibility"][~G.casts(contrib)] == 0).all()
        L_o = G.radiance(rec["contribution"], rec["visibility"], rec["pdf"], f32)
        assert (_bits(init["L_o"][hit]) == _bits(L_o)).all() and (init["L_o"][~hit] == 0).all()
        assert (light["light"][~hit] == M.NULL_INDEX).all() and (rec["weight"] == 0).all() and (rec["selected"] == 0).all()
    assert classes == {0, 1, 2, 3}, f"the light samples at the secondary hits cover the classes {classes}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_replay_of_the_decision_records_is_exact(runs, case):
    """From the decision records alone - samples, targets, pdfs, weights, draws, confidences - the float32 replay of update_reservoir, of
    the confidence sums and their clamp, of uc_weight and of the colour gives the canonical and the history reservoir buffers and `out`
    bit for bit: every pixel, three frames (frame 0 has no history)."""
    run = runs(case)
    o = run.options
    w, h = run.size
    reused = taken = 0
    for fi, f in enumerate(run.frames):
        for v in range(len(run.viewports)):
            surf, init, sec, temp = f["surface"][v], f["initial"][v], f["secondary"][v], f["temporal"][v]
            hit = surf["instance_id"] >= 0
            alive = G.casts(init["L_o"])
            sample = [np.where(alive[..., None], a, f32(0)) for a in (sec["pos"], sec["flat_normal"], init["L_o"])]
            zero3 = np.zeros((h, w, 3), dtype=f32)
            # the temporal kernel
            prev_conf = np.where(temp["reuse"] != 0, temp["prev_confidence"], f32(0)) if o["temporal_reuse"] else np.zeros((h, w), dtype=f32)
            assert (_bits(init["weight"][hit]) == _bits(G.initial_weight(init["target"], np.where(alive, init["pdf"], f32(1)), prev_conf, f32)[hit])).all()
            wsum, take = M.update_reservoir(np.zeros((h, w), dtype=f32), init["weight"], init["sel_draw"])
            assert (take == (init["selected"] != 0))[hit].all() and (take <= alive).all()
            taken += int(take[hit].sum())
            cur = [np.where(take[..., None], a, zero3) for a in sample]
            target = np.where(take, init["target"], f32(0))
            conf = np.ones((h, w), dtype=f32)
            ucw = M.uc_weight(wsum, target, f32)
            if o["temporal_reuse"]:
                reuse = temp["reuse"] != 0
                assert fi > 0 or not reuse.any()
                reused += int(reuse.sum())
                if reuse.any():
                    py, px = np.where(reuse, temp["py"], 0), np.where(reuse, temp["px"], 0)
                    pr = run.frames[fi - 1]["history"][v][py, px]
                    assert (_bits(temp["prev_confidence"][reuse]) == _bits(pr["confidence"][reuse])).all()
                    wsum2, take2 = M.update_reservoir(wsum, temp["weight"], temp["draw"])
                    take2 &= reuse
                    assert (take2 == ((temp["selected"] != 0) & reuse)).all()
                    wsum = np.where(reuse, wsum2, wsum)
                    cur = [np.where(take2[..., None], a, b) for a, b in zip(_sample_of(pr), cur)]
                    target = np.where(take2, temp["target"], target)
                    conf = np.where(reuse, conf + pr["confidence"], conf)
                    ucw = np.where(reuse, M.uc_weight(wsum, target, f32), ucw)
                conf = M.fmin2(conf, f32(o["max_confidence"]))
            can = f["canonical"][v]
            for name, got, want in (("uc_weight", can["uc_weight"], ucw), ("target_function", can["target_function"], target), ("confidence", can["confidence"], conf),
                                    ("x_s", can["x_s"], cur[0]), ("n_s", can["n_s"], cur[1]), ("L_o", can["L_o"], cur[2])):
                assert (_bits(got[hit]) == _bits(np.asarray(want, dtype=f32)[hit])).all(), (fi, v, name)
            # the spatial kernel
            fin, his = f["final"][v], f["history"][v]
            if o["spatial_samples"]:
                wsum = np.zeros((h, w), dtype=f32)
                target = np.zeros((h, w), dtype=f32)
                cur = [zero3, zero3, zero3]
                conf = np.zeros((h, w), dtype=f32)
                for k in range(o["spatial_samples"]):
                    r = f["spatial"][v][..., k]
                    held = (r["px"] >= 0) & hit
                    n = can[np.where(held, r["py"], 0), np.where(held, r["px"], 0)]
                    live = held & ~G.is_null(n["n_s"], n["L_o"])
                    wsum2, take = M.update_reservoir(wsum, r["wi"], r["draw"])
                    take &= live
                    assert (take == ((r["selected"] != 0) & live)).all()
                    wsum = np.where(live, wsum2, wsum)
                    cur = [np.where(take[..., None], a, b) for a, b in zip(_sample_of(n), cur)]
                    target = np.where(take, r["target_n"], target)
                    conf = np.where(held, conf + n["confidence"], conf)
                wsum, take = M.update_reservoir(wsum, fin["wi"], fin["draw"])
                assert (take == (fin["selected"] != 0))[hit].all()
                cur = [np.where(take[..., None], a, b) for a, b in zip(_sample_of(can), cur)]
                target = np.where(take, can["target_function"], target)
                conf = conf + can["confidence"]
                ucw = M.uc_weight(wsum, target, f32)
            else:
                cur, target, conf, ucw = list(_sample_of(can)), can["target_function"], can["confidence"], can["uc_weight"]
            for name, got, want in (("uc_weight", his["uc_weight"], ucw), ("target_function", his["target_function"], target), ("confidence", his["confidence"], conf),
                                    ("x_s", his["x_s"], cur[0]), ("n_s", his["n_s"], cur[1]), ("L_o", his["L_o"], cur[2])):
                assert (_bits(got[hit]) == _bits(np.asarray(want, dtype=f32)[hit])).all(), (fi, v, name)
            # out.rgb = in.rgb + (contribution * visibility) * uc_weight, out.a = in.a
            want = f["in"][v][..., :3] + (fin["contribution"] * fin["visibility"][..., None]) * his["uc_weight"][..., None]
            assert (_bits(f["color"][v][..., :3][hit]) == _bits(want.astype(f32)[hit])).all() and (_bits(f["color"][v][..., 3]) == _bits(f["in"][v][..., 3])).all()
    assert taken > 0
    if o["temporal_reuse"]:
        assert reused > 0, "no pixel of the static room reused its history"


def _model_frame(run, scene, fi, v, dt):
    """The model's own three passes of frame `fi`, viewport `v`, at `dt`: the inputs are the downloaded surface records, the recorded
    secondary hits and their L_o, the recorded visibilities, the previous frame's history and this frame's canonical reservoirs.  Flat
    arrays over the pixels with a surface (`ys`, `xs`)."""
    o, f = run.options, run.frames[fi]
    w, h = run.size
    surf = f["surface"][v]
    ys, xs = np.nonzero(surf["instance_id"] >= 0)
    s = surf[ys, xs]
    cam = scene.camera_data()[run.viewports[v]]
    origin = cam["origin"][:3]
    seed, vp = o["rng_seed"], run.viewports[v]
    out = dict(ys=ys, xs=xs)
    # ---- initial
    rs = M.pcg4d(G.sampler(xs, ys, vp, fi, G.PASS_INITIAL, seed))
    out["initial_draw"] = M.unit(rs, dt)[:, :2]
    out["dir"], out["pdf"], out["cast"] = G.initial_direction(M.unit(rs, dt)[:, :2], s, dt)
    out["light_draw"] = M.pcg4d(rs)
    init, sec = f["initial"][v][ys, xs], f["secondary"][v][ys, xs]
    alive = G.casts(init["L_o"])
    sx, sn, sL = (np.where(alive[:, None], a, f32(0)) for a in (sec["pos"], sec["flat_normal"], init["L_o"]))
    out["initial_target"] = M.luminance(G.contribution(sx, sn, sL, s, dt)[0], dt)
    # ---- temporal
    rs = G.sampler(xs, ys, vp, fi, G.PASS_TEMPORAL, seed)
    prev_conf = np.zeros(len(s), dtype=dt)
    reuse = np.zeros(len(s), dtype=bool)
    if o["temporal_reuse"]:
        rs = M.pcg4d(rs)
        rx, ry = M.reprojected_pixel(cam["view_proj"], s["pos"], run.size, M.unit(rs, dt)[:, :2], dt)
        on = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
        if fi:
            ps = run.frames[fi - 1]["surface"][v][np.where(on, ry, 0), np.where(on, rx, 0)]
            reuse = on & ~M.temporal_rejects(s, ps, origin, dt)
            ph = run.frames[fi - 1]["history"][v][np.where(on, ry, 0), np.where(on, rx, 0)]
            prev_conf = np.where(reuse, ph["confidence"], 0).astype(dt)
        out.update(rx=rx, ry=ry, reuse=reuse)
    rs = M.pcg4d(rs)
    out["sel_draw"] = M.unit(rs, dt)[:, 0]
    # the continuous quantities follow the STAGE's reuse decision and pixel (the discrete test compares those themselves)
    temp = f["temporal"][v][ys, xs]
    st_conf = np.where(temp["reuse"] != 0, temp["prev_confidence"], 0).astype(dt) if o["temporal_reuse"] else prev_conf
    out["initial_weight"] = G.initial_weight(init["target"].astype(dt), np.where(alive, init["pdf"], f32(1)).astype(dt), st_conf, dt)
    if o["temporal_reuse"] and fi:
        held = temp["reuse"] != 0
        sh = run.frames[fi - 1]["history"][v][np.where(held, temp["py"], 0), np.where(held, temp["px"], 0)]
        t = M.luminance(G.contribution(*_sample_of(sh), s, dt)[0], dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["temporal_target"] = t
            out["temporal_weight"] = M.nan_to_zero(((sh["confidence"].astype(dt) / (dt(1) + sh["confidence"].astype(dt))) * t) * sh["uc_weight"].astype(dt))
        rs = M.pcg4d(rs)
        out["temporal_draw"] = M.unit(rs, dt)[:, 0]
    # ---- spatial
    K = o["spatial_samples"]
    can = f["canonical"][v]
    c = can[ys, xs]
    if K:
        rs = G.sampler(xs, ys, vp, fi, G.PASS_SPATIAL, seed)
        offs = []
        for _ in range(2 * K):
            rs = M.pcg4d(rs)
            offs.append(M.neighbour_offsets(M.unit(rs, dt)[:, :2], o["search_radius"], dt))
        offs = np.stack(offs, 1)
        inv = M.inv_max_plane_dist(cam["proj_inverse"], cam["view_inverse"], s["pos"], dt)
        nx, ny = xs[:, None] + offs[..., 0], ys[:, None] + offs[..., 1]
        on = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
        ns = surf[np.where(on, ny, 0), np.where(on, nx, 0)]
        good = np.stack([M.neighbour_is_good(s, ns["pos"][:, k], ns["flat_normal"][:, k], inv, dt) for k in range(2 * K)], 1)
        sid = surf["instance_id"]
        slots = np.zeros((len(s), K, 3), dtype=np.int64)
        for p in range(len(s)):
            g = {(int(nx[p, k]), int(ny[p, k])): bool(good[p, k]) for k in range(2 * K) if on[p, k]}
            got = M.pick_neighbours(int(xs[p]), int(ys[p]), offs[p], run.size, sid, lambda x, y: g[(x, y)], K)
            slots[p] = [(x, y, int(gd)) for x, y, gd in got]
        out["slots"] = slots
        srec = f["spatial"][v][ys, xs]
        held = srec["px"] >= 0
        nres = can[np.where(held, srec["py"], 0), np.where(held, srec["px"], 0)]
        live = held & ~G.is_null(nres["n_s"], nres["L_o"])
        c_live = ~G.is_null(c["n_s"], c["L_o"])
        draws = []
        for k in range(K):
            rs = np.where(live[:, k, None], M.pcg4d(rs), rs)
            draws.append(M.unit(rs, dt)[:, 0])
        rs = M.pcg4d(rs)
        out.update(spatial_live=live, spatial_draw=np.stack(draws, 1), final_draw=M.unit(rs, dt)[:, 0])
        neighbours = []
        for k in range(K):
            n = nres[:, k]
            nsurf = surf[np.where(held[:, k], srec["py"][:, k], 0), np.where(held[:, k], srec["px"][:, k], 0)]
            tn = M.luminance(G.contribution(*_sample_of(n), s, dt)[0] * srec["visibility_n"][:, k].astype(dt)[:, None], dt)
            tc = M.luminance(G.contribution(*_sample_of(c), nsurf, dt)[0] * srec["visibility_c"][:, k].astype(dt)[:, None], dt)
            jn = M.jacobian(nsurf["pos"].astype(dt), s["pos"].astype(dt), n["x_s"].astype(dt), n["n_s"].astype(dt), dt)
            jc = M.jacobian(s["pos"].astype(dt), nsurf["pos"].astype(dt), c["x_s"].astype(dt), c["n_s"].astype(dt), dt)
            neighbours.append(dict(target_function=n["target_function"], uc_weight=n["uc_weight"], confidence=n["confidence"], target_n=tn, jacobian_n=jn, target_c=tc,
                                   jacobian_c=jc, held=held[:, k], live=live[:, k], canonical_live=held[:, k] & c_live))
        sm = G.spatial_merge((c["target_function"], c["uc_weight"], c["confidence"]), neighbours, [srec["draw"][:, k].astype(dt) for k in range(K)],
                             f["final"][v][ys, xs]["draw"].astype(dt), dt)
        for key, field, mask in (("target_n", "target_n", "live"), ("jacobian_n", "jacobian_n", "live"), ("target_c", "target_c", "canonical_live"),
                                 ("jacobian_c", "jacobian_c", "canonical_live")):
            out[key] = np.stack([np.where(n[mask], n[field], dt(0)) for n in neighbours], 1)
        for key in ("m", "wi", "mis_canonical"):
            out[key] = np.stack(sm[key], 1)
        out["canonical_m"], out["final_wi"] = sm["canonical_m"], sm["final_wi"]
    his = f["history"][v][ys, xs]
    out["final_contribution"] = G.contribution(*_sample_of(his), s, dt)[0]
    return out


@pytest.fixture(scope="module")
def modelled(runs, rooms):
    """The model's frames of a run at both precisions, computed once."""
    cache = {}

    def get(case):
        if case not in cache:
            run = runs(case)
            scene, ss = rooms(run.size)
            cache[case] = {(fi, v): (_model_frame(run, scene, fi, v, f32), _model_frame(run, scene, fi, v, f64))
                           for fi in range(len(run.frames)) for v in range(len(run.viewports))}
        return cache[case]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_draws_directions_and_pdfs_are_exact(runs, modelled, case):
    """The model's own pcg4d streams give every recorded draw - the direction's, the light sample's four words, the initial selection's,
    the temporal merge's and, in the spatial stream, after its 2 * spatial_samples offsets, one per slot that holds a neighbour whose sample
    is not null and one for the canonical merge -, and its float32 gives the recorded direction, pdf and cast bit, bit for bit."""
    run = runs(case)
    for (fi, v), (m32, m64) in modelled(case).items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        init = f["initial"][v][ys, xs]
        assert (_bits(init["draw"]) == _bits(m32["initial_draw"])).all()
        assert (_bits(init["dir"]) == _bits(m32["dir"])).all() and (_bits(init["pdf"]) == _bits(m32["pdf"])).all() and ((init["traced"] != 0) == m32["cast"]).all()
        hit2 = init["instance_id"] >= 0
        assert hit2.any() and (init["light_draw"][hit2] == m32["light_draw"][hit2]).all() and (init["light_draw"][~hit2] == 0).all()
        assert (_bits(init["sel_draw"]) == _bits(m32["sel_draw"])).all()
        if "temporal_draw" in m32:
            reuse = f["temporal"][v][ys, xs]["reuse"] != 0
            assert (_bits(f["temporal"][v][ys, xs]["draw"][reuse]) == _bits(m32["temporal_draw"][reuse])).all()
        if "spatial_draw" in m32:
            srec, live = f["spatial"][v][ys, xs], m32["spatial_live"]
            assert live.any() and (_bits(srec["draw"][live]) == _bits(m32["spatial_draw"][live])).all() and (_bits(srec["draw"][~live]) == 0).all()
            assert (_bits(f["final"][v][ys, xs]["draw"]) == _bits(m32["final_draw"])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_continuous_quantities_are_bounded(runs, modelled, case, capsys):
    """Targets, weights, Jacobians, MIS terms and the final contribution, recomputed by the model from the downloaded surface records,
    reservoirs and recorded visibilities: |stage - model64| <= 4 |model32 - model64| + 1 ulp (DI's bound)."""
    run = runs(case)
    failures, worst = [], {}
    for (fi, v), (m32, m64) in modelled(case).items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        every = np.ones(len(ys), dtype=bool)
        init = f["initial"][v][ys, xs]
        checks = [("initial target", init["target"], m32["initial_target"], m64["initial_target"], every),
                  ("initial weight", init["weight"], m32["initial_weight"], m64["initial_weight"], every)]
        temp = f["temporal"][v][ys, xs]
        if "temporal_weight" in m32:
            same = temp["reuse"] != 0
            checks += [("temporal target", temp["target"], m32["temporal_target"], m64["temporal_target"], same),
                       ("temporal weight", temp["weight"], m32["temporal_weight"], m64["temporal_weight"], same)]
        if run.options["spatial_samples"]:
            srec, fin = f["spatial"][v][ys, xs], f["final"][v][ys, xs]
            for k in ("target_n", "jacobian_n", "m", "wi", "target_c", "jacobian_c", "mis_canonical"):
                checks.append(("spatial " + k, srec[k], m32[k], m64[k], every))
            checks += [("canonical_m", fin["canonical_m"], m32["canonical_m"], m64["canonical_m"], every), ("final wi", fin["wi"], m32["final_wi"], m64["final_wi"], every)]
        checks.append(("final contribution", f["final"][v][ys, xs]["contribution"], m32["final_contribution"], m64["final_contribution"], every))
        for name, got, a, b, keep in checks:
            worst[name] = max(worst.get(name, 0.0), _bounded(f"frame {fi} viewport {v} {name}", got, a, b, keep, failures))
    with capsys.disabled():
        print(f"\nrestir gi case {case}: largest error / bound: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_discrete_decisions_match_where_the_precisions_agree(runs, modelled, case, capsys):
    """Neighbour pixels, good / bad bits, the reprojected pixel and its reuse bit: a pixel where the model's own float32 and float64
    disagree on any of them is left out, at most 1 % of a frame may be; on every other pixel the stage's decisions are the model's."""
    run = runs(case)
    counts = []
    for (fi, v), (m32, m64) in modelled(case).items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        out = np.zeros(len(ys), dtype=bool)
        if "rx" in m32:
            out |= (m32["rx"] != m64["rx"]) | (m32["ry"] != m64["ry"]) | (m32["reuse"] != m64["reuse"])
        if "slots" in m32:
            out |= (m32["slots"] != m64["slots"]).any((1, 2))
        counts.append(int(out.sum()))
        assert out.sum() <= 0.01 * run.size[0] * run.size[1], f"frame {fi} viewport {v}: {out.sum()} pixels left out"
        keep = ~out
        if "rx" in m32:
            temp = f["temporal"][v][ys, xs]
            assert (temp["px"][keep] == m32["rx"][keep]).all() and (temp["py"][keep] == m32["ry"][keep]).all()
            assert ((temp["reuse"] != 0)[keep] == m32["reuse"][keep]).all()
        if "slots" in m32:
            srec = f["spatial"][v][ys, xs]
            got = np.stack([srec["px"], srec["py"], np.where(srec["px"] >= 0, srec["good"].astype(np.int64), 0)], -1).astype(np.int64)
            assert (got[keep] == m32["slots"][keep]).all()
    with capsys.disabled():
        print(f"\nrestir gi case {case}: pixels left out of the discrete comparison per frame and viewport: {counts}")


@pytest.mark.gpu
def test_a_changed_viewport_list_is_refused_while_there_is_history(R, ctx, rooms):
    size = SIZES[0]
    scene, ss = rooms(size)
    out = ctx.alloc(size[0] * size[1] * 16 * 2).zero()
    for temporal in (True, False):
        st = R.RestirGiStage(ctx, ss, size, 2, R.restir_gi_options(spatial_samples=0, temporal_reuse=temporal))
        st.run((0, 1), None, out)
        if temporal:
            for other in ((1, 0), (0,)):
                with pytest.raises(R.TrhipError) as e:
                    st.run(other, None, out)
                assert "trhip_restir_gi_render" in str(e.value) and "viewport list differs" in str(e.value)
            st.run((0, 1), None, out)
            st.reset()
        st.run((1, 0), None, out)
        with pytest.raises(R.TrhipError) as e:
            st.run((0, 7), None, out)
        assert "viewport 7 out of range" in str(e.value)
        st.close()
    out.free()


def _frames(R, ctx, ss, size, viewports, frames, stage=None, **options):
    st = stage or R.RestirGiStage(ctx, ss, size, len(viewports), R.restir_gi_options(**options))
    out = ctx.alloc(size[0] * size[1] * 16 * len(viewports)).zero()
    imgs = []
    for _ in range(frames):
        st.run(viewports, None, out)
        imgs.append(out.download((len(viewports), size[1], size[0], 4)))
    out.free()
    if stage is None:
        hist = st.download("history")
        st.close()
        return np.stack(imgs), hist
    return np.stack(imgs)


@pytest.mark.gpu
def test_layouts_runs_reset_and_viewport_split_give_the_same_bits(R, ctx, rooms):
    size = (37, 19)
    opts = dict(spatial_samples=3, temporal_reuse=True, search_radius=6.0, rng_seed=5)
    scene, ss = rooms(size)
    a, ha = _frames(R, ctx, ss, size, [0, 1], 3, **opts)
    b, hb = _frames(R, ctx, ss, size, [0, 1], 3, **opts)
    assert (_bits(a) == _bits(b)).all() and ha.tobytes() == hb.tobytes(), "two fresh runs differ"
    assert not (_bits(a[0]) == _bits(a[1])).all(), "the frames of a sequence draw the same numbers"
    st = R.RestirGiStage(ctx, ss, size, 2, R.restir_gi_options(**opts))
    c = _frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    st.reset()
    d = _frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    st.close()
    assert (_bits(c) == _bits(a[:2])).all() and (_bits(d) == _bits(a[:2])).all(), "reset does not forget the history"
    for v in (0, 1):
        e, _ = _frames(R, ctx, ss, size, [v], 3, **opts)
        assert (_bits(e[:, 0]) == _bits(a[:, v])).all(), f"viewport {v} alone differs"
    for strategy in (1, 2):
        scene, ss2 = rooms(size, as_strategy=strategy)
        g, hg = _frames(R, ctx, ss2, size, [0, 1], 3, **opts)
        assert (_bits(g) == _bits(a)).all() and hg.tobytes() == ha.tobytes(), f"acceleration-structure strategy {strategy} differs"
    rooms(size, as_strategy=0)


@pytest.mark.gpu
def test_a_list_longer_than_one_launch(R):
    """65 viewports are two launches a pass, of 64 and of 1: layer 64 is layer 0 of a one-entry list of its viewport and layer 63 repeats
    layer 0, bit for bit - colour, surface record, canonical and history reservoirs.  17 x 9 pixels leave the tile partial on both axes."""
    from tauray_amd import scene as S
    size = (17, 9)
    own = R.Context(0)      # the module's context holds the scene of `rooms`
    ss = R.SceneStage(own, _room(S, size), as_strategy=0)

    def frame(views):
        st = R.RestirGiStage(own, ss, size, len(views), R.restir_gi_options(spatial_samples=2, temporal_reuse=False, search_radius=4.0, rng_seed=3))
        out = own.alloc(size[0] * size[1] * 16 * len(views)).zero()
        st.run(views, None, out)
        own.sync()
        got = [out.download((len(views), size[1], size[0], 4))] + [st.download(n) for n in ("surface", "canonical", "history")]
        out.free()
        st.close()
        return got

    many, one = frame([0] * 64 + [1]), frame([1])
    assert (many[1]["instance_id"][0] >= 0).any() and many[0][0][..., :3].max() > 0
    for a, b in zip(many, one):
        assert a[64].tobytes() == b[0].tobytes() and a[63].tobytes() == a[0].tobytes()
    assert many[0][64].tobytes() != many[0][0].tobytes(), "the two viewports see the same"
    own.close()


@pytest.mark.gpu
def test_no_draw_is_shared_with_restir_di(R, ctx, rooms):
    """DI and GI run with the same seed in the same frames: no recorded draw of one equals a draw of the other at the same pixel, and the
    sampler states behind them (the model's, which the draw tests hold equal to the stages') differ in every one of the five streams."""
    size = (37, 19)
    scene, ss = rooms(size)
    seed = 19
    gi = _Run(R, ctx, ss, size, frames=3, spatial_samples=3, temporal_reuse=True, search_radius=4.0, rng_seed=seed)
    di = R.RestirDiStage(ctx, ss, size, 2, R.restir_di_options(candidates=4, spatial_samples=3, temporal_reuse=True, search_radius=4.0, rng_seed=seed, record=True))
    sink = ctx.alloc(size[0] * size[1] * 16 * 2).zero()
    compared = 0
    for fi, f in enumerate(gi.frames):
        di.run((0, 1), sink)
        d = {n: di.download(n) for n in ("candidates", "temporal", "spatial", "final")}
        hit = f["surface"]["instance_id"] >= 0
        unit = f["initial"]["light_draw"].astype(f32) * f32(2.3283064365386963e-10)
        mine = np.concatenate([f["initial"]["draw"], f["initial"]["sel_draw"][..., None], f["temporal"]["draw"][..., None], f["spatial"]["draw"], f["final"]["draw"][..., None],
                               unit], -1)[hit]
        theirs = np.concatenate([d["candidates"]["draw"], d["temporal"]["draw"][..., None], d["spatial"]["draw"], d["final"]["draw"][..., None]], -1)[hit]
        same = (mine[:, :, None] == theirs[:, None, :]) & (mine[:, :, None] != 0)
        compared += int((mine != 0).sum())
        assert not same.any(), f"frame {fi}: {int(same.sum())} draws of ReSTIR GI are draws of ReSTIR DI at the same pixel"
        ys, xs = np.nonzero(hit[0])
        for fj in range(len(gi.frames)):
            states = [M.init_sampler(xs, ys, 0, G.di_sampler_w(fj, p), seed) for p in (0, 1)]
            for p in (G.PASS_INITIAL, G.PASS_TEMPORAL, G.PASS_SPATIAL):
                own = G.sampler(xs, ys, 0, fi, p, seed)
                assert all((own != other).any(-1).all() for other in states)
    assert compared > 1000
    di.close()
    sink.free()
    assert len({G.gi_sampler_w(f, p) for f in range(1 << 10) for p in range(3)} & {G.di_sampler_w(f, p) for f in range(1 << 12) for p in range(2)}) == 0


def _indirect_reference(R, ctx, ss, scene, size, K, spp):
    """K batches of the one-bounce indirect light of the room: the path tracer at the depth that adds exactly one bounce of reflected light
    to the direct stage (cosine-hemisphere bounces), minus the direct stage.  That depth is 3: the path tracer at 2 is held equal to the
    direct stage first.  The pixels that see the emissive quad directly are left out of every image (set to 0) - there the path tracer
    counts a visible dielectric emitter's emission twice (the reference's behaviour; measured here as exactly one
    more (3, 2, 1) over those pixels), which is neither direct nor indirect light.  Returns the batches and the mask of the kept pixels."""
    from test_estimator_consistency import _assert_same_mean, _batches, _dup
    st = R.RestirGiStage(ctx, ss, size, 1, R.restir_gi_options(spatial_samples=0, temporal_reuse=False))
    sink = ctx.alloc(size[0] * size[1] * 16).zero()
    st.run([0], None, sink)
    keep = ~(st.download("surface")[0]["emission"] > 0).any(-1)
    st.close()
    sink.free()
    assert keep.mean() > 0.95 and not keep.all()
    keep = keep[None, :, :, None]
    direct = R.DirectStage(ctx, ss, R.options_for_scene(scene, samples_per_pixel=spp, samples_per_pass=1), _dup(size))
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    base = np.zeros((K, size[1], size[0], 3))
    for k in range(K):
        direct.reset_accumulated_samples()
        direct.run(buf)
        base[k] = buf.download((size[1], size[0], 4))[..., :3]
    direct.close()
    buf.free()
    shallow = _batches(R, ctx, ss, scene, size, K, spp, max_bounces=2, bounce_mode=1)
    _assert_same_mean(base * keep, shallow * keep, "the path tracer at depth 2 against the direct stage")
    deep = _batches(R, ctx, ss, scene, size, K, spp, max_bounces=3, bounce_mode=1)
    return (deep - base) * keep, keep


EXPECTATION_CASES = {
    "no reuse": (dict(spatial_samples=0, temporal_reuse=False), 1, 96),
    "temporal reuse, frame 8": (dict(spatial_samples=0, temporal_reuse=True), 9, 24),
    "2 spatial samples at radius 8": (dict(spatial_samples=2, temporal_reuse=False, search_radius=8.0), 1, 48),
    "temporal reuse, 3 spatial samples, frame 8": (dict(spatial_samples=3, temporal_reuse=True, search_radius=8.0), 9, 24),
}


@pytest.fixture(scope="module")
def indirect_reference(R, ctx, rooms):
    cache = {}

    def get():
        if not cache:
            scene, ss = rooms((64, 64))
            cache["ref"] = _indirect_reference(R, ctx, ss, scene, (64, 64), 16, 256)
        return cache["ref"]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXPECTATION_CASES))
def test_same_expectation_as_one_bounce_of_the_path_tracer(R, ctx, rooms, indirect_reference, name, capsys):
    """The room at 64 x 64, `in` = null, K = 16 independent batches, judged by test_estimator_consistency's _assert_same_mean as it is:
    ReSTIR GI against the path tracer's one-bounce indirect light (_indirect_reference).  The configurations without spatial reuse are
    unbiased.  With spatial reuse a neighbour's sample keeps the L_o it sent towards the pixel that found it (limit 1 of restir_gi.h), a
    bias on glossy secondary surfaces: measured on an MI355X in this room the image means differ by -0.16 / -0.36 / -0.45 % (r / g / b;
    2 spatial samples at radius 8) and -0.52 / -0.69 / -0.64 % (temporal reuse with 3 spatial samples, frame 8) with standard errors of
    0.4 ... 0.6 % - inside what _assert_same_mean allows, so all four configurations are held to it as it is."""
    from test_estimator_consistency import _assert_same_mean
    size, K = (64, 64), 16
    scene, ss = rooms(size)
    options, frames, seeds = EXPECTATION_CASES[name]
    base, keep = indirect_reference()
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    got = np.zeros((K, size[1], size[0], 3))
    seed = 1
    for k in range(K):
        for _ in range(seeds):
            st = R.RestirGiStage(ctx, ss, size, 1, R.restir_gi_options(rng_seed=seed, **options))
            seed += 1
            for _f in range(frames):
                st.run([0], None, buf)
            got[k] += buf.download((size[1], size[0], 4))[..., :3] / seeds
            st.close()
    buf.free()
    assert np.isfinite(got).all()
    got = got * keep
    ma, mb = base.mean((1, 2)), got.mean((1, 2))
    rel = (mb.mean(0) - ma.mean(0)) / ma.mean(0)
    se = np.sqrt(ma.var(0, ddof=1) / K + mb.var(0, ddof=1) / K) / ma.mean(0)
    with capsys.disabled():
        print(f"\nrestir gi against one bounce of the path tracer, {name}: image means differ by {np.array2string(rel, precision=4)} relative "
              f"(standard error of the difference {np.array2string(se, precision=4)}); indirect mean {ma.mean(0)}")
    assert (se < 0.0125).all(), "the batches are too noisy to say anything"
    _assert_same_mean(base, got, name)


@pytest.mark.gpu
def test_the_feature_earns_its_keep(R, ctx, capsys):
    """sponza_lights with 64 lights at 128 x 72, static camera: the mean squared error of frame 8 with the defaults (2 spatial samples,
    temporal reuse) against the converged indirect light is strictly lower than that of the same stage with spatial_samples = 0 and
    temporal_reuse off, both averaged over the same 8 seeds.  The converged image is the mean of 2048 frames of the stage without reuse,
    each with a seed of its own (1001 ...): the unbiased configuration, which the room test holds to the path tracer's expectation.  The
    path tracer itself is no reference in this scene: it sees the sphere lights as spheres (the stage lights with points, limit 5), and
    at depth 2 and 3 with cosine-hemisphere bounces it leaves non-finite pixels here (measured: 6 690 of 9 216 at 256 spp)."""
    from tauray_amd import scenes
    size = (128, 72)
    scene = scenes.sponza_lights(64, 1, *size)
    ss = R.SceneStage(ctx, scene)
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    mrd = scene_min_ray_dist(R, scene)
    ref = np.zeros((size[1], size[0], 3))
    N = 2048
    for seed in range(1001, 1001 + N):
        st = R.RestirGiStage(ctx, ss, size, 1, R.restir_gi_options(rng_seed=seed, min_ray_dist=mrd, spatial_samples=0, temporal_reuse=False))
        st.run([0], None, buf)
        ref += buf.download((size[1], size[0], 4))[..., :3].astype(f64) / N
        st.close()
    assert np.isfinite(ref).all() and ref.mean() > 0
    mse = {"defaults": 0.0, "no reuse": 0.0}
    for seed in range(1, 9):
        for name, options, frames in (("defaults", {}, 9), ("no reuse", dict(spatial_samples=0, temporal_reuse=False), 1)):
            st = R.RestirGiStage(ctx, ss, size, 1, R.restir_gi_options(rng_seed=seed, min_ray_dist=mrd, **options))
            for _ in range(frames):
                st.run([0], None, buf)
            img = buf.download((size[1], size[0], 4))[..., :3].astype(f64)
            st.close()
            mse[name] += np.mean((img - ref) ** 2) / 8
    buf.free()
    with capsys.disabled():
        print(f"\nrestir gi on {scene.name} at {size[0]} x {size[1]}: MSE against the converged indirect light: frame 8 of the defaults {mse['defaults']:.4e}, "
              f"no reuse {mse['no reuse']:.4e}, ratio {mse['defaults'] / mse['no reuse']:.3f}")
    assert mse["defaults"] < mse["no reuse"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["still", "camera grid", "animation"])
def test_both_hosts_render_the_same_frames(R, ctx, tmp_path, which):
    """tauray_hip --renderer=restir-gi against the Python RestirGiRenderer: three frames at 96 x 96 as .raw, bit for bit - test.glb, the
    same under a 2 x 1 camera grid, and animated.glb under --animation; -t names the five kernels."""
    from tauray_amd import scene as S
    from tauray_amd.gltf import load_glb
    from tauray_amd.animation import SceneAnimator
    size, frames = (96, 96), 3
    glb = os.path.join(GOLDEN, "animated.glb" if which == "animation" else "test.glb")
    prefix = str(tmp_path / "cpp")
    args = [CLI, glb, "--renderer=restir-gi", "--restir-gi=2,16,8,on", "--restir=2,1,16,16,on", f"--width={size[0]}", f"--height={size[1]}", f"--frames={frames}",
            "--filetype=raw", "--format=rgba32", "--rng-seed=3", "-t", "--headless=" + prefix]
    if which == "camera grid":
        args.append("--camera-grid=2,1,0.1,0.1")
    if which == "animation":
        args.append("--animation")
    p = subprocess.run(args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    for kernel in ("restir di canonical", "restir di spatial", "restir gi initial", "restir gi temporal", "restir gi spatial"):
        assert f"[{kernel}]" in p.stdout
    scene = load_glb(glb, *size)
    if which == "camera grid":
        scene.cameras = S.generate_camera_grid(scene.cameras[0], 2, 1, 0.1, 0.1, 5.0)
    views = max(len(scene.cameras), 1)
    ss = R.SceneStage(ctx, scene)
    animator = None
    if which == "animation":
        animator = SceneAnimator(scene)
        animator.play("")
    mrd = scene_min_ray_dist(R, scene)
    rr = R.RestirGiRenderer(ctx, ss, scene, size, R.restir_gi_options(spatial_samples=2, search_radius=16.0, max_confidence=8.0, temporal_reuse=True, rng_seed=3, min_ray_dist=mrd),
                            R.restir_di_options(candidates=2, spatial_samples=1, search_radius=16.0, max_confidence=16.0, temporal_reuse=True, rng_seed=3, min_ray_dist=mrd))
    shown = []
    for f in range(frames):
        if animator:
            ss.animate(animator, 0 if f == 0 else round(1000000.0 / 60.0), refit=(f % 3 != 2))
        rr.render()
        img = rr.download("display")
        assert np.isfinite(img).all() and img[..., :3].max() > 0
        shown.append(img)
        for v in range(views):
            got = _raw(f"{prefix}{str(v) + '_' if views > 1 else ''}{f}.raw", (size[1], size[0], 4))
            differing = int((_bits(got) != _bits(img[v])).any(-1).sum())
            assert differing == 0, f"{which}, frame {f}, view {v}: {differing} of {size[0] * size[1]} pixels differ"
    assert (shown[0] != shown[1]).any()
    t = rr.timings()
    assert t["indirect"]["initial_name"] == "restir gi initial" and t["indirect"]["frames"] == frames and t["indirect"]["total_ms"] > 0
    assert t["direct"]["canonical_name"] == "restir di canonical" and t["direct"]["frames"] == frames
    rr.close()
