"""ReSTIR DI's power-proportional light selection (trhip_restir_di_set_light_selection, --restir-light-selection; `light selection` of
tauray_amd/csrc/restir_di.h): a point or triangle light candidate drawn through an alias table over the lights'
weights, with the share `uniform_fraction` of the pdf uniform.

CPU: the ABI, the refusals of the setter, of the Python option and of the command line, the model's table, draw and estimator
(tests/restir_di_selection_model.py on top of tests/restir_di_model.py), and the library's host builder against the model byte for byte
under the host sanitizers (tests/restir_light_selection_check.cc).  GPU: the room of tests/test_restir_di.py with 37 more point lights
whose powers span three decades (one of them black) and an emissive fan of 61 triangles whose areas span two: the uniform mode untouched
(G1), weights and table against the model (G2), the replay and the model of every candidate (G3), the frequencies (G4), the direct
stage's expectation (G5, G6: also under a stale table), the quality (G7), refusals and determinism (G8), both hosts (G9).  Helpers and
criteria are tests/test_restir_di.py's and tests/test_restir_di_visibility.py's."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import restir_di_model as M
import restir_di_selection_model as SM
import test_restir_di as T
import test_restir_di_visibility as V
from conftest import GOLDEN, ROOT
from test_restir_di import _bits, _light_split, _lights_of

f32, f64 = np.float32, np.float64
SIZES = T.SIZES
CLI = T.CLI
EXISTING = V.EXISTING + ("sampled",)
VISIBILITIES = V.MODE_NAMES


@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


# =========================================================================================================================== CPU
def test_symbols_resolve_and_the_header_agrees(tmp_path):
    from tauray_amd import _lib
    L = _lib.lib()
    for name in ("trhip_restir_di_set_light_selection", "trhip_restir_di_refresh_light_selection"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    src = tmp_path / "defines.c"
    src.write_text('#include <stdio.h>\n#include "trhip.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %zu\\n", TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM, TRHIP_RESTIR_LIGHT_SELECTION_POWER, TRHIP_RESTIR_DI_LIGHT_WEIGHTS,\n'
                   "           TRHIP_RESTIR_DI_LIGHT_TABLE, sizeof(trhip_restir_di_options));\n    return 0;\n}\n")
    exe = str(tmp_path / "defines")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [0, 1, 8, 9, 32]
    assert C.sizeof(_lib.RestirDiOptionsC) == 32 and np.dtype(_lib.RESTIR_DI_LIGHT_TABLE_DTYPE).itemsize == 16 == SM.ENTRY.itemsize
    assert (_lib.RESTIR_DI_LIGHT_WEIGHTS, _lib.RESTIR_DI_LIGHT_TABLE) == (8, 9) and _lib.RESTIR_LIGHT_SELECTION == {"uniform": 0, "power": 1} == SM.MODES


def test_the_entry_points_refuse_a_null_stage():
    from tauray_amd import _lib
    from tauray_amd import renderer as R
    for mode, fraction in ((0, 0.1), (1, 0.1), (5, 0.1), (1, 2.0)):
        assert _lib.lib().trhip_restir_di_set_light_selection(None, mode, fraction) != 0
        with pytest.raises(R.TrhipError) as e:
            R.check(1)
        assert "trhip_restir_di_set_light_selection: null stage" in str(e.value)
    rebuilt = C.c_uint32(7)
    assert _lib.lib().trhip_restir_di_refresh_light_selection(None, C.byref(rebuilt)) != 0 and rebuilt.value == 0
    with pytest.raises(R.TrhipError) as e:
        R.check(1)
    assert "trhip_restir_di_refresh_light_selection: null stage" in str(e.value)
    assert _lib.lib().trhip_restir_di_refresh_light_selection(None, None) != 0


def test_python_option_refuses_by_name(R):
    o = R.restir_di_options()
    assert o["light_selection"] == "uniform" and o["uniform_fraction"] == 0.1
    for name in ("uniform", "power"):
        for f in (0.05, 0.1, 1.0, 1e-6):
            o = R.restir_di_options(light_selection=name, uniform_fraction=f)
            assert (o["light_selection"], o["uniform_fraction"]) == (name, f)
    for bad in ("maybe", "", "Power", 1, None):
        with pytest.raises(ValueError) as e:
            R.restir_di_options(light_selection=bad)
        assert "light selection" in str(e.value)
    for name in ("uniform", "power"):      # the fraction is checked for uniform too
        for bad in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
            with pytest.raises(ValueError) as e:
                R.restir_di_options(light_selection=name, uniform_fraction=bad)
            assert "uniform_fraction" in str(e.value) and "(0, 1]" in str(e.value)
    with pytest.raises(ValueError):      # the stage refuses the name before anything is created
        R.RestirDiStage(None, None, (16, 16), 1, dict(light_selection="maybe"))
    with pytest.raises(ValueError):
        R.RestirDiStage(None, None, (16, 16), 1, dict(light_selection="power", uniform_fraction=0.0))
    assert hasattr(R.RestirDiStage, "refresh_light_selection") and hasattr(R.RestirDiStage, "set_light_selection")


@pytest.mark.parametrize("args, text", [
    (["--renderer=restir-di", "--restir-light-selection=maybe"], "--restir-light-selection: maybe is neither uniform nor power"),
    (["--renderer=restir-gi", "--restir-light-selection="], "--restir-light-selection:  is neither uniform nor power"),
    (["--renderer=restir-di", "--restir-light-selection=Power,0.1"], "--restir-light-selection: Power is neither uniform nor power"),
    (["--renderer=restir-di", "--restir-light-selection=power,0"], "--restir-light-selection: the uniform fraction 0 is not a number in (0, 1]"),
    (["--renderer=restir-di", "--restir-light-selection=power,1.5"], "--restir-light-selection: the uniform fraction 1.5 is not a number in (0, 1]"),
    (["--renderer=restir-di", "--restir-light-selection=uniform,-0.1"], "--restir-light-selection: the uniform fraction -0.1 is not a number in (0, 1]"),
    (["--renderer=restir-gi", "--restir-light-selection=power,"], "--restir-light-selection: the uniform fraction  is not a number in (0, 1]"),
    (["--renderer=restir-di", "--restir-light-selection=power,0.1x"], "--restir-light-selection: the uniform fraction 0.1x is not a number in (0, 1]"),
    (["--renderer=restir-di", "--restir-light-selection=power,nan"], "--restir-light-selection: the uniform fraction nan is not a number in (0, 1]"),
    (["--restir-light-selection=power"], "--restir-light-selection sets the light selection of --renderer=restir-di"),
    (["--renderer=dshgi", "--restir-light-selection=power,0.1"], "--restir-light-selection sets the light selection of --renderer=restir-di"),
])
def test_cli_refuses(args, text):
    p = subprocess.run([CLI] + args + [os.path.join(GOLDEN, "test.glb"), "--width=16", "--height=16", "--filetype=none"], capture_output=True, text=True)
    assert p.returncode != 0 and text in p.stderr, p.stderr
    assert "--restir-light-selection=uniform|power[,fraction]" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout


def _edge_vectors():
    """Weight vectors of length 1, 2, 3 and 67: all zero, all equal, one zero among non-zeros, one light with 0.999 of the power, and
    NaN, inf and negatives among ordinary weights."""
    rng = np.random.default_rng(33)
    out = []
    for n in (1, 2, 3, 67):
        base = rng.uniform(0.05, 4.0, n).astype(f32)
        out += [("all zero", np.zeros(n, dtype=f32)), ("all equal", np.full(n, 0.7, dtype=f32)), ("random", base)]
        if n > 1:
            z = base.copy()
            z[n // 2] = 0
            out.append(("one zero", z))
            h = base.copy()
            h[n // 3] = f32(999.0 * (base.sum(dtype=f64) - base[n // 3]))
            out.append(("one holds 0.999", h))
            bad = base.copy()
            bad[0], bad[-1] = np.nan, -2.0
            if n > 2:
                bad[1] = np.inf
            out.append(("nan, inf, negative", bad))
    return out


def test_model_table():
    """Every alias is a slot of the table; the probabilities the draw realises - exactly, from the thresholds and the aliases - are p_i to
    2^-30 (ten times the threshold's granularity of 2^-32; the builder's steps are doubles, so nothing else comes near it); pdf and
    alias_pdf are float32(p_i) exactly; a zero-weight light has f / n."""
    worst = 0.0
    for f in (0.05, 0.1, 0.25, 1.0):
        fd = f64(f32(f))
        for name, w in _edge_vectors():
            n = len(w)
            t = SM.alias_table(w, f)
            p = SM.probabilities(w, f)
            cw = SM.clean(w).astype(f64)
            assert (cw >= 0).all() and np.isfinite(cw).all()
            want = (1 - fd) * cw / cw.sum() + fd / n if cw.sum() > 0 else np.full(n, 1.0 / n)
            assert np.abs(p - want).max() <= 1e-15 and abs(p.sum() - 1) <= 1e-12, (name, n, f)
            assert (t["alias_id"] < n).all()
            err = np.abs(SM.reconstructed_probabilities(t) - p).max()
            worst = max(worst, err)
            assert err <= 2.0 ** -30, (name, n, f, err)
            assert (_bits(t["pdf"]) == _bits(p.astype(f32))).all() and (_bits(t["alias_pdf"]) == _bits(p[t["alias_id"]].astype(f32))).all()
            zero = cw == 0
            if cw.sum() > 0:
                assert (p[zero] == fd / n).all() and (f == 1.0 or (p[~zero] > fd / n).all())
            if name == "one holds 0.999" and f == 0.1:
                assert p.max() > 0.89
    assert worst > 0, "every table is exact: the bound checks nothing"


def test_model_draw_frequencies():
    """2^20 seeded words through the draw: every light's count is within 4.5 binomial standard errors of p_i, n = 3 and n = 67; the
    recorded pdf is float32(p_i) of the light drawn."""
    N = 1 << 20
    rng = np.random.default_rng(5)
    for n, f in ((3, 0.1), (67, 0.1), (67, 0.25)):
        w = (10.0 ** rng.uniform(-3, 0, n)).astype(f32)
        w[n // 2] = 0
        t, p = SM.alias_table(w, f), SM.probabilities(w, f)
        words = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
        idx, pdf = SM.draw(t, words)
        assert idx.min() >= 0 and idx.max() < n and (_bits(pdf) == _bits(p.astype(f32)[idx])).all()
        counts = np.bincount(idx, minlength=n)
        se = np.sqrt(N * p * (1 - p))
        z = np.abs(counts - N * p) / se
        assert (z <= 4.5).all(), (n, f, z.max())
        assert counts[n // 2] > 0


def test_model_estimator_has_the_analytic_sum_and_less_variance():
    """test_ris_over_point_lights_has_the_analytic_sum_as_its_mean's construction with one candidate, no reuse, float64, 10^5 draws:
    three point lights of powers 1 : 10 : 1000 at the same distance and elevation above the plane, seen from straight above, so that
    every contribution is its light's power times one common factor.  The mean of contribution * uc_weight is the analytic sum within
    4 standard errors for the uniform and for the power selection (f = 0.1).  The variance: uniform draws 3 c_i with probability 1 / 3,
    var = 3 sum(c_i^2) - (sum c_i)^2 = 1.98e6 c^2; power draws c_i / p_i with p = (0.0342, 0.0422, 0.9235), var = sum(c_i^2 / p_i) -
    (sum c_i)^2 = 6.3e4 c^2: a ratio of 0.032, asserted below 0.1."""
    from tauray_amd import scene as S
    d, elev = 2.0, math.radians(50)
    specs = [((k, k, k), (d * math.cos(elev) * math.cos(a), d * math.sin(elev), d * math.cos(elev) * math.sin(a))) for k, a in ((1.0, 0.3), (10.0, 2.4), (1000.0, 4.5))]
    L = M.Lights(point=T._point_lights(S, specs))
    n = 100_000
    s = T._plane_surface(n)
    every = [M.light_contribution(L, np.zeros(1, dtype=int), np.array([i]), np.zeros((1, 2)), s[:1], f64)[0][0] for i in range(3)]
    want = np.sum(every, 0)
    assert np.allclose(every[1] / every[0], 10, rtol=1e-5) and np.allclose(every[2] / every[0], 1000, rtol=1e-5)
    table = SM.selection_table(SM.light_weights(L.point, None), 3, 0, 0.1)
    var = {}
    for name, tb in (("uniform", None), ("power", table)):
        est, idx = SM.ris_one_candidate(L, s, tb, 7, f64)
        mean, se = est.mean(0), est.std(0, ddof=1) / math.sqrt(n)
        assert (np.abs(mean - want) <= 4 * se).all(), (name, mean, want, se)
        assert set(np.unique(idx)) == {0, 1, 2}
        var[name] = est.var(0, ddof=1)
    assert (var["power"] < var["uniform"]).all()
    assert (var["power"] < 0.1 * var["uniform"]).all(), var


def test_host_builder_and_option_checks_under_the_sanitizers(tmp_path):
    """tests/restir_light_selection_check.cc, built with the address and undefined-behaviour sanitizers and run as a program, no device:
    the library's table builder on hand-derived tables, on the edge vectors and on 64 seeded random vectors of length 1..300 against the
    numpy model byte for byte; --restir-light-selection= parsing and the C++ stage's option check."""
    exe = str(tmp_path / "restir_light_selection_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "restir_light_selection_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)

    def run(*a):
        p = subprocess.run([exe] + list(a), capture_output=True, text=True)
        return p.returncode, p.stdout.strip(), p.stderr.strip()
    assert run("selftest") == (0, "ok", "")
    rng = np.random.default_rng(64)
    vectors = [w for _, w in _edge_vectors()]
    for k in range(64):
        n = int(rng.integers(1, 301))
        w = (10.0 ** rng.uniform(-4, 2, n)).astype(f32)
        w[rng.uniform(size=n) < 0.1] = 0
        vectors.append(w)
    assert {1, 2, 3, 67} <= {len(w) for w in vectors} and max(len(w) for w in vectors) > 200
    path = str(tmp_path / "weights.bin")
    with open(path, "wb") as fh:
        for w in vectors:
            fh.write(np.uint32(len(w)).tobytes() + np.ascontiguousarray(w, dtype="<f4").tobytes())
    for fraction in ("0.1", "0.05", "1"):
        rc, out, err = run("tables", path, fraction)
        assert rc == 0 and err == "", err
        lines = out.split("\n")
        assert len(lines) == len(vectors)
        for w, line in zip(vectors, lines):
            t = SM.alias_table(w, float(fraction))
            want = "".join("%08x" % int(word) for word in t.view("<u4"))      # the entry's four fields are 32-bit words
            assert line == want, (len(w), fraction)
    # the option
    assert run("default") == (0, "0 0.100000001", "")
    for text, want in (("uniform", "0 0.100000001"), ("power", "1 0.100000001"), ("power,0.25", "1 0.25"), ("uniform,0.5", "0 0.5"), ("power,1", "1 1"), ("power,1e-3", "1 0.00100000005")):
        assert run("parse", text) == (0, want, ""), text
    for text in ("", "maybe", "Power", "power ", "1", "uniform;0.1"):
        rc, out, err = run("parse", text)
        assert rc == 1 and out == "" and f"--restir-light-selection: {text.split(',')[0]} is neither uniform nor power" in err, (text, err)
    for text in ("power,", "power,0", "power,-1", "power,1.01", "power,abc", "power,0.1,0.2", "uniform,nan", "power,inf"):
        rc, out, err = run("parse", text)
        assert rc == 1 and out == "" and f"--restir-light-selection: the uniform fraction {text.split(',', 1)[1]} is not a number in (0, 1]" in err, (text, err)
    for mode, fraction in (("0", "0.1"), ("1", "0.1"), ("1", "1"), ("0", "0.001")):
        assert run("check", mode, fraction) == (0, "ok", "")
    for mode in ("-1", "2", "2147483647"):
        rc, out, err = run("check", mode, "0.1")
        assert rc == 1 and f"restir-di: light_selection {mode} is outside 0..1" in err, (mode, err)
    for mode in ("0", "1"):
        for fraction in ("0", "-0.5", "1.5", "nan", "inf"):
            rc, out, err = run("check", mode, fraction)
            assert rc == 1 and "restir-di: uniform_fraction must be in (0, 1]" in err, (mode, fraction, err)


# =========================================================================================================================== GPU
EXTRA_LAMPS, FAN = 37, 61
BLACK = 17                      # the black lamp among the extra ones
ROOM_POINT_LIGHTS = 3           # the room's own


def _fan(S, centre, y_normal=-1.0):
    """An emissive fan of FAN triangles in a horizontal plane around `centre`, facing down: the rim radius grows geometrically over one
    decade, so that the areas - half the product of two neighbouring radii times the sine of the step - span two."""
    angles = np.linspace(0.0, 1.9 * math.pi, FAN + 1)
    radii = 0.06 * 10.0 ** np.linspace(0.0, 1.0, FAN + 1)
    v = np.zeros(FAN + 2, dtype=S.VERTEX)
    c = np.asarray(centre, dtype=f64)
    v["pos"][0] = c
    v["pos"][1:] = c + np.stack([radii * np.cos(angles), np.zeros(FAN + 1), radii * np.sin(angles)], -1)
    v["normal"] = (0, y_normal, 0)
    v["tangent"] = (1, 0, 0, 1)
    v["uv"] = 0.5
    idx = []
    for k in range(FAN):      # cross(rim_k - c, rim_k+1 - c) points to -y
        idx += [0, 1 + k, 2 + k]
    return v, idx


def _extra_lamps(S):
    """EXTRA_LAMPS point lights on a grid under the ceiling; powers log-uniform over three decades, lamp BLACK is black."""
    rng = np.random.default_rng(12)
    out = []
    for k in range(EXTRA_LAMPS):
        power = 12.0 * 10.0 ** (-3.0 * rng.uniform())
        colour = power * rng.uniform(0.6, 1.0, 3)
        if k == BLACK:
            colour = np.zeros(3)
        pos = (-1.7 + 3.4 * (k % 7) / 6.0, 1.8, -1.7 + 3.2 * (k // 7) / 5.0)
        out.append(S.make_point_light(tuple(colour), pos, 0.0))
    return np.concatenate(out)


def _room_plus(S, size, extra=True):
    """tests/test_restir_di.py's room (its quads, cameras, lights and sky, restated: _room builds a finished scene) with the extra lamps
    and the fan."""
    from test_estimator_consistency import _quad, _scene
    from tauray_amd.hdr import load_hdr
    grey = S.make_material(albedo=(0.7, 0.7, 0.7, 1), metallic=0.0, roughness=0.9)
    red = S.make_material(albedo=(0.8, 0.2, 0.15, 1), metallic=0.0, roughness=0.6)
    glossy = S.make_material(albedo=(0.3, 0.5, 0.8, 1), metallic=0.0, roughness=0.35)
    metal = S.make_material(albedo=(0.9, 0.7, 0.3, 1), metallic=1.0, roughness=0.5)
    glow = S.make_material(albedo=(0.2, 0.2, 0.2, 1), metallic=0.0, roughness=1.0, emission=(3.0, 2.0, 1.0))
    fan_glow = S.make_material(albedo=(0.2, 0.2, 0.2, 1), metallic=0.0, roughness=1.0, emission=(5.0, 4.0, 6.0))
    quads = [(*_quad(S, (-2, -1, -2), (0, 0, 4), (4, 0, 0)), grey), (*_quad(S, (-2, -1, -2), (4, 0, 0), (0, 3, 0)), grey),
             (*_quad(S, (-2, -1, -2), (0, 3, 0), (0, 0, 4)), red), (*_quad(S, (2, -1, -2), (0, 0, 4), (0, 3, 0)), grey),
             (*_quad(S, (-2, 2, -2), (4, 0, 0), (0, 0, 2)), grey), (*_quad(S, (-1.99, -0.2, -1.2), (0, 1.0, 0), (0, 0, 1.2)), glow),
             (*_quad(S, (0.2, -1, -0.6), (1.0, 0, 0.3), (0, 1.3, 0)), glossy), (*_quad(S, (-1.2, -0.2, 0.2), (0, 0, 0.9), (0.9, 0, 0)), metal)]
    if extra:
        quads.append((*_fan(S, (0.6, 1.9, -0.9)), fan_glow))
    cams = [V._camera(S, size, eye, (0.0, 0.1, 0.0)) for eye in ((0.0, 0.6, 4.2), (0.9, 1.1, 3.9))]
    point = [S.make_point_light((6, 5, 4), (1.2, 1.4, 0.6), 0.0), S.make_point_light((2, 3, 5), (-1.0, 0.4, 1.2), 0.0),
             S.make_spotlight((14, 13, 11), (0.3, 1.8, 0.9), (-0.2, -1.0, -0.4), 0.0, 35.0, 2.0)]
    if extra:
        point.append(_extra_lamps(S))
    directional = np.concatenate([S.make_directional_light((1.5, 1.4, 1.2), (-0.25, -1.0, -0.6), 3.0), S.make_directional_light((0.6, 0.7, 0.9), (0.3, -1.0, -0.9), 0.0)])
    return _scene(S, quads, cams, point_lights=np.concatenate(point), directional_lights=directional, envmap=load_hdr(os.path.join(GOLDEN, "sky_flat.hdr")),
                  environment_factor=(0.6, 0.6, 0.6, 1.0))


def test_the_room_is_the_room_and_the_additions_span_their_decades():
    """The restated room is test_restir_di's byte for byte; the extra lamps' weights span three decades with one black, the fan's areas two."""
    from tauray_amd import scene as S
    a, b = T._room(S, (13, 7)), _room_plus(S, (13, 7), extra=False)
    for k in ("instances", "spans", "vertices", "indices", "point_lights", "directional_lights"):
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    assert a.camera_data().tobytes() == b.camera_data().tobytes()
    w = SM.light_weights(_extra_lamps(S), None)
    assert len(w) == EXTRA_LAMPS and w[BLACK] == 0 and (np.delete(w, BLACK) > 0).all()
    lit = np.delete(w, BLACK)
    assert 10 ** 2.5 < lit.max() / lit.min() < 10 ** 3.5
    v, idx = _fan(S, (0, 0, 0))
    P = v["pos"][np.asarray(idx).reshape(-1, 3)].astype(f64)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    area = 0.5 * np.linalg.norm(n, axis=-1)
    assert len(area) == FAN and (n[:, 1] < 0).all() and 90 < area.max() / area.min() < 110


class _SRun:
    """V._VRun with the light selection: `frames` frames of a recording stage, per frame the colour and every download; the weights and the
    table of a power stage.  tell: the (name, fraction) trhip_restir_di_set_light_selection is called with behind the create, None: never."""

    def __init__(self, R, ctx, ss, size, frames=3, viewports=(0, 1), tell=None, **options):
        self.size, self.viewports, self.options = size, tuple(viewports), R.restir_di_options(record=True, **options)
        self.mode = V.VM.MODES[self.options["visibility"]]
        st = R.RestirDiStage(ctx, ss, size, len(self.viewports), self.options)
        if tell is not None:
            st.set_light_selection(*tell)
        self.power = st.options["light_selection"] == "power"
        if self.power:
            self.weights, self.table = st.download("light_weights"), st.download("light_table")
        out = ctx.alloc(size[0] * size[1] * 16 * len(self.viewports)).zero()
        self.frames = []
        for _ in range(frames):
            st.run(self.viewports, out)
            f = {n: st.download(n) for n in EXISTING if n != "spatial" or self.options["spatial_samples"]}
            f["color"] = out.download((len(self.viewports), size[1], size[0], 4))
            self.frames.append(f)
        st.close()
        out.free()


@pytest.fixture(scope="module")
def rooms(R, ctx):
    """The room with its additions at every size, uploaded on demand (one scene lives on the device at a time)."""
    from tauray_amd import scene as S
    scenes = {size: _room_plus(S, size) for size in SIZES + ((64, 64),)}
    current = {}

    def get(size, as_strategy=0, fresh=False):
        if fresh or current.get("key") != (size, as_strategy):
            current["ss"] = R.SceneStage(ctx, scenes[size], as_strategy=as_strategy)
            current["key"] = (size, as_strategy)
        return scenes[size], current["ss"]
    return get


REUSE = dict(spatial_samples=2, temporal_reuse=True, search_radius=4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("visibility", VISIBILITIES)
def test_g1_a_stage_told_uniform_is_a_stage_never_told(R, ctx, rooms, visibility):
    """set_light_selection(UNIFORM, f) against no call: every download and the colour byte for byte - three frames, 13 x 7 and 37 x 19,
    every acceleration-structure strategy, this visibility mode."""
    for size in SIZES:
        for strategy in (0, 1, 2):
            scene, ss = rooms(size, as_strategy=strategy)
            opts = dict(candidates=4, rng_seed=9, visibility=visibility, **REUSE)
            a = _SRun(R, ctx, ss, size, **opts)
            b = _SRun(R, ctx, ss, size, tell=("uniform", 0.37), **opts)
            assert not a.power and not b.power and a.frames[-1]["color"][..., :3].max() > 0
            for fi, (fa, fb) in enumerate(zip(a.frames, b.frames)):
                assert set(fa) == set(fb) == set(EXISTING + ("color",))
                for key in fa:
                    assert fa[key].tobytes() == fb[key].tobytes(), (size, strategy, visibility, fi, key)
    rooms(SIZES[0], as_strategy=0)


def _tiny(S, n_point, n_tri):
    """A floor under n_point point lights and an emissive mesh of n_tri triangles."""
    from test_estimator_consistency import _quad, _scene
    grey = S.make_material(albedo=(0.7, 0.6, 0.5, 1), metallic=0.0, roughness=0.7)
    glow = S.make_material(albedo=(0.2, 0.2, 0.2, 1), metallic=0.0, roughness=1.0, emission=(3.0, 2.0, 1.0))
    quads = [(*_quad(S, (-4, -1, -4), (0, 0, 8), (8, 0, 0)), grey)]
    if n_tri:
        v = np.zeros(n_tri + 2, dtype=S.VERTEX)
        v["pos"] = [(0.3 * k * k - 1.0, 3.0, (-1.0) ** k * (0.5 + 0.2 * k)) for k in range(n_tri + 2)]
        v["normal"], v["tangent"], v["uv"] = (0, -1, 0), (1, 0, 0, 1), 0.5
        quads.append((v, [i for k in range(n_tri) for i in (k, k + 1, k + 2)], glow))
    point = [S.make_point_light((1.0 + 5 * k, 0.5, 0.25 * k), (k - 1.0, 1.0 + 0.5 * k, 0.3), 0.0) for k in range(n_point)]
    kw = dict(point_lights=np.concatenate(point)) if point else {}
    return _scene(S, quads, [V._camera(S, (13, 7), (0.0, 2.5, 5.0), (0, -1, 0))], **kw)


def _assert_weights_and_table(stage, scene, ss, fraction):
    tri = ss.tri_lights()
    n_point, n_tri = len(scene.point_lights), len(tri)
    weights, table = stage.download("light_weights"), stage.download("light_table")
    want = SM.light_weights(scene.point_lights, tri)
    assert weights.shape == (n_point + n_tri,) and table.shape == (n_point + n_tri,)
    assert (_bits(weights) == _bits(want)).all(), "the weights are not the model's bits"
    assert table.tobytes() == SM.selection_table(weights, n_point, n_tri, fraction).tobytes(), "the table is not the model's"
    return weights, table


@pytest.mark.gpu
def test_g2_weights_and_table_are_the_models(R, rooms):
    """light_weights against the model's weights and light_table against the model's table of those weights, bit for bit: the room with
    its additions, and tiny scenes with 1, 2 and 3 lights per class and with an empty class; with and without `record`."""
    from tauray_amd import scene as S
    own = R.Context(0)
    for n_point, n_tri in ((1, 1), (2, 2), (3, 3), (0, 2), (2, 0), (1, 3)):
        scene = _tiny(S, n_point, n_tri)
        ss = R.SceneStage(own, scene)
        assert len(ss.tri_lights()) == n_tri
        for record in (False, True):
            st = R.RestirDiStage(own, ss, (13, 7), 1, dict(light_selection="power", uniform_fraction=0.25, record=record))
            w, t = _assert_weights_and_table(st, scene, ss, 0.25)
            assert (w > 0).all()
            out = own.alloc(13 * 7 * 16).zero()
            st.run([0], out)      # a frame of every tiny scene: an empty class is never drawn from
            img = out.download((7, 13, 4))
            assert np.isfinite(img).all() and img[..., :3].max() > 0
            out.free()
            st.close()
    scene = _room_plus(S, (13, 7))
    ss = R.SceneStage(own, scene)
    st = R.RestirDiStage(own, ss, (13, 7), 2, dict(light_selection="power"))
    w, t = _assert_weights_and_table(st, scene, ss, 0.1)
    assert len(w) == ROOM_POINT_LIGHTS + EXTRA_LAMPS + 2 + FAN and w[ROOM_POINT_LIGHTS + BLACK] == 0 and (w > 0).sum() == len(w) - 1
    fan = w[-FAN:]
    assert 90 < fan.max() / fan.min() < 110
    uniform = R.RestirDiStage(own, ss, (13, 7), 2, dict())
    with pytest.raises(R.TrhipError) as e:
        uniform.download("light_table")
    assert "trhip_restir_di_download: the stage has no light selection table (trhip_restir_di_set_light_selection)" in str(e.value)
    uniform.close()
    st.close()
    own.close()


RUNS = {(13, 7): dict(candidates=4, rng_seed=21, **REUSE), (37, 19): dict(candidates=8, rng_seed=22, **REUSE)}


@pytest.fixture(scope="module")
def power_runs(R, ctx, rooms):
    """A recording power stage at both sizes - temporal reuse, two spatial samples, three frames - rendered once; the tests share the
    downloads and leave them unchanged."""
    cache = {}

    def get(size):
        if size not in cache:
            scene, ss = rooms(size)
            cache[size] = _SRun(R, ctx, ss, size, light_selection="power", **RUNS[size])
        return cache[size]
    return get


@pytest.fixture(scope="module")
def power_models(power_runs, rooms):
    """T._model_frame of a power run at both precisions: the model draws through the stage's downloaded table."""
    from tauray_amd import scene as S
    cache = {}

    def get(size):
        if size not in cache:
            run = power_runs(size)
            scene, ss = rooms(size)
            L = _lights_of(S, scene, ss)
            with SM.power_selection(run.table):
                cache[size] = {(fi, v): (T._model_frame(S, run, scene, L, fi, v, f32), T._model_frame(S, run, scene, L, fi, v, f64))
                               for fi in range(len(run.frames)) for v in range(len(run.viewports))}
        return cache[size]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_g3_replay_and_model_of_every_candidate(power_runs, power_models, rooms, size, capsys):
    """The power stage's own stream and downloaded table give every candidate's class, index and light_data (point and directional: bit
    for bit) and a point candidate's pdf bit for bit; the existing float32 replay of update_reservoir, uc_weight and the colour passes
    with the new pdf; the bounded quantities - pdf, triangle light_data, contribution, weight and everything behind them - stay inside
    4 |model32 - model64| + 1 ulp.  Every pixel, three frames, temporal on, two spatial samples, none left out."""
    from tauray_amd import scene as S
    run = power_runs(size)
    scene, ss = rooms(size)
    assert run.power and run.table.tobytes() == SM.selection_table(run.weights, len(scene.point_lights), len(ss.tri_lights()), 0.1).tobytes()
    T.test_replay_of_the_decision_records_is_exact(lambda case: run, 0)
    models = power_models(size)
    T.test_draws_and_picks_are_exact(lambda case: run, lambda case: models, 0)
    T.test_continuous_quantities_are_bounded(lambda case: run, lambda case: models, 0, capsys)
    L = _lights_of(S, scene, ss)
    seen = set()
    for (fi, v), (m32, m64) in models.items():
        cand = run.frames[fi]["candidates"][v][m32["ys"], m32["xs"]]
        t, i = _light_split(cand["light"])
        point = t == 0
        assert (_bits(cand["pdf"][point]) == _bits(m32["pdf"][point])).all(), "a point candidate's pdf is not table pdf * prob_point"
        assert (_bits(cand["pdf"][point]) == _bits(run.table["pdf"][i[point]] * L.prob_point)).all()
        seen |= set(np.unique(t).tolist())
    assert seen == {0, 1, 2, 3}


@pytest.mark.gpu
def test_g4_frequencies_follow_the_recorded_pdf(power_runs, rooms):
    """All recorded candidates of the 37 x 19 run: per class, each light's count is within 4.5 binomial standard errors of pdf / class
    probability = p_i; the black lamp is drawn at its f / n rate - more than zero times, inside the same bound."""
    size = (37, 19)
    run = power_runs(size)
    scene, ss = rooms(size)
    n_point, n_tri = len(scene.point_lights), len(ss.tri_lights())
    types, indices = [], []
    for f in run.frames:
        hit = f["surface"]["instance_id"] >= 0
        t, i = _light_split(f["candidates"]["light"][hit])
        keep = ~((t == 0) & (i == M.NULL_INDEX))
        types.append(t[keep])
        indices.append(i[keep])
    t, i = np.concatenate(types), np.concatenate(indices)
    for cls, n, table in ((0, n_point, run.table[:n_point]), (1, n_tri, run.table[n_point:])):
        p = table["pdf"].astype(f64)
        assert abs(p.sum() - 1) < 1e-5
        N = int((t == cls).sum())
        counts = np.bincount(i[t == cls], minlength=n)
        assert N > 4000 and len(counts) == n
        z = np.abs(counts - N * p) / np.sqrt(N * p * (1 - p))
        assert (z <= 4.5).all(), (cls, N, z.max(), int(z.argmax()))
        if cls == 0:
            black = ROOM_POINT_LIGHTS + BLACK
            assert _bits(table["pdf"][black]) == _bits(f32(f64(f32(0.1)) / n_point)) and counts[black] > 0, counts[black]


POWER_EXPECTATION = {
    "8 candidates, no reuse": (dict(candidates=8, spatial_samples=0, temporal_reuse=False, light_selection="power"), 1, 24),
    "the defaults, frame 8": (dict(light_selection="power"), 9, 24),
    "uniform pdf through the table (f = 1), 8 candidates, no reuse": (dict(candidates=8, spatial_samples=0, temporal_reuse=False, light_selection="power", uniform_fraction=1.0), 1, 24),
}


@pytest.fixture(scope="module")
def direct64(R, ctx, rooms):
    """The direct stage's 16 batches at 64 spp of the room with its additions at 64 x 64, rendered once."""
    cache = {}

    def get():
        if not cache:
            scene, ss = rooms((64, 64))
            cache["base"] = V._direct_batches(R, ctx, ss, scene, (64, 64), 16)
        return cache["base"]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POWER_EXPECTATION))
def test_g5_power_has_the_direct_stages_expectation(R, ctx, rooms, direct64, name, capsys):
    """T.test_same_expectation_as_the_direct_stage's procedure, _assert_same_mean as it is, for the power selection: without reuse, with
    the defaults at frame 8, and with f = 1 - a uniform pdf through the table path."""
    from test_estimator_consistency import _assert_same_mean
    size, K = (64, 64), 16
    base = direct64()
    scene, ss = rooms(size)
    options, frames, seeds = POWER_EXPECTATION[name]
    got = V._restir_batches(R, ctx, ss, size, K, options, frames, seeds, "per-target")
    assert np.isfinite(got).all()
    se = got.mean((1, 2)).std(0, ddof=1) / math.sqrt(K) / got.mean((0, 1, 2))
    with capsys.disabled():
        print(f"\nrestir di power selection against the direct stage, {name}: standard error of a batch mean {se.max():.2%} (times sqrt(K): {se.max() * math.sqrt(K):.3f})")
    assert (se * math.sqrt(K) < 0.05).all(), "a batch is too noisy to say anything"
    rel, z = _assert_same_mean(base, got, name)
    with capsys.disabled():
        print(f"restir di power selection against the direct stage, {name}: image means differ by {rel:.3%} ({z:.2f} standard errors)")


@pytest.mark.gpu
def test_g6_a_stale_table_keeps_the_expectation_and_a_refresh_rebuilds_once(R, ctx, rooms, capsys):
    """update_lights swaps the colours of the brightest lamp and the black one behind the stage's back: the table now gives the
    lamp that holds most of the power its f / n share.  Rendered without a refresh and with one, 8 candidates and no reuse: both have the
    direct stage's mean of the swapped scene (_assert_same_mean as it is).  The refresh reports rebuilt = 1, a second one 0."""
    from test_estimator_consistency import _assert_same_mean
    size, K, seeds = (64, 64), 16, 24
    scene, ss = rooms(size, fresh=True)
    before = np.array(scene.point_lights, copy=True)
    bright, black = int(SM.light_weights(before, None).argmax()), ROOM_POINT_LIGHTS + BLACK
    share = 20 * f64(f32(0.1)) / len(before)      # twenty times the uniform share: what the brightest lamp's pdf exceeds by far, and the black one's is not
    after = before.copy()
    after["color"][[bright, black]] = before["color"][[black, bright]]
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    got = {False: np.zeros((K, size[1], size[0], 3)), True: np.zeros((K, size[1], size[0], 3))}
    try:
        seed = 1
        for k in range(K):
            for _ in range(seeds):
                for refresh in (False, True):
                    ss.update_lights(before, scene.directional_lights)
                    st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(rng_seed=seed, candidates=8, spatial_samples=0, temporal_reuse=False, light_selection="power"))
                    assert st.refresh_light_selection() is False      # nothing moved yet
                    ss.update_lights(after, scene.directional_lights)
                    if refresh:
                        assert st.refresh_light_selection() is True and st.refresh_light_selection() is False
                        if seed == 1:
                            t = st.download("light_table")
                            assert t["pdf"][bright] == f32(f64(f32(0.1)) / len(before)) and t["pdf"][black] > share
                    elif seed == 1:
                        t = st.download("light_table")
                        assert t["pdf"][black] == f32(f64(f32(0.1)) / len(before)) and t["pdf"][bright] > share, "the table is not stale"
                    st.run([0], buf)
                    got[refresh][k] += buf.download((size[1], size[0], 4))[..., :3] / seeds
                    st.close()
                seed += 1
        base = V._direct_batches(R, ctx, ss, scene, size, K)
    finally:
        ss.update_lights(before, scene.directional_lights)
        buf.free()
    for refresh, name in ((False, "stale table"), (True, "refreshed table")):
        assert np.isfinite(got[refresh]).all()
        se = got[refresh].mean((1, 2)).std(0, ddof=1) / math.sqrt(K) / got[refresh].mean((0, 1, 2))
        rel, z = _assert_same_mean(base, got[refresh], name)
        with capsys.disabled():
            print(f"\nrestir di power selection, {name}: image means differ from the direct stage's by {rel:.3%} ({z:.2f} standard errors), "
                  f"standard error of a batch mean {se.max():.2%}")
        assert (se * math.sqrt(K) < 0.05).all(), "a batch is too noisy to say anything"


@pytest.mark.gpu
def test_g7_power_has_the_lower_error(R, ctx, rooms, capsys):
    """One candidate, no temporal or spatial reuse, 64 x 64, 16 seeds: the mean squared error against a 4096 spp direct-stage image is
    strictly lower for the power selection than for the uniform one."""
    from test_estimator_consistency import _dup
    size = (64, 64)
    scene, ss = rooms(size)
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    direct = R.DirectStage(ctx, ss, R.options_for_scene(scene, samples_per_pixel=4096, samples_per_pass=1, rng_seed=999), _dup(size))
    direct.run(buf)
    ref = buf.download((size[1], size[0], 4))[..., :3].astype(f64)
    direct.close()
    mse = dict(uniform=0.0, power=0.0)
    for seed in range(1, 17):
        for name in mse:
            st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(rng_seed=seed, candidates=1, spatial_samples=0, temporal_reuse=False, light_selection=name))
            st.run([0], buf)
            img = buf.download((size[1], size[0], 4))[..., :3].astype(f64)
            st.close()
            assert np.isfinite(img).all()
            mse[name] += np.mean((img - ref) ** 2) / 16
    buf.free()
    with capsys.disabled():
        print(f"\nrestir di light selection in the room with 40 point and 63 triangle lights at 64 x 64, one candidate, no reuse: MSE against 4096 spp: "
              f"uniform {mse['uniform']:.4e}, power {mse['power']:.4e}, ratio {mse['power'] / mse['uniform']:.3f}")
    assert mse["power"] < mse["uniform"]


@pytest.mark.gpu
def test_g8_refusals_and_determinism(R, ctx, rooms):
    from tauray_amd import scene as S
    size = (37, 19)
    scene, ss = rooms(size)
    st = R.RestirDiStage(ctx, ss, size, 2, R.restir_di_options(light_selection="power", **REUSE))
    out = ctx.alloc(size[0] * size[1] * 16 * 2).zero()
    st.set_light_selection("uniform", 0.5)      # no history yet: anything
    st.set_light_selection("power", 0.2)
    st.run([0, 1], out)
    st.set_light_selection("power", 0.2)        # the history's own
    for other in (("uniform", 0.2), ("power", 0.25), ("uniform", 0.1)):
        with pytest.raises(R.TrhipError) as e:
            st.set_light_selection(*other)
        assert "trhip_restir_di_set_light_selection: the stage holds history of the power selection with uniform_fraction 0.2" in str(e.value)
        assert ": call trhip_restir_di_reset first" in str(e.value)
        assert (st.options["light_selection"], st.options["uniform_fraction"]) == ("power", 0.2)
    assert st.refresh_light_selection() is False      # allowed with history; nothing moved
    for mode, fraction, text in ((2, 0.1, "mode 2 is outside 0..1"), (-1, 0.1, "mode -1 is outside 0..1"), (1, 0.0, "uniform_fraction must be in (0, 1]"),
                                 (0, 1.5, "uniform_fraction must be in (0, 1]"), (1, float("nan"), "uniform_fraction must be in (0, 1]")):
        with pytest.raises(R.TrhipError) as e:
            R.check(st._fn("set_light_selection")(st.h, mode, fraction))
        assert "trhip_restir_di_set_light_selection: " + text in str(e.value)
    st.reset()
    st.set_light_selection("uniform", 0.1)
    st.run([0, 1], out)
    with pytest.raises(R.TrhipError):
        st.set_light_selection("power", 0.1)
    st.reset()
    st.set_light_selection("power", 0.1)
    st.run([0, 1], out)
    # a scene with another light count under the stage: render names the refresh
    ctx.sync()
    fewer = _room_plus(S, size, extra=False)
    ss2 = R.SceneStage(ctx, fewer)
    with pytest.raises(R.TrhipError) as e:
        st.run([0, 1], out)
    assert ("trhip_restir_di_render: the scene has 3 point and 2 triangle lights, the light selection table was built for 40 and 63: "
            "call trhip_restir_di_refresh_light_selection first") in str(e.value)
    assert st.refresh_light_selection() is True
    st.run([0, 1], out)
    st.close()
    out.free()
    # a power stage on a device without a scene
    empty = R.Context(0)
    with pytest.raises(R.TrhipError) as e:
        R.RestirDiStage(empty, None, size, 1, R.restir_di_options(light_selection="power"))
    assert "trhip_restir_di_set_light_selection: no scene" in str(e.value)
    empty.close()
    # determinism: two fresh runs, the structures, one stage against two
    scene, ss = rooms(size, fresh=True)
    opts = dict(candidates=4, spatial_samples=3, temporal_reuse=True, search_radius=6.0, rng_seed=5, light_selection="power")
    a, ha = T._frames(R, ctx, ss, size, [0, 1], 3, **opts)
    b, hb = T._frames(R, ctx, ss, size, [0, 1], 3, **opts)
    assert (_bits(a) == _bits(b)).all() and ha.tobytes() == hb.tobytes(), "two fresh runs differ"
    c, hc = T._frames(R, ctx, ss, size, [0, 1], 3, **dict(opts, light_selection="uniform"))
    assert not (_bits(a) == _bits(c)).all(), "the selection changes nothing in the room"
    for v in (0, 1):
        e, _ = T._frames(R, ctx, ss, size, [v], 3, **opts)
        assert (_bits(e[:, 0]) == _bits(a[:, v])).all(), f"viewport {v} alone differs"
    for strategy in (1, 2):
        scene, ss2 = rooms(size, as_strategy=strategy)
        g, hg = T._frames(R, ctx, ss2, size, [0, 1], 3, **opts)
        assert (_bits(g) == _bits(a)).all() and hg.tobytes() == ha.tobytes(), f"acceleration-structure strategy {strategy} differs"
    rooms(size, as_strategy=0)


@pytest.mark.gpu
@pytest.mark.parametrize("renderer, which", [("restir-di", "still"), ("restir-di", "animation"), ("restir-gi", "still")])
def test_g9_both_hosts_render_the_same_frames(R, ctx, tmp_path, renderer, which):
    """tauray_hip --restir-light-selection=power,0.1 against the Python renderers: three frames at 96 x 96 as .raw, bit for bit - test.glb
    under restir-di and restir-gi, and animated.glb under --animation with restir-di (a refresh per frame on both sides)."""
    from tauray_amd.gltf import load_glb
    from tauray_amd.animation import SceneAnimator
    size, frames = (96, 96), 3
    glb = os.path.join(GOLDEN, "animated.glb" if which == "animation" else "test.glb")
    prefix = str(tmp_path / "cpp")
    args = [CLI, glb, "--renderer=" + renderer, "--restir=4,2,16,16,on", "--restir-light-selection=power,0.1", f"--width={size[0]}", f"--height={size[1]}",
            f"--frames={frames}", "--filetype=raw", "--format=rgba32", "--rng-seed=3", "--headless=" + prefix]
    if renderer == "restir-gi":
        args.append("--restir-gi=2,16,8,on")
    if which == "animation":
        args.append("--animation")
    p = subprocess.run(args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    scene = load_glb(glb, *size)
    ss = R.SceneStage(ctx, scene)
    mrd = T.scene_min_ray_dist(R, scene)
    animator = None
    if which == "animation":
        animator = SceneAnimator(scene)
        animator.play("")
    di = R.restir_di_options(candidates=4, spatial_samples=2, search_radius=16.0, max_confidence=16.0, temporal_reuse=True, rng_seed=3, min_ray_dist=mrd,
                             light_selection="power", uniform_fraction=0.1)
    if renderer == "restir-di":
        rr = R.RestirDiRenderer(ctx, ss, scene, size, di)
    else:
        rr = R.RestirGiRenderer(ctx, ss, scene, size, R.restir_gi_options(spatial_samples=2, search_radius=16.0, max_confidence=8.0, temporal_reuse=True, rng_seed=3, min_ray_dist=mrd), di)
    stage = rr.stage if renderer == "restir-di" else rr.direct
    assert stage.options["light_selection"] == "power" and stage.options["uniform_fraction"] == 0.1
    for f in range(frames):
        if animator:
            ss.animate(animator, 0 if f == 0 else round(1000000.0 / 60.0), refit=(f % 3 != 2))
        rr.render()
        img = rr.download("display")
        assert np.isfinite(img).all() and img[..., :3].max() > 0
        got = T._raw(f"{prefix}{f}.raw", (size[1], size[0], 4))
        differing = int((_bits(got) != _bits(img[0])).any(-1).sum())
        assert differing == 0, f"{renderer} {which}, frame {f}: {differing} of {size[0] * size[1]} pixels differ"
    rr.close()
