"""ReSTIR DI (trhip_restir_di_*, tauray_amd/csrc/restir_di.{h,hip}).

CPU: the ABI, the refusals of create and of the command line, the host sanitizers' program, and the numpy model of restir_di.h
(tests/restir_di_model.py) held to closed forms that need no GPU.  GPU: the stage against that model - exactly where the model can be
exact (the replay of the reservoir updates from the decision records, the random draws, the light picks), within
4 |float32 model - float64 model| + one float32 ulp where it cannot (DESIGN.md section 19's bound) - against the direct stage for its
expectation, against itself for reuse and layout, and both hosts against each other."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import restir_di_model as M
from conftest import GOLDEN, ROOT

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
        assert hasattr(L, "trhip_restir_di_" + name) and "trhip_restir_di_" + name in _lib.SYMBOLS
    structs = ["options", "surface", "reservoir", "candidate", "temporal", "spatial", "final", "timings"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "trhip.h"\nint main(void) {\n' +
                   "".join(f'    printf("%zu\\n", sizeof(trhip_restir_di_{s}));\n' for s in structs) +
                   '    printf("%d %d %d %d %d %d %d\\n", TRHIP_RESTIR_DI_SURFACE, TRHIP_RESTIR_DI_CANONICAL, TRHIP_RESTIR_DI_HISTORY, TRHIP_RESTIR_DI_CANDIDATES,'
                   " TRHIP_RESTIR_DI_TEMPORAL, TRHIP_RESTIR_DI_SPATIAL, TRHIP_RESTIR_DI_FINAL);\n    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    header = dict(zip(structs, (int(v) for v in out[:len(structs)])))
    assert header == dict(options=32, surface=112, reservoir=32, candidate=48, temporal=32, spatial=64, final=32, timings=144)
    assert C.sizeof(_lib.RestirDiOptionsC) == header["options"] and C.sizeof(_lib.RestirDiTimingsC) == header["timings"]
    for s, dtype in (("surface", _lib.RESTIR_DI_SURFACE_DTYPE), ("reservoir", _lib.RESTIR_DI_RESERVOIR_DTYPE), ("candidate", _lib.RESTIR_DI_CANDIDATE_DTYPE),
                     ("temporal", _lib.RESTIR_DI_TEMPORAL_DTYPE), ("spatial", _lib.RESTIR_DI_SPATIAL_DTYPE), ("final", _lib.RESTIR_DI_FINAL_DTYPE)):
        assert np.dtype(dtype).itemsize == header[s], s
    assert [int(v) for v in out[len(structs)].split()] == [_lib.RESTIR_DI_SURFACE, _lib.RESTIR_DI_CANONICAL, _lib.RESTIR_DI_HISTORY, _lib.RESTIR_DI_CANDIDATES,
                                                           _lib.RESTIR_DI_TEMPORAL, _lib.RESTIR_DI_SPATIAL, _lib.RESTIR_DI_FINAL]
    assert _lib.RESTIR_DI_NULL_INDEX == M.NULL_INDEX


class _NoDevice:
    h = None


@pytest.mark.parametrize("size, layers, options, text", [
    ((16, 16), 1, {}, "no CPU fallback"),
    ((0, 16), 1, {}, "zero width, height or layer count"),
    ((16, 16), 0, {}, "zero width, height or layer count"),
    ((16385, 16), 1, {}, "image too large"),
    ((16, 16), 4097, {}, "image too large"),
    ((16, 16), 1, dict(candidates=0), "candidates 0 is outside 1..32"),
    ((16, 16), 1, dict(candidates=33), "candidates 33 is outside 1..32"),
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
        R.RestirDiStage(None, None, size, layers, options)
    assert "trhip_restir_di_create" in str(e.value) and text in str(e.value)
    with pytest.raises(AttributeError):
        R.restir_di_options(candidate=3)


@pytest.mark.parametrize("args, text", [
    (["--renderer=restir-di", "--denoiser=bmfr"], "--renderer=restir-di: no --denoiser"),
    (["--renderer=restir-di", "--taa=4"], "--renderer=restir-di: no --taa"),
    (["--renderer=restir-di", "--temporal-reprojection=0.5"], "--renderer=restir-di: no --spatial-reprojection or --temporal-reprojection"),
    (["--renderer=restir-di", "--camera-grid=2,1,0.1,0.1", "--spatial-reprojection=0"], "--renderer=restir-di: no --spatial-reprojection or --temporal-reprojection"),
    (["--renderer=restir-di", "--display=looking-glass"], "--renderer=restir-di: no --display=looking-glass"),
    (["--renderer=restir-di", "--samples-per-pixel=2"], "--samples-per-pixel must be 1"),
    (["--renderer=restir-di", "--devices=0,1"], "--renderer=restir-di runs on one device"),
    (["--renderer=restir-di", "--process-count=2", "--process-rank=0"], "--renderer=restir-di runs in one process"),
    (["--renderer=restir-di", "--restir=0"], "--restir: candidates must be a whole number in 1..32"),
    (["--renderer=restir-di", "--restir=4,5"], "--restir: spatial_samples must be a whole number in 0..4"),
    (["--renderer=restir-di", "--restir=4,2,-1"], "search_radius must be in (0, 1024]"),
    (["--renderer=restir-di", "--restir=4,2,8,0"], "max_confidence must be finite and at least 1"),
    (["--renderer=restir-di", "--restir=temporal_reuse=maybe"], "temporal_reuse=maybe is neither on nor off"),
    (["--renderer=restir-di", "--restir=radius=3"], "--restir: radius is not one of its fields"),
    (["--restir=4"], "--restir sets the options of --renderer=restir-di"),
    (["--renderer=restir"], "unknown renderer restir "),
])
def test_cli_refuses(args, text):
    p = subprocess.run([CLI] + args + [os.path.join(GOLDEN, "test.glb"), "--width=16", "--height=16", "--filetype=none"], capture_output=True, text=True)
    assert p.returncode != 0 and text in p.stderr, p.stderr
    assert "--restir=candidates,spatial_samples,search_radius,max_confidence,temporal_reuse" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout


def test_host_option_checks_under_the_sanitizers(tmp_path):
    """tests/restir_di_check.cc: --restir= parsing and the C++ renderer's option checks, built with address and undefined-behaviour
    sanitizers, no device."""
    exe = str(tmp_path / "restir_di_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "restir_di_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)

    def run(*a):
        p = subprocess.run([exe] + list(a), capture_output=True, text=True)
        return p.returncode, p.stdout.strip(), p.stderr.strip()
    assert run("parse", "") == (0, "4 2 32 16 1", "")
    assert run("parse", "8,3,12.5,20,off") == (0, "8 3 12.5 20 0", "")
    assert run("parse", "spatial_samples=0,temporal_reuse=false,candidates=32") == (0, "32 0 32 16 0", "")
    assert run("parse", "1,max_confidence=4") == (0, "1 2 32 4 1", "")
    for text, why in (("33", "candidates must be a whole number in 1..32"), ("2.5", "candidates must be a whole number"), ("4,2,8,16,on,1", "more than 5 values"),
                      ("candidates=", "candidates has no value"), ("4,x", "spatial_samples=x is not a number"), ("4,2,0", "search_radius must be in (0, 1024]"),
                      ("4,2,nan", "search_radius must be in (0, 1024]"), ("bogus=1", "bogus is not one of its fields")):
        rc, out, err = run("parse", text)
        assert rc == 1 and why in err, (text, err)
    assert run("check", "4", "2", "32", "16", "1e-4") == (0, "ok", "")
    for a, why in ((("0", "2", "32", "16", "1e-4"), "candidates 0 is outside 1..32"), (("4", "5", "32", "16", "1e-4"), "spatial_samples 5 is outside 0..4"),
                   (("4", "2", "32", "0.5", "1e-4"), "max_confidence"), (("4", "2", "32", "16", "0"), "min_ray_dist")):
        rc, out, err = run("check", *a)
        assert rc == 1 and why in err, (a, err)


# ---- the model against closed forms
def test_update_reservoir_selects_in_proportion_to_the_weights():
    """Streaming update_reservoir over weights w picks index i with frequency w_i / sum: 10^5 seeded streams, 4 binomial standard errors."""
    rng = np.random.default_rng(16)
    w = np.array([0.5, 0.0, 2.0, 1.25, 0.25, 3.0], dtype=f32)
    n = 100_000
    u = rng.random((n, len(w))).astype(f32)
    wsum = np.zeros(n, dtype=f32)
    chosen = np.full(n, -1)
    for i, wi in enumerate(w):
        wsum, take = M.update_reservoir(wsum, np.full(n, wi, dtype=f32), u[:, i])
        chosen[take] = i
    assert (wsum == w.sum(dtype=f32)).all()
    p = w.astype(f64) / w.sum()
    freq = np.bincount(chosen, minlength=len(w)) / n
    assert (np.abs(freq - p) <= 4 * np.sqrt(p * (1 - p) / n) + 1e-12).all(), (freq, p)
    assert freq[1] == 0


def test_pairwise_mis_weights_sum_to_one():
    """Equal target functions and unit Jacobians: mis_canonical summed over the neighbours plus every mis_noncanonical plus the canonical
    sample's own confidence share is 1, whatever the confidences."""
    rng = np.random.default_rng(3)
    for dt, tol in ((f32, 4e-7), (f64, 1e-15)):
        for _ in range(50):
            k = int(rng.integers(1, 5))
            conf = rng.uniform(1, 16, k + 1).astype(dt)
            total = conf[0]
            for c in conf[1:]:
                total = dt(total + c)
            p = dt(rng.uniform(0.1, 3.0))
            one = dt(1)
            canonical_m = dt(conf[0] / total)
            s = dt(0)
            for c in conf[1:]:
                canonical_m = dt(canonical_m + M.mis_canonical(conf[0], c, total, p, p, one, dt))
                s = dt(s + M.mis_noncanonical(conf[0], c, total, p, p, one, dt))
            assert abs(float(canonical_m) + float(s) - 1.0) <= tol * (k + 1)
    assert M.mis_canonical(f32(4), f32(4), f32(8), f32(0), f32(1), f32(1), f32) == 0 and M.mis_noncanonical(f32(4), f32(4), f32(8), f32(0), f32(1), f32(1), f32) == 0


def test_reconnection_jacobian():
    """1 for identical source points; for a displaced one the ratio of the solid angles a small patch of the light subtends from the two
    points (finite differences); 1 without a normal (point lights); 0 instead of inf / NaN."""
    dst, n = np.array([[0.3, 2.0, -0.4]]), np.array([[0.0, -1.0, 0.0]])
    a, b = np.array([[0.1, 0.0, 0.2]]), np.array([[-0.7, 0.4, 0.9]])
    assert M.jacobian(a, a, dst, n, f64)[0] == 1.0 and M.jacobian(a.astype(f32), a.astype(f32), dst.astype(f32), n.astype(f32), f32)[0] == 1.0

    def solid_angle(src, eps=1e-4):      # of the square patch of side eps around dst in the light's plane, by its corners' spherical excess
        e1, e2 = np.array([1.0, 0, 0]), np.array([0, 0, 1.0])
        c = [dst[0] + eps * (sx * e1 + sy * e2) / 2 - src[0] for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        c = [v / np.linalg.norm(v) for v in c]

        def tri(p, q, r):
            return 2 * math.atan2(abs(np.dot(p, np.cross(q, r))), 1 + np.dot(p, q) + np.dot(q, r) + np.dot(p, r))
        return tri(c[0], c[1], c[2]) + tri(c[0], c[2], c[3])
    want = solid_angle(b) / solid_angle(a)      # d omega at the current source per d omega at the previous one
    got = M.jacobian(a, b, dst, n, f64)[0]
    assert abs(got / want - 1) < 1e-6, (got, want)
    assert abs(M.jacobian(a.astype(f32), b.astype(f32), dst.astype(f32), n.astype(f32), f32)[0] / want - 1) < 1e-5
    assert M.jacobian(a, b, dst, np.zeros((1, 3)), f64)[0] == 1.0
    assert M.jacobian(dst, b, dst, n, f64)[0] == 0.0 and M.jacobian(a, dst, dst, n, f64)[0] == 0.0


def _plane_surface(n, dt=f32, pos=None, albedo=(0.8, 0.5, 0.3), roughness=1.0, view=(0, -1, 0)):
    """n surface records of a diffuse dielectric plane y = 0 seen from above."""
    from tauray_amd import _lib
    s = np.zeros(n, dtype=np.dtype(_lib.RESTIR_DI_SURFACE_DTYPE))
    s["pos"] = 0 if pos is None else pos
    s["mapped_normal"] = s["flat_normal"] = (0, 1, 0)
    s["view"] = np.asarray(view, dtype=f64) / np.linalg.norm(view)
    s["albedo"] = tuple(albedo) + (1,)
    s["metallic"], s["roughness"], s["transmittance"] = 0.0, roughness * roughness, 0.0
    s["ior_in"], s["ior_out"] = 1.0, 1.45
    s["f0"] = ((1.45 - 1) / (1.45 + 1)) ** 2
    return s


def _point_lights(S, specs):
    return np.concatenate([S.make_point_light(c, p, 0.0) for c, p in specs])


def test_light_contribution_at_normal_incidence():
    """A point light straight above a rough dielectric: the contribution is modulate_bsdf of the lobes (test_estimator_consistency's
    double-precision material model, which shares no code with the kernels) times color / d^2."""
    from tauray_amd import scene as S
    from test_estimator_consistency import _bsdf_lobes
    colour, d = np.array([3.0, 2.0, 1.0]), 2.5
    L = M.Lights(point=_point_lights(S, [(tuple(colour), (0.0, d, 0.0))]))
    for roughness in (1.0, 0.5):
        for view in ((0, -1, 0), (0.6, -0.8, 0.0)):
            s = _plane_surface(1, roughness=roughness, view=view)
            v = -np.asarray(s["view"][0], dtype=f64)
            tview = np.array([np.dot(v, t[0]) for t in M.create_tangent_space(np.array([[0.0, 1.0, 0.0]]), f64)])
            dif, spec = _bsdf_lobes(tview, np.array([0.0, 0.0, 1.0]), roughness)
            want = (np.array([0.8, 0.5, 0.3]) * dif + spec) * colour / d ** 2
            for dt, tol in ((f64, 1e-6), (f32, 1e-5)):
                value, direction, dist2, normal = M.light_contribution(L, np.array([0]), np.array([0]), np.zeros((1, 2)), s, dt)
                assert np.abs(value[0] / want - 1).max() < tol, (roughness, view, value, want)
                assert np.allclose(direction[0], (0, 1, 0)) and abs(dist2[0] - d * d) < 1e-5 and (normal == 0).all()
    # the null sample, an index past the table and a light below the horizon give nothing
    s = _plane_surface(3)
    value = M.light_contribution(L, np.array([0, 0, 0]), np.array([M.NULL_INDEX, 1, 0]), np.zeros((3, 2)), s, f32)[0]
    assert (value[:2] == 0).all() and (value[2] > 0).all()
    L2 = M.Lights(point=_point_lights(S, [((1, 1, 1), (0.0, -1.0, 0.0))]))
    assert (M.light_contribution(L2, np.array([0]), np.array([0]), np.zeros((1, 2)), s[:1], f32)[0] == 0).all()


def test_ris_over_point_lights_has_the_analytic_sum_as_its_mean():
    """RIS as the canonical kernel runs it (uniform light choice, target = luminance, the final estimate contribution * uc_weight), all
    lights visible: the mean over 40 000 seeded pixels is the sum over the lights of their contributions, 4 standard errors."""
    from tauray_amd import scene as S
    specs = [((4, 3, 2), (0.5, 1.5, 0.2)), ((1, 2, 6), (-1.0, 0.7, 0.4)), ((9, 9, 9), (0.2, 3.0, -1.0)), ((2, 0.5, 0.5), (1.5, 0.4, 1.0)), ((1, 1, 1), (0.0, -2.0, 0.0))]
    L = M.Lights(point=_point_lights(S, specs))
    n, candidates = 40_000, 4
    s = _plane_surface(n)
    every = [M.light_contribution(L, np.zeros(1, dtype=int), np.array([i]), np.zeros((1, 2)), s[:1], f64)[0][0] for i in range(len(specs))]
    want = np.sum(every, 0)
    assert (every[4] == 0).all() and (want > 0).all()
    for dt in (f32, f64):
        rs = M.init_sampler(np.arange(n) % 200, np.arange(n) // 200, 0, 0, 7)
        wsum, target, chosen = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt), np.full(n, M.NULL_INDEX)
        for _ in range(candidates):
            rs = M.pcg4d(rs)
            typ, idx, data, pdf = M.sample_canonical(L, rs, s["pos"], 1e-4, dt)
            assert (typ == 0).all() and idx.min() == 0 and idx.max() == len(specs) - 1
            t = M.luminance(M.light_contribution(L, typ, idx, data, s, dt)[0], dt)
            w = M.nan_to_zero((dt(1) / dt(candidates)) * t / pdf)
            rs = M.pcg4d(rs)
            wsum, take = M.update_reservoir(wsum, w, M.unit(rs, dt)[:, 0])
            chosen, target = np.where(take, idx, chosen), np.where(take, t, target)
        ucw = M.uc_weight(wsum, target, dt)
        est = M.light_contribution(L, np.zeros(n, dtype=int), chosen, np.zeros((n, 2)), s, dt)[0] * ucw[:, None]
        mean, se = est.mean(0, dtype=f64), est.std(0, ddof=1, dtype=f64) / math.sqrt(n)
        assert (np.abs(mean - want) <= 4 * se).all(), (dt, mean, want, se)
        assert (se < 0.02 * want).all()


# ---- the model at float32 against float64
def _synthetic_records(n, seed=5):
    """Seeded random surface records above a jittered floor, random materials, and a light table with every class but the environment."""
    from tauray_amd import scene as S
    rng = np.random.default_rng(seed)
    s = _plane_surface(n)
    s["pos"] = np.stack([rng.uniform(-2, 2, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-2, 2, n)], -1)
    nrm = np.stack([rng.normal(0, 0.15, n), np.ones(n), rng.normal(0, 0.15, n)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    s["mapped_normal"] = s["flat_normal"] = nrm
    eye = np.array([0.0, 3.0, 4.0])
    view = s["pos"].astype(f64) - eye
    s["view"] = view / np.linalg.norm(view, axis=-1, keepdims=True)
    s["albedo"][:, :3] = rng.uniform(0.1, 0.9, (n, 3))
    s["metallic"] = rng.choice([0.0, 1.0, 0.3], n)
    s["roughness"] = rng.uniform(0.2, 1.0, n) ** 2
    s["instance_id"] = 0
    point = np.concatenate([S.make_point_light((4, 3, 2), (0.5, 1.5, 0.2), 0.0), S.make_point_light((1, 2, 6), (-1.0, 0.7, 0.4), 0.0),
                            S.make_spotlight((9, 8, 7), (0.2, 2.0, -1.0), (0.1, -1.0, 0.3), 0.0, 40.0, 2.0)])
    directional = np.concatenate([S.make_directional_light((1.5, 1.4, 1.2), (-0.2, -1.0, -0.3), 3.0), S.make_directional_light((0.5, 0.6, 0.9), (0.4, -1.0, 0.1), 0.0)])
    tri = np.zeros(2, dtype=S.TRI_LIGHT)
    tri["pos"][0] = [(-1.0, 1.5, -2.5), (1.0, 1.5, -2.5), (1.0, 2.5, -2.5)]
    tri["pos"][1] = [(-1.0, 1.5, -2.5), (1.0, 2.5, -2.5), (-1.0, 2.5, -2.5)]
    tri["emission_factor"] = (255 << 0) | (200 << 9) | (150 << 18) | (19 << 27)
    tri["emission_tex_id"] = -1
    return s, M.Lights(point=point, tri=tri, directional=directional), eye


def test_model_float32_against_float64(capsys):
    """The model at both precisions on seeded random surface records and lights: the disagreement of every continuous quantity relative
    to the largest value of its kind (section 20's measure), and the share of pixels whose discrete decisions - the neighbour offsets
    after rounding, the good / bad bits, the reuse bit, the selected candidate - differ.  At most 1 % of the pixels may differ: that is
    the cap the GPU tests below leave out of their comparison."""
    n, candidates = 4096, 8
    s, L, eye = _synthetic_records(n)
    out = {}
    for dt in (f32, f64):
        rs = M.init_sampler(np.arange(n) % 64, np.arange(n) // 64, 0, 4, 0)
        q = dict(pdf=[], contribution=[], weight=[])
        wsum, target, chosen = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt), np.full(n, -1)
        for c in range(candidates):
            rs = M.pcg4d(rs)
            typ, idx, data, pdf = M.sample_canonical(L, rs, s["pos"], 1e-4, dt)
            contrib = M.light_contribution(L, typ, idx, data, s, dt)[0]
            t = M.luminance(contrib, dt)
            w = M.nan_to_zero((dt(1) / dt(candidates)) * t / pdf)
            rs = M.pcg4d(rs)
            wsum, take = M.update_reservoir(wsum, w, M.unit(rs, dt)[:, 0])
            chosen, target = np.where(take, c, chosen), np.where(take, t, target)
            q["pdf"].append(pdf), q["contribution"].append(contrib), q["weight"].append(w)
        q = {k: np.stack(v) for k, v in q.items()}
        q["uc_weight"] = M.uc_weight(wsum, target, dt)
        rs2 = M.init_sampler(np.arange(n) % 64, np.arange(n) // 64, 0, 5, 0)
        offs = []
        for _ in range(4):
            rs2 = M.pcg4d(rs2)
            offs.append(M.neighbour_offsets(M.unit(rs2, dt)[:, :2], 8.0, dt))
        # neighbours: the record 1, 2, 3 and 4 places on, against the frustum size of a camera at `eye`
        inv = dt(1) / (dt(1.1547) * np.abs(M.dot(np.array([0.0, 0.6, 0.8], dtype=dt), eye.astype(dt) - s["pos"].astype(dt))))
        good = np.stack([M.neighbour_is_good(s, np.roll(s["pos"], k, 0), np.roll(s["flat_normal"], k, 0), inv, dt) for k in (1, 2, 3, 4)])
        prev = np.roll(s, 1)
        reuse = ~M.temporal_rejects(s, dict(pos=s["pos"] + f32(1e-3) * prev["pos"], mapped_normal=prev["mapped_normal"]), eye, dt)
        out[dt] = q, dict(offsets=np.stack(offs), good=good, reuse=reuse, chosen=chosen)
    (q32, d32), (q64, d64) = out[f32], out[f64]
    report = {}
    for k in q32:
        finite = np.isfinite(q64[k]) & np.isfinite(q32[k].astype(f64))
        rel = np.abs(q32[k].astype(f64) - q64[k])[finite].max() / np.abs(q64[k][finite]).max()
        report[k] = rel
        # section 20's measure and bound: 2^-12 of the largest value is 256 eps - a contribution is a few dozen roundings, and the GGX
        # distribution's squared denominator and the triangle sampler's differences amplify each by a small factor
        assert rel <= 2.0 ** -12, (k, rel)
    differ = np.zeros(n, dtype=bool)
    for k in d32:
        a, b = d32[k], d64[k]
        differ |= (a != b).reshape(-1, n).any(0) if a.shape[-1] == n else (a != b).reshape(a.shape[0], n, -1).any((0, 2))
    share = differ.mean()
    with capsys.disabled():
        print(f"\nrestir di model, float32 against float64 over {n} records: " + ", ".join(f"{k} {v:.2e}" for k, v in report.items()) +
              f"; pixels with a differing discrete decision {share:.3%}")
    assert d32["reuse"].any() and not d32["reuse"].all() and d32["good"].any() and not d32["good"].all()
    assert share <= 0.01


# =========================================================================================================================== GPU
def _room(S, size):
    """A small flat-shaded opaque room, open at the front and in its ceiling's front half (the sky shows through both): point lights of
    radius 0, one of them a spotlight, a sun with an angle and one without, an emissive quad on the left wall, two occluders that put
    part of the floor in every light's shadow.  Two cameras."""
    from test_estimator_consistency import _quad, _scene
    from tauray_amd.hdr import load_hdr
    grey = S.make_material(albedo=(0.7, 0.7, 0.7, 1), metallic=0.0, roughness=0.9)
    red = S.make_material(albedo=(0.8, 0.2, 0.15, 1), metallic=0.0, roughness=0.6)
    glossy = S.make_material(albedo=(0.3, 0.5, 0.8, 1), metallic=0.0, roughness=0.35)
    metal = S.make_material(albedo=(0.9, 0.7, 0.3, 1), metallic=1.0, roughness=0.5)
    glow = S.make_material(albedo=(0.2, 0.2, 0.2, 1), metallic=0.0, roughness=1.0, emission=(3.0, 2.0, 1.0))
    quads = [(*_quad(S, (-2, -1, -2), (0, 0, 4), (4, 0, 0)), grey),            # floor, normal +y
             (*_quad(S, (-2, -1, -2), (4, 0, 0), (0, 3, 0)), grey),            # back wall, normal +z
             (*_quad(S, (-2, -1, -2), (0, 3, 0), (0, 0, 4)), red),             # left wall, normal +x
             (*_quad(S, (2, -1, -2), (0, 0, 4), (0, 3, 0)), grey),             # right wall, normal -x
             (*_quad(S, (-2, 2, -2), (4, 0, 0), (0, 0, 2)), grey),             # the back half of a ceiling, normal -y
             (*_quad(S, (-1.99, -0.2, -1.2), (0, 1.0, 0), (0, 0, 1.2)), glow),  # emissive quad on the left wall, facing +x
             (*_quad(S, (0.2, -1, -0.6), (1.0, 0, 0.3), (0, 1.3, 0)), glossy),  # occluders
             (*_quad(S, (-1.2, -0.2, 0.2), (0, 0, 0.9), (0.9, 0, 0)), metal)]
    cams = []
    for eye in ((0.0, 0.6, 4.2), (0.9, 1.1, 3.9)):
        cam = S.Camera(fov=60, aspect=size[0] / size[1])
        m = np.eye(4)
        f = np.array([0.0, 0.1, 0.0]) - np.array(eye)
        f /= np.linalg.norm(f)
        r = np.cross(f, (0, 1, 0))
        r /= np.linalg.norm(r)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, np.cross(r, f), -f, eye
        cam.transform = m
        cams.append(cam)
    point = np.concatenate([S.make_point_light((6, 5, 4), (1.2, 1.4, 0.6), 0.0), S.make_point_light((2, 3, 5), (-1.0, 0.4, 1.2), 0.0),
                            S.make_spotlight((14, 13, 11), (0.3, 1.8, 0.9), (-0.2, -1.0, -0.4), 0.0, 35.0, 2.0)])
    directional = np.concatenate([S.make_directional_light((1.5, 1.4, 1.2), (-0.25, -1.0, -0.6), 3.0), S.make_directional_light((0.6, 0.7, 0.9), (0.3, -1.0, -0.9), 0.0)])
    return _scene(S, quads, cams, point_lights=point, directional_lights=directional, envmap=load_hdr(os.path.join(GOLDEN, "sky_flat.hdr")),
                  environment_factor=(0.6, 0.6, 0.6, 1.0))


def _lights_of(S, scene, ss):
    env = np.asarray(scene.envmap, dtype=np.float32)
    return M.Lights(point=scene.point_lights, tri=ss.tri_lights(), directional=scene.directional_lights, envmap=env, alias=S.build_alias_table(env),
                    environment_factor=scene.environment_factor)


class _Run:
    """`frames` frames of a recording stage over both viewports of the room: per frame the colour and every download."""
    NAMES = ("surface", "canonical", "history", "candidates", "temporal", "final")

    def __init__(self, R, ctx, ss, size, frames=3, viewports=(0, 1), **options):
        self.size, self.viewports, self.options = size, tuple(viewports), R.restir_di_options(record=True, **options)
        st = R.RestirDiStage(ctx, ss, size, len(self.viewports), self.options)
        out = ctx.alloc(size[0] * size[1] * 16 * len(self.viewports)).zero()
        self.frames = []
        for _ in range(frames):
            st.run(self.viewports, out)
            f = {n: st.download(n) for n in self.NAMES}
            if self.options["spatial_samples"]:
                f["spatial"] = st.download("spatial")
            f["color"] = out.download((len(self.viewports), size[1], size[0], 4))
            self.frames.append(f)
        self.timings = st.timings()
        st.close()
        out.free()


@pytest.fixture(scope="module")
def rooms(R, ctx):
    """The room at both sizes, uploaded on demand (one scene lives on the device at a time)."""
    from tauray_amd import scene as S
    scenes = {size: _room(S, size) for size in SIZES + ((64, 64),)}
    current = {}

    def get(size, as_strategy=0):
        if current.get("key") != (size, as_strategy):
            current["ss"] = R.SceneStage(ctx, scenes[size], as_strategy=as_strategy)
            current["key"] = (size, as_strategy)
        return scenes[size], current["ss"]
    return get


RUN_CASES = [((13, 7), dict(candidates=1, spatial_samples=0, temporal_reuse=False)), ((13, 7), dict(candidates=4, spatial_samples=2, temporal_reuse=True, search_radius=4.0)),
             ((13, 7), dict(candidates=32, spatial_samples=4, temporal_reuse=True, search_radius=3.0)), ((37, 19), dict(candidates=4, spatial_samples=4, temporal_reuse=False, search_radius=6.0)),
             ((37, 19), dict(candidates=1, spatial_samples=2, temporal_reuse=True, search_radius=8.0)), ((37, 19), dict(candidates=32, spatial_samples=0, temporal_reuse=True)),
             ((37, 19), dict(candidates=4, spatial_samples=3, temporal_reuse=True, search_radius=5.0, max_confidence=6.0))]


@pytest.fixture(scope="module")
def runs(R, ctx, rooms):
    """Every case of RUN_CASES rendered once; the tests below share the downloads and leave them unchanged."""
    cache = {}

    def get(i):
        if i not in cache:
            size, options = RUN_CASES[i]
            scene, ss = rooms(size)
            cache[i] = _Run(R, ctx, ss, size, rng_seed=11 + i, **options)
        return cache[i]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _light_split(light):
    return (light >> 30).astype(np.int64), (light & 0x3FFFFFFF).astype(np.int64)


@pytest.mark.gpu
def test_surface_record_and_miss_pixels(R, ctx, rooms):
    """The surface record is trhip_feature_render's position, normal and instance id and k_dshgi_indirect's material fields, bit for bit;
    a pixel without a surface has a null reservoir in both buffers and the direct stage's miss colour."""
    from tauray_amd import scene as S
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    glowing = 0
    for size in SIZES:
        scene, ss = rooms(size)
        w, h = size
        run = _Run(R, ctx, ss, size, frames=1, candidates=2, spatial_samples=1)
        f = run.frames[0]
        dist = DistributionParams(size, DISTRIBUTION_DUPLICATE, 0, 1, True)
        buf = ctx.alloc(w * h * 16)
        ds = R.DshgiStage(ctx, ss, size, 2, order=0, record_surface=True)
        texel = ctx.alloc(8).zero()
        ds.set_grids([S.ShGrid((1, 1, 1))], [texel])
        ds.set_instance_grids(np.full(len(scene.instances), -1, dtype=np.int32))
        table = ctx.alloc(8).zero()
        ds.set_brdf_integration(table, 1, 1)
        sink = ctx.alloc(w * h * 16 * 2)
        ds.run([0, 1], None, sink)
        dsurf = ds.download("surface")
        direct = R.DirectStage(ctx, ss, R.options_for_scene(scene), dist)
        dcol = ctx.alloc(w * h * 16 * 2).zero()
        direct.run(dcol, 2)
        dimg = dcol.download((2, h, w, 4))
        misses = 0
        for v in (0, 1):
            feats = {}
            for name, code in (("pos", R.FEATURE_WORLD_POS), ("normal", R.FEATURE_WORLD_NORMAL), ("id", R.FEATURE_INSTANCE_ID)):
                R.FeatureStage(ctx, ss, code, dist).run(buf, v)
                feats[name] = buf.download((h, w, 4))
            s = f["surface"][v]
            hit = s["instance_id"] >= 0
            assert (hit == ~np.isnan(feats["pos"][..., 0])).all() and hit.any() and not hit.all()
            assert (s["instance_id"][hit] == feats["id"][..., 0][hit].astype(np.int32)).all()
            assert (_bits(s["pos"][hit]) == _bits(feats["pos"][..., :3][hit])).all()
            assert (_bits(s["mapped_normal"][hit]) == _bits(feats["normal"][..., :3][hit])).all()
            for k in ("albedo", "metallic", "roughness", "f0", "transmittance", "view", "pos", "mapped_normal"):
                assert (_bits(s[k][hit]) == _bits(dsurf[v][k][hit])).all(), k
            # flat_normal and emission against the scene itself: instance i is quad i, four vertices each, flat-shaded
            quad = scene.vertices["pos"].astype(np.float64).reshape(-1, 4, 3)
            face = np.cross(quad[:, 1] - quad[:, 0], quad[:, 3] - quad[:, 0])
            face /= np.linalg.norm(face, axis=-1, keepdims=True)
            ids = s["instance_id"][hit]
            assert (np.abs(np.abs((s["flat_normal"][hit].astype(np.float64) * face[ids]).sum(-1)) - 1) < 1e-6).all()
            assert (np.abs(np.linalg.norm(s["flat_normal"][hit], axis=-1) - 1) < 1e-6).all()
            glow = ids == 5
            glowing += int(glow.sum())
            assert (s["emission"][hit][glow] == np.array([3.0, 2.0, 1.0], dtype=f32)).all() and (s["emission"][hit][~glow] == 0).all()
            miss = ~hit
            misses += int(miss.sum())
            assert (_bits(s[miss].view(np.uint32).reshape(-1, 28)[:, [0, 1, 2] + list(range(4, 28))]) == 0).all()
            for name in ("canonical", "history"):
                r = f[name][v][miss]
                assert (r["light"] == M.NULL_INDEX).all() and (r["uc_weight"] == 0).all() and (r["confidence"] == 0).all() and (r["target_function"] == 0).all()
            assert (_bits(f["color"][v][miss]) == _bits(dimg[v][miss])).all()
            assert (f["color"][v][..., 3] == 1).all() and np.isfinite(f["color"][v]).all()
        assert misses > 0
        for b in (buf, texel, table, sink, dcol):
            b.free()
        ds.close()
        direct.close()
    assert glowing > 0, "no pixel of either size sees the emissive quad"


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(RUN_CASES)))
def test_replay_of_the_decision_records_is_exact(runs, case):
    """From the decision records alone - weights, draws, targets, confidences - the float32 replay of update_reservoir, of the confidence
    sums and their clamp and of uc_weight gives the canonical and the history reservoir buffers bit for bit: every pixel, three frames
    (frame 0 has no history, frames 1 and 2 do)."""
    run = runs(case)
    o = run.options
    w, h = run.size
    reused = 0
    for fi, f in enumerate(run.frames):
        for v in range(len(run.viewports)):
            hit = f["surface"][v]["instance_id"] >= 0
            cand, temp = f["candidates"][v], f["temporal"][v]
            wsum = np.zeros((h, w), dtype=f32)
            target = np.zeros((h, w), dtype=f32)
            light = np.full((h, w), M.NULL_INDEX, dtype=np.uint32)
            data = np.zeros((h, w, 2), dtype=f32)
            conf = np.zeros((h, w), dtype=f32)
            for c in range(o["candidates"]):
                r = cand[..., c]
                t = M.luminance(r["contribution"] * r["visibility"][..., None], f32)
                wsum, take = M.update_reservoir(wsum, r["weight"], r["draw"])
                assert (take == (r["selected"] != 0))[hit].all()
                light, target = np.where(take, r["light"], light), np.where(take, t, target)
                data = np.where(take[..., None], r["light_data"], data)
                conf = conf + f32(1)
            ucw = M.uc_weight(wsum, target, f32)
            if o["temporal_reuse"]:
                reuse = temp["reuse"] != 0
                assert fi > 0 or not reuse.any()
                reused += int(reuse.sum())
                prev = run.frames[fi - 1]["history"][v] if fi else None
                if reuse.any():
                    py, px = np.where(reuse, temp["py"], 0), np.where(reuse, temp["px"], 0)
                    pr = prev[py, px]
                    assert (_bits(temp["prev_confidence"][reuse]) == _bits(pr["confidence"][reuse])).all()
                    wsum2, take = M.update_reservoir(wsum, temp["weight"], temp["draw"])
                    take &= reuse
                    assert (take == ((temp["selected"] != 0) & reuse)).all()
                    wsum = np.where(reuse, wsum2, wsum)
                    light, target = np.where(take, pr["light"], light), np.where(take, temp["target"], target)
                    data = np.where(take[..., None], pr["light_data"], data)
                    conf = np.where(reuse, conf + pr["confidence"], conf)
                    ucw = np.where(reuse, M.uc_weight(wsum, target, f32), ucw)
                conf = M.fmin2(conf, f32(o["max_confidence"]))
            can = f["canonical"][v]
            for name, got, want in (("uc_weight", can["uc_weight"], ucw), ("target_function", can["target_function"], target), ("light", can["light"], light),
                                    ("confidence", can["confidence"], conf), ("light_data", can["light_data"], data)):
                assert (_bits(got[hit]) == _bits(np.asarray(want)[hit])).all(), (fi, v, name)
            # the spatial kernel
            fin, his = f["final"][v], f["history"][v]
            if o["spatial_samples"]:
                wsum = np.zeros((h, w), dtype=f32)
                target = np.zeros((h, w), dtype=f32)
                light = np.full((h, w), M.NULL_INDEX, dtype=np.uint32)
                data = np.zeros((h, w, 2), dtype=f32)
                conf = np.zeros((h, w), dtype=f32)
                for k in range(o["spatial_samples"]):
                    r = f["spatial"][v][..., k]
                    held = (r["px"] >= 0) & hit
                    n = can[np.where(held, r["py"], 0), np.where(held, r["px"], 0)]
                    live = held & (n["light"] != M.NULL_INDEX)
                    wsum2, take = M.update_reservoir(wsum, r["wi"], r["draw"])
                    take &= live
                    assert (take == ((r["selected"] != 0) & live)).all()
                    wsum = np.where(live, wsum2, wsum)
                    light, target = np.where(take, n["light"], light), np.where(take, r["target_n"], target)
                    data = np.where(take[..., None], n["light_data"], data)
                    conf = np.where(held, conf + n["confidence"], conf)
                wsum, take = M.update_reservoir(wsum, fin["wi"], fin["draw"])
                assert (take == (fin["selected"] != 0))[hit].all()
                light, target = np.where(take, can["light"], light), np.where(take, can["target_function"], target)
                data = np.where(take[..., None], can["light_data"], data)
                conf = conf + can["confidence"]
                ucw = M.uc_weight(wsum, target, f32)
            else:
                light, target, data, conf, ucw = can["light"], can["target_function"], can["light_data"], can["confidence"], can["uc_weight"]
            for name, got, want in (("uc_weight", his["uc_weight"], ucw), ("target_function", his["target_function"], target), ("light", his["light"], light),
                                    ("confidence", his["confidence"], conf), ("light_data", his["light_data"], data)):
                assert (_bits(got[hit]) == _bits(np.asarray(want)[hit])).all(), (fi, v, name)
            # out = contribution * uc_weight + emission, from the records
            want = (fin["contribution"] * fin["visibility"][..., None]) * his["uc_weight"][..., None] + f["surface"][v]["emission"]
            assert (_bits(f["color"][v][..., :3][hit]) == _bits(want.astype(f32)[hit])).all() and (f["color"][v][..., 3] == 1).all()
    if o["temporal_reuse"]:
        assert reused > 0, "no pixel of the static room reused its history"


def _model_frame(S, run, scene, L, fi, v, dt):
    """The model's own canonical and spatial pass of frame `fi`, viewport `v`, at `dt`: the inputs are the downloaded surface records,
    the light tables, the recorded visibilities, the previous frame's history and this frame's canonical reservoirs.  Flat arrays over
    the pixels with a surface (`ys`, `xs`)."""
    o, f = run.options, run.frames[fi]
    w, h = run.size
    surf = f["surface"][v]
    ys, xs = np.nonzero(surf["instance_id"] >= 0)
    s = surf[ys, xs]
    cam = scene.camera_data()[run.viewports[v]]
    origin = cam["origin"][:3]
    out = dict(ys=ys, xs=xs)
    rs = M.init_sampler(xs, ys, run.viewports[v], 2 * fi, o["rng_seed"])
    prev_conf = np.zeros(len(s), dtype=dt)
    if o["temporal_reuse"]:
        rs = M.pcg4d(rs)
        rx, ry = M.reprojected_pixel(cam["view_proj"], s["pos"], run.size, M.unit(rs, dt)[:, :2], dt)
        on = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
        reuse = np.zeros(len(s), dtype=bool)
        if fi:
            ps = run.frames[fi - 1]["surface"][v][np.where(on, ry, 0), np.where(on, rx, 0)]
            reuse = on & ~M.temporal_rejects(s, ps, origin, dt)
            ph = run.frames[fi - 1]["history"][v][np.where(on, ry, 0), np.where(on, rx, 0)]
            prev_conf = np.where(reuse, ph["confidence"], 0).astype(dt)
        out.update(rx=rx, ry=ry, reuse=reuse)
    cand = f["candidates"][v][ys, xs]
    q = dict(type=[], index=[], data=[], pdf=[], contribution=[], weight=[], draw=[])
    mis = dt(1) / (dt(o["candidates"]) + prev_conf)
    for c in range(o["candidates"]):
        rs = M.pcg4d(rs)
        typ, idx, data, pdf = M.sample_canonical(L, rs, s["pos"], o["min_ray_dist"], dt)
        contrib = M.light_contribution(L, typ, idx, data, s, dt)[0]
        t = M.luminance(contrib * cand["visibility"][:, c].astype(dt)[:, None], dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            wgt = M.nan_to_zero(mis * t / pdf)
        rs = M.pcg4d(rs)
        for k, val in zip(q, (typ, idx, data, pdf, contrib, wgt, M.unit(rs, dt)[:, 0])):
            q[k].append(val)
    out.update({k: np.stack(val, 1) for k, val in q.items()})
    if o["temporal_reuse"] and fi:
        pt, pi = _light_split(ph["light"])
        t = M.luminance(M.light_contribution(L, pt, pi, ph["light_data"], s, dt)[0], dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["temporal_target"] = t
            out["temporal_weight"] = M.nan_to_zero(((ph["confidence"].astype(dt) / (dt(o["candidates"]) + ph["confidence"].astype(dt))) * t) * ph["uc_weight"].astype(dt))
        rs = M.pcg4d(rs)
        out["temporal_draw"] = M.unit(rs, dt)[:, 0]
    # ---- spatial
    K = o["spatial_samples"]
    can = f["canonical"][v]
    c = can[ys, xs]
    ct, ci = _light_split(c["light"])
    if K:
        rs = M.init_sampler(xs, ys, run.viewports[v], 2 * fi + 1, o["rng_seed"])
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
        total = c["confidence"].astype(dt)
        # the continuous quantities follow the STAGE's slots (the discrete test compares the slots themselves)
        held = srec["px"] >= 0
        nres = can[np.where(held, srec["py"], 0), np.where(held, srec["px"], 0)]
        for k in range(K):
            total = np.where(held[:, k], total + nres["confidence"][:, k].astype(dt), total)
        with np.errstate(invalid="ignore", divide="ignore"):
            canonical_m = c["confidence"].astype(dt) / total
        # the tail of the spatial stream: one draw per held slot whose neighbour's sample is not null, in slot order, then the canonical merge's
        live = held & (nres["light"] != M.NULL_INDEX)
        draws = []
        for k in range(K):
            rs = np.where(live[:, k, None], M.pcg4d(rs), rs)
            draws.append(M.unit(rs, dt)[:, 0])
        rs = M.pcg4d(rs)
        out.update(spatial_live=live, spatial_draw=np.stack(draws, 1), final_draw=M.unit(rs, dt)[:, 0])
        sq = dict(target_n=[], jacobian_n=[], m=[], wi=[], target_c=[], jacobian_c=[], mis_canonical=[])
        for k in range(K):
            n = nres[:, k]
            nsurf = surf[np.where(held[:, k], srec["py"][:, k], 0), np.where(held[:, k], srec["px"][:, k], 0)]
            nt, ni = _light_split(n["light"])
            contrib, ldir, d2, lnorm = M.light_contribution(L, nt, ni, n["light_data"], s, dt)
            tn = M.luminance(contrib * srec["visibility_n"][:, k].astype(dt)[:, None], dt)
            with np.errstate(invalid="ignore", over="ignore"):
                x = s["pos"].astype(dt) + ldir * np.sqrt(d2)[:, None]
                jn = np.where(nt > 1, dt(1), M.jacobian(nsurf["pos"].astype(dt), s["pos"].astype(dt), x, lnorm, dt))
                m = M.mis_noncanonical(c["confidence"].astype(dt), n["confidence"].astype(dt), total, n["target_function"].astype(dt), tn, jn, dt)
                wi = M.nan_to_zero(((tn * m) * n["uc_weight"].astype(dt)) * jn)
            contrib, ldir, d2, lnorm = M.light_contribution(L, ct, ci, c["light_data"], nsurf, dt)
            tc = M.luminance(contrib * srec["visibility_c"][:, k].astype(dt)[:, None], dt)
            with np.errstate(invalid="ignore", over="ignore"):
                x = nsurf["pos"].astype(dt) + ldir * np.sqrt(d2)[:, None]
                jc = np.where(ct > 1, dt(1), M.jacobian(s["pos"].astype(dt), nsurf["pos"].astype(dt), x, lnorm, dt))
                mc = M.mis_canonical(c["confidence"].astype(dt), n["confidence"].astype(dt), total, c["target_function"].astype(dt), tc, jc, dt)
            live = held[:, k] & (n["light"] != M.NULL_INDEX)
            cl = held[:, k] & (c["light"] != M.NULL_INDEX)
            canonical_m = np.where(cl, canonical_m + mc, canonical_m)
            for key, val, mask in (("target_n", tn, live), ("jacobian_n", jn, live), ("m", m, live), ("wi", wi, live), ("target_c", tc, cl), ("jacobian_c", jc, cl),
                                   ("mis_canonical", mc, cl)):
                sq[key].append(np.where(mask, val, dt(0)))
        out.update({k: np.stack(val, 1) for k, val in sq.items()})
        out["canonical_m"] = canonical_m
        out["final_wi"] = M.nan_to_zero((canonical_m * c["target_function"].astype(dt)) * c["uc_weight"].astype(dt))
    his = f["history"][v][ys, xs]
    ht, hi = _light_split(his["light"])
    out["final_contribution"] = M.light_contribution(L, ht, hi, his["light_data"], s, dt)[0]
    return out


@pytest.fixture(scope="module")
def modelled(runs, rooms):
    """The model's frames of a run at both precisions, computed once."""
    from tauray_amd import scene as S
    cache = {}

    def get(case):
        if case not in cache:
            run = runs(case)
            scene, ss = rooms(run.size)
            L = _lights_of(S, scene, ss)
            cache[case] = {(fi, v): (_model_frame(S, run, scene, L, fi, v, f32), _model_frame(S, run, scene, L, fi, v, f64))
                           for fi in range(len(run.frames)) for v in range(len(run.viewports))}
        return cache[case]
    return get


MODEL_CASES = tuple(range(len(RUN_CASES)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODEL_CASES)
def test_draws_and_picks_are_exact(runs, modelled, case):
    """The model's own pcg4d streams give every recorded selection draw - the candidates', the temporal merge's, and in the spatial stream,
    after its 2 * spatial_samples offsets, one per slot that holds a neighbour whose sample is not null and one for the canonical merge -,
    every candidate's light class and index, and light_data of point and directional candidates, bit for bit.  A slot without a draw
    records 0."""
    run = runs(case)
    classes = set()
    for (fi, v), (m32, m64) in modelled(case).items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        cand = f["candidates"][v][ys, xs]
        assert (_bits(cand["draw"]) == _bits(m32["draw"])).all()
        t, i = _light_split(cand["light"])
        assert (t == m32["type"]).all() and (i == m32["index"]).all()
        exact = (t == 0) | (t == 2)
        assert (_bits(cand["light_data"][exact]) == _bits(m32["data"][exact])).all()
        classes |= set(np.unique(t).tolist())
        if "temporal_draw" in m32:
            reuse = f["temporal"][v][ys, xs]["reuse"] != 0
            assert (_bits(f["temporal"][v][ys, xs]["draw"][reuse]) == _bits(m32["temporal_draw"][reuse])).all()
        if "spatial_draw" in m32:
            srec, live = f["spatial"][v][ys, xs], m32["spatial_live"]
            assert live.any() and (_bits(srec["draw"][live]) == _bits(m32["spatial_draw"][live])).all() and (_bits(srec["draw"][~live]) == 0).all()
            assert (_bits(f["final"][v][ys, xs]["draw"]) == _bits(m32["final_draw"])).all()
    assert classes == {0, 1, 2, 3}, f"the room's candidates cover the classes {classes}"


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=f64)).astype(f32)).astype(f64)


def _bounded(name, got, m32, m64, keep, failures):
    """|stage - float64 model| <= 4 |float32 model - float64 model| + one float32 ulp of the value's magnitude"""
    got, a, b = (np.asarray(x, dtype=f64) for x in (got, m32, m64))
    keep = np.broadcast_to(keep.reshape(keep.shape + (1,) * (got.ndim - keep.ndim)), got.shape) & np.isfinite(b) & np.isfinite(got)
    err, bound = np.abs(got - b), 4 * np.abs(a - b) + _ulp32(np.maximum(np.abs(b), np.abs(got)))
    bad = keep & (err > bound)
    worst = float((err / bound)[keep].max()) if keep.any() else 0.0
    if bad.any():
        failures.append(f"{name}: {int(bad.sum())} of {int(keep.sum())} values past the bound, largest error / bound {worst:.2f}")
    return worst


def _discrete_mismatch(run, fi, v, m32, m64):
    """Pixels (flat, over the surface pixels) whose rounding-dependent decisions the model's own two precisions disagree on."""
    differ = np.zeros(len(m32["ys"]), dtype=bool)
    if "rx" in m32:
        differ |= (m32["rx"] != m64["rx"]) | (m32["ry"] != m64["ry"]) | (m32["reuse"] != m64["reuse"])
    if "slots" in m32:
        differ |= (m32["slots"] != m64["slots"]).any((1, 2))
    return differ


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODEL_CASES)
def test_continuous_quantities_are_bounded(runs, modelled, case, capsys):
    """pdfs, triangle light_data, unshadowed contributions, Jacobians, MIS terms and weights, recomputed by the model from the downloaded
    surface records, the scene's light tables and the recorded visibilities: section 19's bound.

    The kernels take sin, cos, pow and atan2 of the resampling code as the double function rounded once (RoundedMath, csrc/common.h), which
    is what the model's float32 does: measured on an MI355X the largest error / bound is 0.25 for every quantity, the figure of a stage
    that has the float32 model's bits.  With the device library's sinf / cosf / powf / atan2f instead, 0.1 ... 0.5 % of the triangle-light
    and environment values missed the bound, triangle light_data by up to 107."""
    run = runs(case)
    failures, worst = [], {}
    for (fi, v), (m32, m64) in modelled(case).items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        every = np.ones(len(ys), dtype=bool)
        cand = f["candidates"][v][ys, xs]
        checks = [("pdf", cand["pdf"], m32["pdf"], m64["pdf"], every), ("contribution", cand["contribution"], m32["contribution"], m64["contribution"], every),
                  ("weight", cand["weight"], m32["weight"], m64["weight"], every), ("light_data", cand["light_data"], m32["data"], m64["data"], every)]
        temp = f["temporal"][v][ys, xs]
        if "temporal_weight" in m32:
            # the reuse bit is the stage's; where the model's precisions disagree on the pixel, the history sample is another one
            same = (temp["reuse"] != 0) & (temp["px"] == m32["rx"]) & (temp["py"] == m32["ry"]) & (m32["rx"] == m64["rx"]) & (m32["ry"] == m64["ry"])
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
        print(f"\nrestir di case {case}: largest error / bound: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODEL_CASES)
def test_discrete_decisions_match_where_the_precisions_agree(runs, modelled, case, capsys):
    """Neighbour pixels, good / bad bits, the reprojected pixel and its reuse bit: a pixel where the model's own float32 and float64
    disagree on any of them is left out, at most 1 % of a frame may be; on every other pixel the stage's decisions are the model's."""
    run = runs(case)
    counts = []
    for (fi, v), (m32, m64) in modelled(case).items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        out = _discrete_mismatch(run, fi, v, m32, m64)
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
        print(f"\nrestir di case {case}: pixels left out of the discrete comparison per frame and viewport: {counts}")


@pytest.mark.gpu
def test_a_changed_viewport_list_is_refused_while_there_is_history(R, ctx, rooms):
    """History is kept per layer: with temporal reuse another list on a later frame is refused until reset; without, it is rendered."""
    size = SIZES[0]
    scene, ss = rooms(size)
    out = ctx.alloc(size[0] * size[1] * 16 * 2).zero()
    for temporal in (True, False):
        st = R.RestirDiStage(ctx, ss, size, 2, R.restir_di_options(candidates=1, spatial_samples=0, temporal_reuse=temporal))
        st.run((0, 1), out)
        if temporal:
            for other in ((1, 0), (0,)):
                with pytest.raises(R.TrhipError) as e:
                    st.run(other, out)
                assert "trhip_restir_di_render" in str(e.value) and "viewport list differs" in str(e.value)
            st.run((0, 1), out)
            st.reset()
        st.run((1, 0), out)
        st.close()
    out.free()


def _frames(R, ctx, ss, size, viewports, frames, stage=None, **options):
    st = stage or R.RestirDiStage(ctx, ss, size, len(viewports), R.restir_di_options(**options))
    out = ctx.alloc(size[0] * size[1] * 16 * len(viewports)).zero()
    imgs = []
    for _ in range(frames):
        st.run(viewports, out)
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
    opts = dict(candidates=4, spatial_samples=3, temporal_reuse=True, search_radius=6.0, rng_seed=5)
    scene, ss = rooms(size)
    a, ha = _frames(R, ctx, ss, size, [0, 1], 3, **opts)
    b, hb = _frames(R, ctx, ss, size, [0, 1], 3, **opts)
    assert (_bits(a) == _bits(b)).all() and (_bits(ha.view(np.uint32)) == _bits(hb.view(np.uint32))).all(), "two fresh runs differ"
    assert not (_bits(a[0]) == _bits(a[1])).all(), "the frames of a sequence draw the same numbers"
    # reset, then a frame = the first frame of a new stage
    st = R.RestirDiStage(ctx, ss, size, 2, R.restir_di_options(**opts))
    c = _frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    st.reset()
    d = _frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    st.close()
    assert (_bits(c) == _bits(a[:2])).all() and (_bits(d) == _bits(a[:2])).all(), "reset does not forget the history"
    # one stage rendering viewports (0, 1) = two stages rendering one each
    for v in (0, 1):
        e, _ = _frames(R, ctx, ss, size, [v], 3, **opts)
        assert (_bits(e[:, 0]) == _bits(a[:, v])).all(), f"viewport {v} alone differs"
    # both acceleration-structure layouts
    for strategy in (1, 2):
        scene, ss2 = rooms(size, as_strategy=strategy)
        g, hg = _frames(R, ctx, ss2, size, [0, 1], 3, **opts)
        assert (_bits(g) == _bits(a)).all() and (_bits(hg.view(np.uint32)) == _bits(ha.view(np.uint32))).all(), f"acceleration-structure strategy {strategy} differs"
    rooms(size, as_strategy=0)


@pytest.mark.gpu
def test_a_list_longer_than_one_launch(R):
    """65 viewports are two launches a pass, of 64 and of 1: layer 64 is layer 0 of a one-entry list of its viewport and layer 63 repeats
    layer 0 (the sampler is seeded by the viewport, and without temporal reuse one frame has no history), bit for bit - colour, surface
    record, canonical and history reservoirs.  17 x 9 pixels leave the tile partial on both axes."""
    from tauray_amd import scene as S
    size = (17, 9)
    own = R.Context(0)      # the module's context holds the scene of `rooms`
    ss = R.SceneStage(own, _room(S, size), as_strategy=0)

    def frame(views):
        st = R.RestirDiStage(own, ss, size, len(views), R.restir_di_options(candidates=4, spatial_samples=2, temporal_reuse=False, search_radius=4.0, rng_seed=3))
        out = own.alloc(size[0] * size[1] * 16 * len(views)).zero()
        st.run(views, out)
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


EXPECTATION_CASES = {
    "1 candidate, no reuse": (dict(candidates=1, spatial_samples=0, temporal_reuse=False), 1, 64),
    "8 candidates, no reuse": (dict(candidates=8, spatial_samples=0, temporal_reuse=False), 1, 24),
    "4 candidates, temporal reuse, frame 8": (dict(candidates=4, spatial_samples=0, temporal_reuse=True), 9, 24),
    "4 candidates, 2 spatial samples at radius 8": (dict(candidates=4, spatial_samples=2, temporal_reuse=False, search_radius=8.0), 1, 24),
    "4 candidates, temporal reuse, 3 spatial samples, frame 8": (dict(candidates=4, spatial_samples=3, temporal_reuse=True, search_radius=8.0), 9, 24),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXPECTATION_CASES))
def test_same_expectation_as_the_direct_stage(R, ctx, rooms, name, capsys):
    """The room at 64 x 64, K = 16 independent sequences with their own rng_seed, judged by test_estimator_consistency's _assert_same_mean
    with its z values, outlier share and bias floor as they are: the direct stage at 64 spp against ReSTIR DI.  A batch is the mean over
    enough seeds that its standard error is a few per cent of the mean."""
    from test_estimator_consistency import _assert_same_mean, _dup
    size, K = (64, 64), 16
    scene, ss = rooms(size)
    options, frames, seeds = EXPECTATION_CASES[name]
    direct = R.DirectStage(ctx, ss, R.options_for_scene(scene, samples_per_pixel=64, samples_per_pass=1), _dup(size))
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    base = np.zeros((K, size[1], size[0], 3))
    for k in range(K):
        direct.reset_accumulated_samples()
        direct.run(buf)
        base[k] = buf.download((size[1], size[0], 4))[..., :3]
    direct.close()
    got = np.zeros((K, size[1], size[0], 3))
    seed = 1
    for k in range(K):
        for _ in range(seeds):
            st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(rng_seed=seed, **options))
            seed += 1
            for _f in range(frames):
                st.run([0], buf)
            got[k] += buf.download((size[1], size[0], 4))[..., :3] / seeds
            st.close()
    buf.free()
    assert np.isfinite(got).all()
    se = got.mean((1, 2)).std(0, ddof=1) / math.sqrt(K) / got.mean((0, 1, 2))
    rel, z = _assert_same_mean(base, got, name)
    with capsys.disabled():
        print(f"\nrestir di against the direct stage, {name}: image means differ by {rel:.3%} ({z:.2f} standard errors), standard error of a batch mean {se.max():.2%}")
    assert (se * math.sqrt(K) < 0.05).all(), "a batch is too noisy to say anything"


@pytest.mark.gpu
def test_the_feature_earns_its_keep(R, ctx, capsys):
    """sponza_lights with 64 lights at 128 x 72: the mean squared error against a converged direct-stage image (4096 spp) of frame 8 with
    the defaults (4 candidates, 2 spatial samples, temporal reuse) is strictly lower than the direct stage's at 4 samples per pixel, both
    averaged over the same 8 seeds."""
    from tauray_amd import scenes
    from test_estimator_consistency import _dup
    size = (128, 72)
    scene = scenes.sponza_lights(64, 1, *size)
    ss = R.SceneStage(ctx, scene)
    buf = ctx.alloc(size[0] * size[1] * 16).zero()

    def direct(spp, seed):
        st = R.DirectStage(ctx, ss, R.options_for_scene(scene, samples_per_pixel=spp, samples_per_pass=1, rng_seed=seed), _dup(size))
        st.run(buf)
        img = buf.download((size[1], size[0], 4))[..., :3].astype(f64)
        st.close()
        return img
    ref = direct(4096, 999)
    mse_restir = mse_direct = 0.0
    for seed in range(1, 9):
        st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(rng_seed=seed, min_ray_dist=scene_min_ray_dist(R, scene)))
        for _ in range(9):
            st.run([0], buf)
        img = buf.download((size[1], size[0], 4))[..., :3].astype(f64)
        st.close()
        mse_restir += np.mean((img - ref) ** 2) / 8
        mse_direct += np.mean((direct(4, seed) - ref) ** 2) / 8
    buf.free()
    with capsys.disabled():
        print(f"\nrestir di on {scene.name} at {size[0]} x {size[1]}: MSE against 4096 spp: frame 8 of the defaults {mse_restir:.4e}, direct stage at 4 spp {mse_direct:.4e}, "
              f"ratio {mse_restir / mse_direct:.3f}")
    assert mse_restir < mse_direct


def scene_min_ray_dist(R, scene):
    return float(R.options_for_scene(scene).min_ray_dist)


def _raw(path, shape):
    return np.fromfile(path, dtype=np.float32).reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["still", "camera grid", "animation"])
def test_both_hosts_render_the_same_frames(R, ctx, tmp_path, which):
    """tauray_hip --renderer=restir-di against the Python RestirDiRenderer: three frames at 96 x 96 as .raw, bit for bit - test.glb, the
    same under a 2 x 1 camera grid, and animated.glb under --animation (the temporal path over moving geometry); -t names both kernels."""
    from tauray_amd import scene as S
    from tauray_amd.gltf import load_glb
    from tauray_amd.animation import SceneAnimator
    size, frames = (96, 96), 3
    glb = os.path.join(GOLDEN, "animated.glb" if which == "animation" else "test.glb")
    prefix = str(tmp_path / "cpp")
    args = [CLI, glb, "--renderer=restir-di", "--restir=4,2,16,16,on", f"--width={size[0]}", f"--height={size[1]}", f"--frames={frames}", "--filetype=raw", "--format=rgba32",
            "--rng-seed=3", "-t", "--headless=" + prefix]
    if which == "camera grid":
        args.append("--camera-grid=2,1,0.1,0.1")
    if which == "animation":
        args.append("--animation")
    p = subprocess.run(args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "[restir di canonical]" in p.stdout and "[restir di spatial]" in p.stdout
    scene = load_glb(glb, *size)
    if which == "camera grid":
        scene.cameras = S.generate_camera_grid(scene.cameras[0], 2, 1, 0.1, 0.1, 5.0)
    views = max(len(scene.cameras), 1)
    ss = R.SceneStage(ctx, scene)
    animator = None
    if which == "animation":
        animator = SceneAnimator(scene)
        animator.play("")
    rr = R.RestirDiRenderer(ctx, ss, scene, size, R.restir_di_options(candidates=4, spatial_samples=2, search_radius=16.0, max_confidence=16.0, temporal_reuse=True, rng_seed=3,
                                                                       min_ray_dist=scene_min_ray_dist(R, scene)))
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
    assert t["canonical_name"] == "restir di canonical" and t["spatial_name"] == "restir di spatial" and t["frames"] == frames and t["total_ms"] > 0
    rr.close()
