"""ReSTIR DI's sphere lights as area lights (trhip_restir_di_set_sphere_lights; restir_di.h `sphere lights`; tauray_amd/csrc/
restir_di_sphere.{h,hip}).

CPU: the ABI, the refusals of Python and of the command line, the host sanitizers' program, and the numpy model of the rule
(tests/restir_di_sphere_model.py over tests/restir_di_model.py): the octahedral map, the sampler against its pdf, the closed form of a
sphere above a Lambertian receiver, the Jacobian against finite differences, the corners, float32 against float64.  GPU: the three
set-ups that must be the same bits, the replay of recorded frames, point mode's image as area mode's expectation, the direct stage's
expectation, the penumbra, stage behaviour, both hosts.  The bounds on recorded quantities are test_restir_di.py's own comparisons,
called as they are with the area mode's model in restir_di_model's place."""
import math
import os
import subprocess

import numpy as np
import pytest

import restir_di_model as M
import restir_di_selection_model as SM
import restir_di_sphere_model as A
import restir_di_visibility_model as VM
import test_restir_di as T
import test_restir_di_bsdf_candidates as TB
import test_restir_di_visibility as V
from conftest import GOLDEN, ROOT
from test_restir_di import SIZES, _bits, _light_split, _lights_of, _plane_surface, _raw, _room, scene_min_ray_dist

f32, f64 = np.float32, np.float64
CLI = os.path.join(ROOT, "tauray_amd", "tauray_hip")


@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


# =========================================================================================================================== CPU
def test_symbol_and_defines(R, tmp_path):
    from tauray_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "trhip_restir_di_set_sphere_lights") and "trhip_restir_di_set_sphere_lights" in _lib.SYMBOLS
    src = tmp_path / "defines.c"
    src.write_text('#include <stdio.h>\n#include "trhip.h"\nint main(void) {\n'
                   '    int (*f)(trhip_restir_di*, int) = trhip_restir_di_set_sphere_lights;\n    (void)f;\n'
                   '    printf("%d %d %zu\\n", TRHIP_RESTIR_SPHERE_LIGHTS_POINT, TRHIP_RESTIR_SPHERE_LIGHTS_AREA, sizeof(trhip_restir_di_options));\n'
                   "    return 0;\n}\n")
    exe = str(tmp_path / "defines")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip",
                    "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["0", "1", "32"]
    assert _lib.RESTIR_SPHERE_LIGHTS == {"point": 0, "area": 1}
    for mode in (0, 1, 7):      # the null stage is refused ahead of the mode
        assert L.trhip_restir_di_set_sphere_lights(None, mode) != 0
        assert "trhip_restir_di_set_sphere_lights: null stage" in L.trhip_last_error().decode()


def test_python_option_refuses_by_name(R):
    assert R.restir_di_options()["sphere_lights"] == "point" and R.restir_di_options(sphere_lights="area")["sphere_lights"] == "area"
    for name in ("sphere", "Area", 1, None):
        with pytest.raises(ValueError) as e:
            R.restir_di_options(sphere_lights=name)
        assert f"unknown ReSTIR DI sphere lights mode {name!r} (point, area)" in str(e.value)
    with pytest.raises(AttributeError):
        R.restir_di_options(sphere_light="area")


@pytest.mark.parametrize("args, text", [
    (["--renderer=restir-di", "--restir-sphere-lights=disc"], "--restir-sphere-lights: disc is neither point nor area"),
    (["--renderer=restir-gi", "--restir-sphere-lights="], "--restir-sphere-lights:  is neither point nor area"),
    (["--restir-sphere-lights=area"], "--restir-sphere-lights sets how --renderer=restir-di lights a point light that has a radius"),
    (["--renderer=direct", "--restir-sphere-lights=point"], "--restir-sphere-lights sets how --renderer=restir-di lights a point light that has a radius"),
])
def test_cli_refuses_and_helps(args, text):
    p = subprocess.run([CLI] + args + [os.path.join(GOLDEN, "test.glb"), "--width=16", "--height=16", "--filetype=none"], capture_output=True, text=True)
    assert p.returncode != 0 and text in p.stderr, p.stderr
    usage = subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
    assert "--restir-sphere-lights=point|area   (point)" in usage


def test_host_option_checks_under_the_sanitizers(tmp_path):
    """tests/restir_sphere_lights_check.cc: the flag's parser and the C++ options check, built with the address and undefined-behaviour
    sanitizers as test_restir_di.py builds its program, no device."""
    exe = str(tmp_path / "restir_sphere_lights_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "restir_sphere_lights_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)

    def run(*a):
        p = subprocess.run([exe] + list(a), capture_output=True, text=True)
        return p.returncode, p.stdout.strip(), p.stderr.strip()
    assert run("default") == (0, "0", "") and run("parse", "point") == (0, "0", "") and run("parse", "area") == (0, "1", "")
    assert run("check", "0") == (0, "ok", "") and run("check", "1") == (0, "ok", "")
    for a, why in ((("parse", "AREA"), "--restir-sphere-lights: AREA is neither point nor area"), (("parse", ""), "is neither point nor area"),
                   (("parse", "1"), "1 is neither point nor area"), (("check", "2"), "restir-di: sphere_lights 2 is outside 0..1"),
                   (("check", "-1"), "restir-di: sphere_lights -1 is outside 0..1")):
        rc, out, err = run(*a)
        assert rc == 1 and why in err, (a, err)


# ---- the model
def _unit_vectors(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_octahedral_round_trip(capsys):
    """10^5 seeded unit vectors, the six axes and the z = 0 seam through encode and decode: every vector comes back within four times the
    float32 model's own largest deviation from the float64 model.  The float64 model's own error is rounding (1e-15), so that relative
    bound says little more than that no vector is an outlier; the working bound is the absolute one: the float32 error is a few roundings
    (a dozen operations of 2^-24 each on components of at most 1), below 2^-20."""
    seam = np.stack([np.cos(np.linspace(0, 2 * np.pi, 257)), np.sin(np.linspace(0, 2 * np.pi, 257)), np.zeros(257)], -1)
    seam_below = seam + np.array([0, 0, -1e-9])
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    n = np.concatenate([_unit_vectors(100_000, 29), axes, seam, seam_below / np.linalg.norm(seam_below, axis=-1, keepdims=True)])
    back64 = A.oct_decode(A.oct_encode(n, f64), f64)
    back32 = A.oct_decode(A.oct_encode(n.astype(f32), f32), f32)
    assert back32.dtype == f32 and A.oct_encode(n.astype(f32), f32).dtype == f32
    assert np.abs(back64 - n).max() < 1e-15 * 8
    p = A.oct_encode(n, f64)
    assert (np.abs(p) <= 1).all() and np.isfinite(p).all()
    bound = 4 * np.abs(back32.astype(f64) - back64).max()
    err = np.abs(back32.astype(f64) - n).max()
    with capsys.disabled():
        print(f"\nsphere lights, octahedral round trip over {len(n)} vectors: float32 error {err:.3e}, bound (4 x float32 against float64 model) {bound:.3e}")
    assert err <= bound and err < 2.0 ** -20
    # the axes and the seam come back exactly in float64: their encodings are exact
    assert (A.oct_decode(A.oct_encode(axes, f64), f64) == axes).all()
    # sign(0) = 1: the lower half's fold of a vector with a zero component stays finite and on the square's rim
    low = A.oct_encode(np.array([[0.0, 0.0, -1.0], [0.0, -0.6, -0.8], [-0.6, 0.0, -0.8]]), f64)
    assert (low[0] == (1, 1)).all() and np.isfinite(low).all()


def _sphere_light(S, colour, pos, radius, spot=None):
    if spot is None:
        return S.make_point_light(colour, pos, radius)
    return S.make_spotlight(colour, pos, spot[0], radius, spot[1], spot[2])


def _draws(n, seed):
    return M.pcg4d(M.init_sampler(np.arange(n) % 256, np.arange(n) // 256, 0, 0, seed))


@pytest.mark.parametrize("ratio", [0.05, 0.3, 0.7, 0.95, 0.999])
def test_sampler_agrees_with_its_pdf(ratio, capsys):
    """Receivers outside the sphere at r / d = ratio: the mean of 1 / solid_pdf over the draws is the cap's solid angle
    2 pi (1 - cutoff) - no draw takes the guard -, the directions are uniform in the cone (the mean cosine to the axis is
    (1 + cutoff) / 2, 4 standard errors), and every drawn point has dot(n, dir) < 0 and lies on the sphere to rounding:
    b^2 - dist2 + r^2 carries an absolute error of about 3 eps dist2, the square root of a quantity clamped at 0 turns an error e into at
    most sqrt(e), so the point is off the sphere by less than 2 sqrt(eps) d; the test allows 4 sqrt(eps) d."""
    from tauray_amd import scene as S
    n, r = 40_000, 0.8
    d = r / ratio
    pl = np.repeat(_sphere_light(S, (1, 1, 1), (0.3, 1.0, -0.2), r), n)
    centre = pl["pos"][0].astype(f64)
    axis = np.array([0.48, -0.6, 0.64])
    pos = np.broadcast_to(centre + d * axis, (n, 3))
    for dt in (f32, f64):
        u = M.unit(_draws(n, 3), dt)[:, 1:3]
        nrm, pdf, direction, length = A.sphere_point(pl, pos, u, 1e-4, dt)
        cutoff = math.sqrt(1 - ratio * ratio)
        cap = 2 * math.pi * (1 - cutoff)
        assert (pdf < 1e8).all(), "a draw took the guard"
        # TR_PI has twelve digits and the light's record is float32: 1e-6; 1 - cutoff cancels for a small cap: a few eps / (1 - cutoff)
        assert abs(np.mean(1 / pdf.astype(f64)) / cap - 1) < 1e-6 + 8 * np.finfo(dt).eps / (1 - cutoff)
        cos_axis = -(direction.astype(f64) @ axis)
        want, se = (1 + cutoff) / 2, cos_axis.std(ddof=1) / math.sqrt(n)
        assert abs(cos_axis.mean() - want) <= 4 * se + 1e-6, (cos_axis.mean(), want, se)
        assert (cos_axis >= cutoff - 1e-5).all()
        assert ((nrm.astype(f64) * direction.astype(f64)).sum(-1) < 0).all()
        x = pos + direction.astype(f64) * length.astype(f64)[:, None]
        off = np.abs(np.linalg.norm(x - centre, axis=-1) - r).max()
        assert off <= 4 * math.sqrt(np.finfo(dt).eps) * d, (dt, off)
        assert np.abs(np.linalg.norm(nrm.astype(f64), axis=-1) - 1).max() < 8 * np.finfo(dt).eps


def _lambert(n, normal, dt=f32):
    """A Lambertian receiver: equal media leave no Fresnel term, the diffuse lobe is albedo cos / pi"""
    s = _plane_surface(n, dt)
    normal = np.asarray(normal, dtype=f64) / np.linalg.norm(normal)
    s["mapped_normal"] = s["flat_normal"] = normal
    view = -normal + np.array([0.3, 0.0, 0.1])
    s["view"] = view / np.linalg.norm(view)
    s["ior_in"] = s["ior_out"] = 1.0
    s["f0"] = 0.0
    return s


def _estimate(L, s, n, seed, dt):
    rs = _draws(n, seed)
    with A.area_mode():
        typ, idx, data, pdf = M.sample_canonical(L, rs, s["pos"], 1e-4, dt)
        value = M.light_contribution(L, typ, idx, data, s, dt)[0]
    assert (typ == 0).all() and (idx == 0).all()
    return value.astype(f64) / pdf.astype(f64)[:, None]


@pytest.mark.parametrize("dist, tilt", [(1.5, 0.0), (3.0, 35.0), (6.0, 60.0)])
def test_a_sphere_above_the_horizon_is_the_point_light(dist, tilt, capsys):
    """A uniformly emitting sphere wholly above a Lambertian receiver's horizon gives the point light's irradiance c cos(theta) / d^2: the
    mean of contribution / pdf over the model's draws is within 4 standard errors of the point mode's contribution."""
    from tauray_amd import scene as S
    n, r = 60_000, 0.7
    t = math.radians(tilt)
    normal = np.array([math.sin(t), math.cos(t), 0.0])
    centre = (0.0, dist, 0.0)
    assert dist * math.cos(t) > r, "the sphere is cut by the horizon"
    L = M.Lights(point=_sphere_light(S, (3.0, 2.0, 1.0), centre, r))
    s = _lambert(n, normal)
    point = M.light_contribution(L, np.zeros(1, dtype=int), np.zeros(1, dtype=int), np.zeros((1, 2)), s[:1], f64)[0][0]
    want = np.array([0.8, 0.5, 0.3]) / math.pi * np.array([3.0, 2.0, 1.0]) * math.cos(t) / dist ** 2
    assert np.abs(point / want - 1).max() < 1e-6
    for dt in (f32, f64):
        est = _estimate(L, s, n, 7, dt)
        mean, se = est.mean(0), est.std(0, ddof=1) / math.sqrt(n)
        assert (np.abs(mean - point) <= 4 * se).all(), (dt, mean, point, se)
        assert (se < 0.01 * point).all()
    with capsys.disabled():
        print(f"\nsphere lights, closed form at d = {dist}, tilt {tilt}: mean / point {mean / point}, standard error / point {se / point}")


def test_a_sphere_cut_by_the_horizon_gives_less_than_uncut_and_more_than_the_point_light(capsys):
    """A sphere that the receiver's horizon cuts: the draws below the horizon contribute nothing, so the mean of contribution / pdf is
    strictly less, by more than 4 standard errors of the paired difference, than what the same draws give when the hidden part lights
    the receiver too (radiance |cos| over the whole cap).  It is not less than the point light's c cos(theta) / d^2, and the test says so:
    that closed form is the integral of the signed cosine over the whole cap, the part below the horizon enters it negatively, and the
    cut sphere gives strictly more (the centre on the horizon: the point light gives 0, the visible half of the sphere does not)."""
    from tauray_amd import scene as S
    n, r, dist = 60_000, 0.7, 1.5
    t = math.radians(75.0)
    assert dist * math.cos(t) < r
    L = M.Lights(point=_sphere_light(S, (3.0, 2.0, 1.0), (0.0, dist, 0.0), r))
    normal = np.array([math.sin(t), math.cos(t), 0.0])
    s = _lambert(n, normal)
    point = M.light_contribution(L, np.zeros(1, dtype=int), np.zeros(1, dtype=int), np.zeros((1, 2)), s[:1], f64)[0][0]
    est = _estimate(L, s, n, 9, f64)
    nrm, pdf, direction, length = A.sphere_point(np.repeat(L.point, n), s["pos"], M.unit(_draws(n, 9), f64)[:, 1:3], 1e-4, f64)
    radiance = np.array([3.0, 2.0, 1.0]) / (r * r * math.pi)
    uncut = (np.array([0.8, 0.5, 0.3]) / math.pi * radiance) * (np.abs(direction @ normal) / pdf)[:, None]
    hidden = (direction @ normal) < 0
    # above the horizon the two are the same integrand, to the material model's own small terms
    assert 0.05 < hidden.mean() < 0.95 and (est[hidden] == 0).all() and np.abs(est[~hidden] / uncut[~hidden] - 1).max() < 1e-4
    diff = uncut - est
    mean, se = est.mean(0), est.std(0, ddof=1) / math.sqrt(n)
    with capsys.disabled():
        print(f"\nsphere lights, a sphere cut by the horizon: {hidden.mean():.1%} of the draws hidden, cut / uncut {mean / uncut.mean(0)}, cut / point light {mean / point}")
    assert (mean > 0).all() and (diff.mean(0) > 4 * diff.std(0, ddof=1) / math.sqrt(n)).all()
    assert (mean - 4 * se > point).all(), (mean, se, point)


def test_jacobian_of_a_sphere_sample():
    """The reconnection Jacobian of a point on a sphere between two receivers against the ratio of the solid angles a small patch of the
    sphere's tangent plane subtends from them (finite differences), as test_restir_di.py does for triangles; the model's contribution
    returns the point's normal, not 0."""
    from tauray_amd import scene as S
    r = 0.6
    L = M.Lights(point=_sphere_light(S, (1, 1, 1), (0.3, 2.0, -0.4), r))
    centre, r = L.point["pos"][0].astype(f64), float(L.point["radius"][0])
    n = np.array([0.36, -0.8, 0.48])
    data = A.oct_encode(n[None], f64)
    a, b = np.array([[0.1, 0.0, 0.2]]), np.array([[-0.7, 0.4, 0.9]])
    sa, sb = _plane_surface(1, pos=a), _plane_surface(1, pos=b)
    a, b = sa["pos"].astype(f64), sb["pos"].astype(f64)      # as the float32 records hold them
    typ = idx = np.zeros(1, dtype=int)
    va, da, d2a, na = A.light_contribution(L, typ, idx, data, sa, f64)
    vb, db, d2b, nb = A.light_contribution(L, typ, idx, data, sb, f64)
    x = centre + r * n
    assert np.abs(na[0] - n).max() < 1e-15 and np.abs(a[0] + da[0] * math.sqrt(d2a[0]) - x).max() < 1e-14 and np.abs(b[0] + db[0] * math.sqrt(d2b[0]) - x).max() < 1e-14
    assert (va > 0).all() and (vb > 0).all()
    e1 = np.cross(n, [1.0, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)

    def solid_angle(src, eps=1e-4):
        c = [x + eps * (sx * e1 + sy * e2) / 2 - src[0] for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        c = [v / np.linalg.norm(v) for v in c]

        def tri(p, q, w):
            return 2 * math.atan2(abs(np.dot(p, np.cross(q, w))), 1 + np.dot(p, q) + np.dot(q, w) + np.dot(p, w))
        return tri(c[0], c[1], c[2]) + tri(c[0], c[2], c[3])
    want = solid_angle(b) / solid_angle(a)
    got = M.jacobian(a, b, x[None], na, f64)[0]
    assert abs(got / want - 1) < 1e-6, (got, want)
    got32 = M.jacobian(a.astype(f32), b.astype(f32), x[None].astype(f32), na.astype(f32), f32)[0]
    assert abs(got32 / want - 1) < 1e-5
    # the point mode's sample of the same light has no normal: Jacobian 1
    assert (M.light_contribution(L, typ, idx, data, sa, f64)[3] == 0).all()


def test_corners_are_finite_and_give_nothing():
    """A receiver inside the sphere, one exactly on its surface (k = 0), r far larger than d, a spotlight with a radius, NaN in data: the
    pdf is finite and positive, the contribution 0 where the rule says so and never NaN, light_data, the candidate weight and the Jacobian
    finite.  The one NaN the rule leaves is the direction of a drawn point that is the receiver itself (normalize of 0, as for a triangle
    sample): its colour is 0 by the rule's test and no ray is cast."""
    from tauray_amd import scene as S
    n = 4096
    words = _draws(n, 13)
    for dt in (f32, f64):
        for name, centre, r, pos in (("inside", (0.0, 0.5, 0.0), 1.0, (0.0, 0.0, 0.0)), ("on the surface", (0.0, 1.0, 0.0), 1.0, (0.0, 0.0, 0.0)),
                                     ("r far larger than d", (0.0, 1e-3, 0.0), 1e4, (0.0, 0.0, 0.0))):
            L = M.Lights(point=_sphere_light(S, (3, 2, 1), centre, r))
            s = _plane_surface(n, pos=pos)
            with A.area_mode():
                typ, idx, data, pdf = M.sample_canonical(L, words, s["pos"], 1e-4, dt)
                value, direction, dist2, normal = M.light_contribution(L, typ, idx, data, s, dt)
            assert np.isfinite(pdf).all() and (pdf > 0).all(), name
            assert np.isfinite(value).all() and np.isfinite(data).all() and np.isfinite(dist2).all(), name
            # the direction is NaN only where the drawn point is the receiver itself (p = 0): nothing is lit and nothing is cast there
            assert (np.isfinite(direction).all(-1) | (dist2 == 0)).all(), name
            assert (value == 0).all(), name + ": a receiver in or on the sphere is lit"
            w = M.nan_to_zero(M.luminance(value, dt) / pdf)
            assert np.isfinite(w).all() and (w == 0).all()
        # a spotlight with a radius: the cone is judged at the centre's direction; finite, and lit inside the cone only
        spot = _sphere_light(S, (3, 2, 1), (0.0, 2.0, 0.0), 0.4, spot=((0.0, -1.0, 0.0), 30.0, 2.0))
        L = M.Lights(point=spot)
        s = _plane_surface(n)
        s["pos"][:, 0] = np.linspace(-3, 3, n)
        with A.area_mode():
            typ, idx, data, pdf = M.sample_canonical(L, words, s["pos"], 1e-4, dt)
            value = M.light_contribution(L, typ, idx, data, s, dt)[0]
        assert np.isfinite(value).all() and np.isfinite(pdf).all() and (pdf < 1e8).all()
        inside_cone = np.abs(s["pos"][:, 0]) < 2.0 * math.tan(math.radians(30.0)) - 0.01
        outside_cone = np.abs(s["pos"][:, 0]) > 2.0 * math.tan(math.radians(30.0)) + 0.01
        assert (value[inside_cone] > 0).any() and (value[outside_cone] == 0).all()
        # NaN in data: nothing, a finite weight, and the Jacobian's own guard gives 0
        bad = np.full((n, 2), np.nan)
        value, direction, dist2, normal = A.light_contribution(L, typ, idx, bad, s, dt)
        assert (value == 0).all()
        jac = M.jacobian(s["pos"].astype(dt), s["pos"].astype(dt) + dt(0.1), s["pos"].astype(dt) + direction * np.sqrt(dist2)[:, None], normal, dt)
        assert np.isfinite(jac).all() and (jac == 0).all()
        # a radius of 0 is the point mode, bit for bit
        L0 = M.Lights(point=_sphere_light(S, (3, 2, 1), (0.0, 2.0, 0.0), 0.0))
        with A.area_mode():
            got = M.sample_canonical(L0, words, s["pos"], 1e-4, dt) + M.light_contribution(L0, typ, idx, np.zeros((n, 2)), s, dt)
        want = M.sample_canonical(L0, words, s["pos"], 1e-4, dt) + M.light_contribution(L0, typ, idx, np.zeros((n, 2)), s, dt)
        for g, w_ in zip(got, want):
            assert np.asarray(g).tobytes() == np.asarray(w_).tobytes()


def test_model_float32_against_float64(capsys):
    """4096 seeded records, lights of mixed radii (0 among them, one a spot): no discrete decision differs between the precisions - class,
    index, which samples have a radius, which take the guard, which contributions are 0 - and pdfs, contributions and weights agree to
    the relative figure test_restir_di.py's model test holds the other classes to (2^-12 of the largest value of the kind, section 20's
    measure), by that test's own measure."""
    from tauray_amd import scene as S
    n, candidates = 4096, 8
    s, L0, eye = T._synthetic_records(n)
    point = np.concatenate([S.make_point_light((4, 3, 2), (0.5, 1.5, 0.2), 0.3), S.make_point_light((1, 2, 6), (-1.0, 0.7, 0.4), 0.0),
                            S.make_spotlight((9, 8, 7), (0.2, 2.0, -1.0), (0.1, -1.0, 0.3), 0.15, 40.0, 2.0), S.make_point_light((2, 2, 2), (1.5, 0.9, -1.0), 0.6)])
    L = M.Lights(point=point, tri=L0.tri, directional=L0.directional)
    out = {}
    for dt in (f32, f64):
        rs = M.init_sampler(np.arange(n) % 64, np.arange(n) // 64, 0, 4, 0)
        q = dict(pdf=[], contribution=[], weight=[])
        d = dict(type=[], index=[], guard=[], lit=[])
        with A.area_mode():
            for c in range(candidates):
                rs = M.pcg4d(rs)
                typ, idx, data, pdf = M.sample_canonical(L, rs, s["pos"], 1e-4, dt)
                contrib = M.light_contribution(L, typ, idx, data, s, dt)[0]
                w = M.nan_to_zero((dt(1) / dt(candidates)) * M.luminance(contrib, dt) / pdf)
                rs = M.pcg4d(rs)
                q["pdf"].append(pdf), q["contribution"].append(contrib), q["weight"].append(w)
                d["type"].append(typ), d["index"].append(idx), d["guard"].append(pdf > 1e6), d["lit"].append((contrib > 0).any(-1))
        out[dt] = {k: np.stack(v) for k, v in q.items()}, {k: np.stack(v) for k, v in d.items()}
    (q32, d32), (q64, d64) = out[f32], out[f64]
    sphere = (d64["type"] == 0) & np.isin(d64["index"], (0, 2, 3))
    assert sphere.sum() > n and ((d64["type"] == 0) & (d64["index"] == 1)).any() and set(np.unique(d64["type"])) == {0, 1, 2}
    report = {}
    for k in q32:
        finite = np.isfinite(q64[k]) & np.isfinite(q32[k].astype(f64))
        report[k] = np.abs(q32[k].astype(f64) - q64[k])[finite].max() / np.abs(q64[k][finite]).max()
        assert report[k] <= 2.0 ** -12, (k, report[k])
    differing = {k: int((d32[k] != d64[k]).sum()) for k in d32}
    with capsys.disabled():
        print(f"\nsphere lights model, float32 against float64 over {n} records x {candidates} candidates ({int(sphere.sum())} on a sphere): " +
              ", ".join(f"{k} {v:.2e}" for k, v in report.items()) + f"; differing discrete decisions {differing}")
    assert not any(differing.values()), differing


# =========================================================================================================================== GPU
RADII = (0.25, 0.3, 0.6)


def _room_with_radii(S, size, inside=True):
    """test_restir_di.py's room with its three point lights given a radius.  The two point lights stand outside both cameras' frusta, in
    front of the room's open side; the spotlight stands 0.4 from the right wall with a radius of 0.6, so the wall's pixels around it are
    inside the sphere - with inside = False its radius is 0.3 and no receiver is inside any sphere (the direct stage lights a receiver
    inside a sphere through a shadow ray of negative length, the rule here gives 0: the comparison with it uses that room)."""
    scene = _room(S, size)
    point = np.concatenate([S.make_point_light((14, 12, 10), (1.7, 1.6, 3.0), RADII[0]), S.make_point_light((5, 7, 11), (-1.8, 0.4, 3.2), RADII[1]),
                            S.make_spotlight((14, 13, 11), (1.6, 0.3, 0.5), (-0.5, -1.0, -0.2), RADII[2] if inside else 0.3, 50.0, 2.0)])
    scene.point_lights = point
    return scene


class _Rooms:
    """Scenes by (kind, size), uploaded on demand: one scene lives on the device at a time."""

    def __init__(self, R, ctx):
        self.R, self.ctx, self.scenes, self.key, self.ss = R, ctx, {}, None, None

    def __call__(self, kind, size, as_strategy=0):
        from tauray_amd import scene as S
        if (kind, size) not in self.scenes:
            self.scenes[(kind, size)] = {"room": lambda: _room(S, size), "radii": lambda: _room_with_radii(S, size),
                                         "radii outside": lambda: _room_with_radii(S, size, inside=False)}[kind]()
        if self.key != (kind, size, as_strategy):
            self.ss = self.R.SceneStage(self.ctx, self.scenes[(kind, size)], as_strategy=as_strategy)
            self.key = (kind, size, as_strategy)
        return self.scenes[(kind, size)], self.ss


@pytest.fixture(scope="module")
def rooms(R, ctx):
    return _Rooms(R, ctx)


NAMES = ("surface", "canonical", "history", "candidates", "temporal", "spatial", "final", "sampled")


def _record_run(R, ctx, ss, size, frames=3, viewports=(0, 1), tell=None, **options):
    """Frames of a recording stage: per frame the colour and every download.  tell: set_sphere_lights(tell) after create."""
    o = R.restir_di_options(record=True, **options)
    st = R.RestirDiStage(ctx, ss, size, len(viewports), o)
    if tell is not None:
        st.set_sphere_lights(tell)
    out = ctx.alloc(size[0] * size[1] * 16 * len(viewports)).zero()
    got = []
    for _ in range(frames):
        st.run(viewports, out)
        f = {n: st.download(n) for n in NAMES if n != "spatial" or o["spatial_samples"]}
        if st.options["bsdf_candidates"]:
            f["bsdf_candidates"] = st.download("bsdf_candidates")
        f["color"] = out.download((len(viewports), size[1], size[0], 4))
        got.append(f)
    st.close()
    out.free()
    return got, o


def _same_bits(name, a, b):
    """Byte for byte.  The one exception is the field `dir` of the BSDF candidates' record, where a NaN may differ from a NaN in its sign
    alone: IEEE 754 leaves the sign of a NaN open, two compilations of one expression differ in it (a source modifier negates a NaN's sign
    bit too), and that debug field keeps the direction of a triangle candidate whose light_data is NaN.  Every other field of that record,
    and every other buffer and record, holds no differing word."""
    if name != "bsdf_candidates":
        return a.tobytes() == b.tobytes()
    for field in a.dtype.names:
        x, y = (np.ascontiguousarray(r[field]).view(np.uint32) for r in (a, b))
        if field != "dir":
            if not (x == y).all():
                return False
            continue
        nan = lambda w: (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)      # noqa: E731
        if not ((x == y) | (nan(x) & nan(y) & ((x ^ y) == np.uint32(0x80000000)))).all():
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_point_told_never_told_and_area_without_radii_are_the_same_bits(R, ctx, rooms, size):
    """G1: on the existing room, whose lights have radius 0, a stage told `point`, a stage never told and a stage told `area` write the
    same bits to every buffer and record: three acceleration-structure strategies (both layouts), the three visibility modes, both light
    selections, with and without BSDF candidates."""
    base = dict(spatial_samples=2, temporal_reuse=True, search_radius=4.0, candidates=3, rng_seed=7)
    for strategy in (0, 1, 2):
        scene, ss = rooms("room", size, as_strategy=strategy)
        assert (scene.point_lights["radius"] == 0).all()
        for visibility, selection, bsdf in (("per-target", "uniform", 0), ("shared", "uniform", 0), ("sampled", "power", 0), ("per-target", "power", 2), ("shared", "uniform", 2)):
            o = dict(base, visibility=visibility, light_selection=selection, bsdf_candidates=bsdf)
            never, _ = _record_run(R, ctx, ss, size, **o)
            for tell in ("point", "area"):
                told, _ = _record_run(R, ctx, ss, size, tell=tell, **o)
                for fa, fb in zip(never, told):
                    assert fa.keys() == fb.keys()
                    for k in fa:
                        assert _same_bits(k, fa[k], fb[k]), (strategy, visibility, selection, bsdf, tell, k)


# ---- G2: the replay
class _ARun(T._Run):
    """T._Run in area mode; with the power selection, the table the stage drew through."""

    def __init__(self, R, ctx, ss, size, **options):
        self.table = None
        if options.get("light_selection") == "power":
            st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(light_selection="power"))
            self.table = st.download("light_table")
            st.close()
        super().__init__(R, ctx, ss, size, sphere_lights="area", **options)


@pytest.fixture(scope="module")
def area_runs(R, ctx, rooms):
    """The seven option sets of T.RUN_CASES in area mode on the room with radii, per light selection, rendered once and left unchanged"""
    cache = {}

    def get(selection, case):
        if (selection, case) not in cache:
            size, options = T.RUN_CASES[case]
            scene, ss = rooms("radii", size)
            cache[(selection, case)] = _ARun(R, ctx, ss, size, rng_seed=31 + case, light_selection=selection, **options)
        return cache[(selection, case)]
    return get


class _modelling:
    """The model in the run's mode: area, and the power selection's sampler beneath it when the run drew through a table"""

    def __init__(self, run):
        self.power = SM.power_selection(run.table) if getattr(run, "table", None) is not None else None
        self.area = A.area_mode()

    def __enter__(self):
        if self.power:
            self.power.__enter__()
        self.area.__enter__()

    def __exit__(self, *exc):
        self.area.__exit__(*exc)
        if self.power:
            self.power.__exit__(*exc)


@pytest.fixture(scope="module")
def area_models(area_runs, rooms):
    from tauray_amd import scene as S
    cache = {}

    def get(selection, case):
        if (selection, case) not in cache:
            run = area_runs(selection, case)
            scene, ss = rooms("radii", run.size)
            L = _lights_of(S, scene, ss)
            with _modelling(run):
                cache[(selection, case)] = {(fi, v): (T._model_frame(S, run, scene, L, fi, v, f32), T._model_frame(S, run, scene, L, fi, v, f64))
                                            for fi in range(len(run.frames)) for v in range(len(run.viewports))}
        return cache[(selection, case)]
    return get


def _sphere_candidates(run, scene, models):
    """Counts over a run's candidates: on a light with a radius, of those on the spot, of those whose pixel is inside the sphere"""
    seen = dict(sphere=0, spot=0, inside=0, lit=0)
    for (fi, v), (m32, m64) in models.items():
        f = run.frames[fi]
        ys, xs = m32["ys"], m32["xs"]
        cand = f["candidates"][v][ys, xs][:, :run.options["candidates"]]
        t, i = _light_split(cand["light"])
        on = (t == 0) & (i < len(scene.point_lights))
        seen["sphere"] += int(on.sum())
        seen["spot"] += int((on & (i == 2)).sum())
        pos = f["surface"][v][ys, xs]["pos"].astype(f64)
        inside = np.linalg.norm(pos - scene.point_lights["pos"][2].astype(f64), axis=-1) < RADII[2]
        seen["inside"] += int((on & (i == 2) & inside[:, None]).sum())
        assert (cand["contribution"][on & (i == 2) & inside[:, None]] == 0).all(), "a pixel inside the sphere is lit by it"
        seen["lit"] += int((on & (cand["contribution"] > 0).any(-1)).sum())
        # a sphere candidate's data is a point of the octahedral square, and its recorded pdf is the model's bit for bit unless guarded
        assert (np.abs(cand["light_data"][on]) <= 1).all()
        assert (_bits(cand["pdf"][on]) == _bits(m32["pdf"][:, :run.options["candidates"]][on])).all(), "a sphere candidate's pdf"
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("selection", ["uniform", "power"])
@pytest.mark.parametrize("case", range(len(T.RUN_CASES)))
def test_replay_in_area_mode(area_runs, area_models, rooms, selection, case, capsys):
    """G2, B = 0, per-target: test_restir_di.py's own three checks, called as they are on an area run of the room with radii with the
    area mode's model in restir_di_model's place - the float32 replay of the decision records gives both reservoir buffers and the
    colour bit for bit; the model's two pcg4d streams give every recorded draw, class, index and the light_data of type-0 candidates,
    the sphere candidates' octahedral data among them, bit for bit; pdfs, contributions, Jacobians, MIS terms and weights are held by
    4 |model32 - model64| + 1 ulp.  Some pixels are inside the spot's sphere and are not lit by it."""
    run, models = area_runs(selection, case), area_models(selection, case)
    scene, ss = rooms("radii", run.size)
    T.test_replay_of_the_decision_records_is_exact(lambda c: run, 0)
    T.test_draws_and_picks_are_exact(lambda c: run, lambda c: models, 0)
    T.test_continuous_quantities_are_bounded(lambda c: run, lambda c: models, 0, capsys)
    T.test_discrete_decisions_match_where_the_precisions_agree(lambda c: run, lambda c: models, 0, capsys)
    seen = _sphere_candidates(run, scene, models)
    with capsys.disabled():
        print(f"\nsphere lights replay, {selection}, case {case}: candidates {seen}")
    assert seen["sphere"] > 0 and seen["lit"] > 0
    if run.size == (37, 19):
        assert seen["spot"] > 0 and seen["inside"] > 0, "no pixel of the frame is inside the spot's sphere"
    # a Jacobian of a sphere sample is not the point mode's constant 1
    if run.options["spatial_samples"]:
        jn = np.concatenate([run.frames[fi]["spatial"][v]["jacobian_n"].ravel() for fi in range(len(run.frames)) for v in range(2)])
        assert ((jn != 0) & (jn != 1)).any()


VISIBILITY_CASES = (1, 6)


@pytest.fixture(scope="module")
def visibility_runs(R, ctx, rooms):
    cache = {}

    def get(mode, case):
        if (mode, case) not in cache:
            size, options = T.RUN_CASES[case]
            scene, ss = rooms("radii", size)
            cache[(mode, case)] = V._VRun(R, ctx, ss, size, rng_seed=51 + case, visibility=V.MODE_NAMES[mode], sphere_lights="area", **options)
        return cache[(mode, case)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("case", VISIBILITY_CASES)
@pytest.mark.parametrize("mode", [VM.SHARED, VM.SAMPLED])
def test_replay_in_area_mode_under_the_visibility_modes(visibility_runs, rooms, mode, case, capsys):
    """G2 in the modes shared and sampled on two of the option sets (per-target is test_replay_in_area_mode): test_restir_di_visibility.py's
    replay and its model check, called as they are."""
    from tauray_amd import scene as S
    run = visibility_runs(mode, case)
    scene, ss = rooms("radii", run.size)
    V._replay(run)
    L = _lights_of(S, scene, ss)
    with A.area_mode():
        models = {(fi, v): tuple(VM.model_frame(T._model_frame, run, scene, L, fi, v, dt, mode) for dt in (f32, f64))
                  for fi in range(len(run.frames)) for v in range(len(run.viewports))}
    V.test_the_model_gives_the_draws_the_picks_and_the_bounded_quantities(lambda m, c: run, lambda m, c: models, mode, case, capsys)
    t, i = _light_split(run.frames[0]["candidates"]["light"])
    assert ((t == 0) & (i < 3)).any()


def _light_candidates_are_the_models(frames, o, scene, L, table):
    """The light candidates of recorded frames against the model's canonical stream, whatever follows them: class, index, light_data of
    type-0 and directional candidates and the pdf of type-0 candidates bit for bit.  A BSDF candidate takes two draws like a light one."""
    total = o["candidates"] + o["bsdf_candidates"]
    seen = 0
    run = type("run", (), dict(table=table))
    with _modelling(run):
        for fi, f in enumerate(frames):
            for v in range(2):
                surf = f["surface"][v]
                ys, xs = np.nonzero(surf["instance_id"] >= 0)
                s = surf[ys, xs]
                rs = M.init_sampler(xs, ys, v, 2 * fi, o["rng_seed"])
                if o["temporal_reuse"]:
                    rs = M.pcg4d(rs)
                for c in range(total):
                    rs = M.pcg4d(rs)
                    if c < o["candidates"]:
                        typ, idx, data, pdf = M.sample_canonical(L, rs, s["pos"], o["min_ray_dist"], f32)
                        cr = f["candidates"][v][ys, xs][:, c]
                        t, i = _light_split(cr["light"])
                        assert (t == typ).all() and (i == idx).all()
                        exact = (t == 0) | (t == 2)
                        assert (_bits(cr["light_data"][exact]) == _bits(data[exact])).all(), (fi, v, c, "light_data")
                        assert (_bits(cr["pdf"][t == 0]) == _bits(pdf[t == 0])).all(), (fi, v, c, "pdf")
                        seen += int(((t == 0) & (i < len(scene.point_lights))).sum())
                    rs = M.pcg4d(rs)
                    assert (_bits(M.unit(rs, f32)[:, 0]) == _bits(f["candidates"][v][ys, xs][:, c]["draw"])).all(), (fi, v, c, "draw")
    return seen


BSDF_CASES = tuple(i for i, (size, o) in enumerate(T.RUN_CASES) if o["candidates"] + 2 <= 32)      # the two sets of 32 candidates cannot take B = 2


class _BRun:
    """An area run with B BSDF candidates in the shape of T._Run; with the power selection, the table the stage drew through.  `options`
    counts every candidate of a pixel as T's replay of the records wants it (candidates = L + B); n_light and n_bsdf say which is which."""

    def __init__(self, R, ctx, ss, size, n_bsdf, selection, **options):
        self.table = None
        if selection == "power":
            st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(light_selection="power"))
            self.table = st.download("light_table")
            st.close()
        self.frames, self.stage_options = _record_run(R, ctx, ss, size, bsdf_candidates=n_bsdf, sphere_lights="area", light_selection=selection, **options)
        self.size, self.viewports = size, (0, 1)
        self.n_light, self.n_bsdf = self.stage_options["candidates"], n_bsdf
        self.options = dict(self.stage_options, candidates=self.n_light + n_bsdf)


def _bsdf_frames_are_the_models(run, scene, ss, L, capsys, what):
    """test_restir_di_bsdf_candidates.py's comparison of every candidate of a frame with B > 0, with and without temporal reuse and under
    either selection: a light candidate's pdf is the model's own (the sampler of the run's mode, the sphere helper behind it), a found
    sample's p_l the identity pdf through the run's table; the found sample's type, index and light_data from the recorded hit bit for
    bit; direction, p_b, p_l, denom, contribution and weight within 4 |model32 - model64| + 1 ulp.  A candidate whose discrete outcome
    differs between the model's two precisions is left out, at most 1 % of them."""
    import restir_di_bsdf_model as B
    o, n_light, n_bsdf = run.stage_options, run.n_light, run.n_bsdf
    base = TB._light_base_ids(scene, ss)
    failures, worst, left_out, seen = [], {}, 0, 0
    with _modelling(run):
        for fi, f in enumerate(run.frames):
            for v in range(2):
                surf, cand, rec, temp = f["surface"][v], f["candidates"][v], f["bsdf_candidates"][v], f["temporal"][v]
                hit = surf["instance_id"] >= 0
                ys, xs = np.nonzero(hit)
                s = surf[hit]
                rs = M.init_sampler(xs, ys, v, 2 * fi, o["rng_seed"])
                if o["temporal_reuse"]:
                    rs = M.pcg4d(rs)
                reuse = (temp["reuse"] != 0)[hit]
                prev_conf = np.where(reuse, temp["prev_confidence"][hit], f32(0)).astype(f32)
                assert (fi > 0 and o["temporal_reuse"]) or not reuse.any()
                for c in range(n_light + n_bsdf):
                    cr, br = cand[..., c][hit], rec[..., c][hit]
                    rs = M.pcg4d(rs)
                    first = rs
                    rs = M.pcg4d(rs)
                    typ_s, idx_s = _light_split(cr["light"])
                    keep = np.ones(len(s), dtype=bool)
                    m = {}
                    for dt in (f32, f64):
                        if c < n_light:
                            assert (br["technique"] == 0).all() and (br["traced"] == 0).all()
                            p_l = M.sample_canonical(L, first, s["pos"], o["min_ray_dist"], dt)[3]
                            contrib, cdir, _, _ = M.light_contribution(L, typ_s, idx_s, cr["light_data"], s, dt)
                            pb = B.light_candidate_p_b(typ_s, s, br["dir"].astype(dt), dt)
                            m[dt] = dict(dir=cdir, p_b=pb, p_l=p_l, contribution=contrib)
                        else:
                            assert (br["technique"] == 1).all()
                            d, pb0, cast, disc = B.candidate_direction(M.unit(first, dt), s, dt)
                            direction = br["dir"].astype(dt)
                            pb = np.where(cast, B.p_b(s, direction, dt), pb0)
                            typ, idx, data = B.sample_of_hit(L, cast, br["instance_id"].astype(np.int64), br["primitive_id"].astype(np.int64), br["u"], br["v"], direction, base, dt)
                            contrib, cdir, _, _ = M.light_contribution(L, typ, idx, data, s, dt)
                            p_l = B.identity_light_pdf(L, typ, idx, data, s["pos"], cdir, o["min_ray_dist"], dt, light_table=run.table)
                            m[dt] = dict(dir=d, p_b=pb, p_l=p_l, contribution=contrib, cast=cast, disc=disc + (np.where(typ == 3, B.env_pixel(L, data, dt), -1),),
                                         sample=(typ, idx, data))
                        t = M.luminance(m[dt]["contribution"] * cr["visibility"].astype(dt)[:, None], dt)
                        m[dt]["denom"], m[dt]["weight"] = B.balance_weight(n_light, n_bsdf, m[dt]["p_l"], m[dt]["p_b"], t, prev_conf.astype(dt), dt)
                    if c >= n_light:
                        for x, y in zip(m[f32]["disc"] + (m[f32]["cast"],), m[f64]["disc"] + (m[f64]["cast"],)):
                            keep &= x == y
                        left_out += int((~keep).sum())
                        assert ((br["traced"] != 0) == m[f32]["cast"])[keep].all(), (fi, v, c, "traced")
                        typ, idx, data = m[f32]["sample"]
                        assert (typ == typ_s)[keep].all() and (idx == idx_s)[keep].all(), (fi, v, c, "found sample")
                        assert (_bits(data.astype(f32)) == _bits(cr["light_data"]))[keep].all(), (fi, v, c, "light_data")
                        assert not ((typ_s == 0) & (idx_s != M.NULL_INDEX)).any(), "a BSDF candidate found a sphere light"
                        assert (cr["visibility"] == (cr["contribution"] > 0).any(-1))[keep].all()
                    seen += len(s)
                    got = dict(dir=br["dir"], p_b=br["p_b"], p_l=cr["pdf"], denom=br["denom"], contribution=cr["contribution"], weight=cr["weight"])
                    for k in got:
                        name = ("bsdf " if c >= n_light else "light ") + k
                        worst[name] = max(worst.get(name, 0.0), T._bounded(f"frame {fi} view {v} candidate {c} {name}", got[k], m[f32][k], m[f64][k], keep, failures))
    with capsys.disabled():
        print(f"\nsphere lights replay with B = {n_bsdf}, {what}: {left_out} of {seen} candidates left out; largest error / bound: " + ", ".join(f"{k} {x:.2f}" for k, x in worst.items()))
    assert left_out <= 0.01 * seen
    assert not failures, "\n".join(failures[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("selection", ["uniform", "power"])
@pytest.mark.parametrize("case", BSDF_CASES)
def test_replay_in_area_mode_with_bsdf_candidates(R, ctx, rooms, selection, case, capsys):
    """G2 with B = 2 on the five option sets of T.RUN_CASES that can take it, under both selections, on the room with radii.
    test_restir_di.py's replay of the decision records, called as it is over all L + B candidates of a pixel, gives both reservoir buffers
    and the colour bit for bit; the model's stream gives every candidate's selection draw and the light candidates' class, index, sphere
    data and type-0 pdf bit for bit; every candidate of either technique is held to the model as
    test_restir_di_bsdf_candidates.py holds them, the power selection's identity pdf through the stage's table."""
    from tauray_amd import scene as S
    size, options = T.RUN_CASES[case]
    scene, ss = rooms("radii", size)
    run = _BRun(R, ctx, ss, size, 2, selection, rng_seed=71 + case, **options)
    assert run.n_light == options["candidates"] and run.frames[0]["candidates"].shape[-1] == run.n_light + 2
    T.test_replay_of_the_decision_records_is_exact(lambda c: run, 0)
    L = _lights_of(S, scene, ss)
    assert _light_candidates_are_the_models(run.frames, run.stage_options, scene, L, run.table) > 0
    _bsdf_frames_are_the_models(run, scene, ss, L, capsys, f"{selection}, case {case}")


# ---- the small scenes of G3 and G5
def _down_camera(S, size, eye):
    """A perspective camera at `eye` looking straight down, image columns along +x"""
    cam = S.Camera(fov=60, aspect=size[0] / size[1])
    m = np.eye(4)
    f, up = np.array([0.0, -1.0, 0.0]), np.array([0.0, 0.0, -1.0])
    r = np.cross(f, up)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, np.cross(r, f), -f, eye
    cam.transform = m
    return cam


def _floor_scene(S, size, light, occluder=False, lambertian=False):
    """A floor y = 0 seen from (0, 1.2, 0) looking down, one sphere light above and behind the camera (outside its frustum), and with
    `occluder` a horizontal quad at y = 1.5 over x >= -1.5, above the camera, whose edge along z puts the floor's x > 0 in the shadow of
    the light's centre at (-3, 3, 0): by similar triangles the penumbra is as wide on the floor as the sphere looks from the edge."""
    from test_estimator_consistency import _quad, _scene
    mat = S.make_material(albedo=(0.7, 0.6, 0.5, 1), metallic=0.0, roughness=1.0, ior=1.0 if lambertian else 1.45)
    quads = [(*_quad(S, (-8, 0, -8), (0, 0, 16), (16, 0, 0)), mat)]
    if occluder:
        quads.append((*_quad(S, (-1.5, 1.5, -8), (0, 0, 16), (6, 0, 0)), mat))
    return _scene(S, quads, [_down_camera(S, size, (0.0, 1.2, 0.0))], point_lights=light)


def _area_frames(R, ctx, ss, size, K, mode, **options):
    """K frames of one stage without temporal reuse: the sampler is seeded by the frame, the frames are independent"""
    st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(temporal_reuse=False, sphere_lights=mode, **options))
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    imgs = np.zeros((K, size[1], size[0], 3))
    for k in range(K):
        st.run([0], buf)
        imgs[k] = buf.download((size[1], size[0], 4))[..., :3]
    st.close()
    buf.free()
    return imgs


@pytest.mark.gpu
def test_point_modes_image_is_area_modes_expectation(R, capsys):
    """G3: a Lambertian floor, one sphere light wholly above every pixel's horizon, no occluder, one candidate, no reuse.  Point mode's
    frame is deterministic and is the closed form c cos / d^2; area mode averaged over K independent frames is within 4 standard errors,
    from the per-frame sample variance, of it, per pixel row and per channel."""
    from tauray_amd import scene as S
    size, K = (37, 19), 256
    own = R.Context(0)
    scene = _floor_scene(S, size, S.make_point_light((30, 24, 18), (-1.5, 2.5, 0.4), 0.6), lambertian=True)
    ss = R.SceneStage(own, scene)
    o = dict(candidates=1, spatial_samples=0, rng_seed=5, min_ray_dist=scene_min_ray_dist(R, scene))
    point = _area_frames(R, own, ss, size, 2, "point", **o)
    assert (_bits(point[0].astype(f32)) == _bits(point[1].astype(f32))).all() and (point[0] > 0).all()
    area = _area_frames(R, own, ss, size, K, "area", **o)
    own.close()
    assert np.isfinite(area).all() and not (area[0] == area[1]).all()
    rows = area.mean(2)                                   # (K, rows, 3)
    mean, se = rows.mean(0), rows.std(0, ddof=1) / math.sqrt(K)
    z = np.abs(mean - point[0].mean(1)) / se
    with capsys.disabled():
        print(f"\nsphere lights, point mode's frame against {K} area frames per pixel row: largest deviation {z.max():.2f} standard errors, standard error / mean {np.max(se / mean):.3%}")
    assert (z <= 4).all(), z.max()
    assert (se < 0.02 * mean).all()


EXPECTATION_CASES = {
    "no reuse": (dict(candidates=4, spatial_samples=0, temporal_reuse=False), 1, 24),
    "temporal reuse, 3 spatial samples, frame 8": (dict(candidates=4, spatial_samples=3, temporal_reuse=True, search_radius=8.0), 9, 24),
    "shared visibility": (dict(candidates=4, spatial_samples=2, temporal_reuse=False, search_radius=8.0, visibility="shared"), 1, 24),
    "power selection": (dict(candidates=4, spatial_samples=0, temporal_reuse=False, light_selection="power"), 1, 24),
    "B = 2": (dict(candidates=2, bsdf_candidates=2, spatial_samples=0, temporal_reuse=False), 1, 24),
}


@pytest.fixture(scope="module")
def direct64(R, ctx, rooms):
    """The direct stage's 16 batches at 64 spp on the room with radii, computed once"""
    from test_estimator_consistency import _dup
    size, K = (64, 64), 16
    scene, ss = rooms("radii outside", size)
    direct = R.DirectStage(ctx, ss, R.options_for_scene(scene, samples_per_pixel=64, samples_per_pass=1), _dup(size))
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    base = np.zeros((K, size[1], size[0], 3))
    for k in range(K):
        direct.reset_accumulated_samples()
        direct.run(buf)
        base[k] = buf.download((size[1], size[0], 4))[..., :3]
    direct.close()
    buf.free()
    return base


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXPECTATION_CASES))
def test_same_expectation_as_the_direct_stage(R, ctx, rooms, direct64, name, capsys):
    """G4: test_restir_di.py's comparison, unchanged - 64 x 64, 16 batches, _assert_same_mean with its z values, outlier share and bias
    floor as they are - of the direct stage at 64 spp against area mode on the room with radii in which no receiver is inside a sphere
    (_room_with_radii says why)."""
    from test_estimator_consistency import _assert_same_mean
    size, K = (64, 64), 16
    scene, ss = rooms("radii outside", size)
    options, frames, seeds = EXPECTATION_CASES[name]
    buf = ctx.alloc(size[0] * size[1] * 16).zero()
    got = np.zeros((K, size[1], size[0], 3))
    seed = 1
    for k in range(K):
        for _ in range(seeds):
            st = R.RestirDiStage(ctx, ss, size, 1, R.restir_di_options(rng_seed=seed, sphere_lights="area", **options))
            seed += 1
            for _f in range(frames):
                st.run([0], buf)
            got[k] += buf.download((size[1], size[0], 4))[..., :3] / seeds
            st.close()
    buf.free()
    assert np.isfinite(got).all()
    se = got.mean((1, 2)).std(0, ddof=1) / math.sqrt(K) / got.mean((0, 1, 2))
    rel, z = _assert_same_mean(direct64, got, name)
    with capsys.disabled():
        print(f"\nsphere lights against the direct stage, {name}: image means differ by {rel:.3%} ({z:.2f} standard errors), standard error of a batch mean {se.max():.2%}")
    assert (se * math.sqrt(K) < 0.05).all(), "a batch is too noisy to say anything"


@pytest.mark.gpu
def test_penumbra(R, capsys):
    """G5, what the feature is for.  A floor, a sphere light of radius 0.5 at (-3, 3, 0), an occluder edge at height 1.5 halfway down:
    the penumbra on the floor is about as wide as the sphere looks, a unit, and the camera 1.2 above the floor sees 2.5 units across 64
    columns.  Visibility is the direct stage's image divided by its image without the occluder, both from 8 batches of 512 spp; the band
    is the columns whose visibility lies in [0.2, 0.8]; its size and both deviations are printed (profiles/r29/restir_sphere_lights.txt keeps
    a run's line).  Area mode: over the band the mean of K frames is within 4 standard errors (of
    the difference: the frames' and the reference batches') of the reference per pixel column.  Point mode: the same assertion fails,
    and every band pixel is fully lit or fully dark."""
    from tauray_amd import scene as S
    from test_estimator_consistency import _dup
    size, K, B = (64, 36), 256, 8
    light = S.make_point_light((60, 50, 40), (-3.0, 3.0, 0.0), 0.5)
    own = R.Context(0)
    ref = {}
    for occluder in (True, False):
        scene = _floor_scene(S, size, light, occluder=occluder)
        ss = R.SceneStage(own, scene)
        buf = own.alloc(size[0] * size[1] * 16).zero()
        batches = np.zeros((B, size[1], size[0], 3))
        for b in range(B):
            st = R.DirectStage(own, ss, R.options_for_scene(scene, samples_per_pixel=512, samples_per_pass=1, rng_seed=100 + b), _dup(size))
            st.run(buf)
            batches[b] = buf.download((size[1], size[0], 4))[..., :3]
            st.close()
        buf.free()
        ref[occluder] = batches
        if occluder:
            o = dict(candidates=1, spatial_samples=0, rng_seed=3, min_ray_dist=scene_min_ray_dist(R, scene))
            area = _area_frames(R, own, ss, size, K, "area", **o)
            point = _area_frames(R, own, ss, size, 2, "point", **o)
    own.close()
    lum = lambda a: a @ np.array([0.2126, 0.7152, 0.0722])      # noqa: E731
    visibility = lum(ref[True].mean(0)).mean(0) / lum(ref[False].mean(0)).mean(0)      # per column
    band = np.nonzero((visibility >= 0.2) & (visibility <= 0.8))[0]
    assert len(band) >= 6 and (np.diff(band) == 1).all(), f"the band is {len(band)} columns"
    assert visibility[:band[0]].min() > 0.8 and visibility[band[-1] + 1:].max() < 0.2

    def deviation(frames):      # per band column, in standard errors of the difference
        cols, rcols = lum(frames).mean(1)[:, band], lum(ref[True]).mean(1)[:, band]
        se = np.sqrt(cols.var(0, ddof=1) / len(cols) + rcols.var(0, ddof=1) / B) if len(cols) > 1 else np.sqrt(rcols.var(0, ddof=1) / B)
        return np.abs(cols.mean(0) - rcols.mean(0)) / se
    z_area = deviation(area)
    # point mode is deterministic: its frame against the reference, in the reference's own standard errors and in the area frames'
    assert (_bits(point[0].astype(f32)) == _bits(point[1].astype(f32))).all()
    cols_p, rcols = lum(point[:1]).mean(1)[:, band], lum(ref[True]).mean(1)[:, band]
    se_p = np.sqrt(lum(area).mean(1)[:, band].var(0, ddof=1) / K + rcols.var(0, ddof=1) / B)
    z_point = (np.abs(cols_p[0] - rcols.mean(0)) / se_p)
    unoccluded = lum(ref[False].mean(0))[:, band]
    p = lum(point[0])[:, band]
    binary = (p == 0) | (np.abs(p / unoccluded - 1) < 0.1)
    text = (f"penumbra at {size[0]} x {size[1]}: band of {len(band)} columns ({band[0]}..{band[-1]}), visibility {visibility[band[0]]:.2f}..{visibility[band[-1]]:.2f}; "
            f"area mode, {K} frames: largest deviation {z_area.max():.2f} standard errors; point mode: largest {z_point.max():.1f}, smallest {z_point.min():.1f} standard errors, "
            f"band pixels fully lit or fully dark {binary.mean():.0%}")
    with capsys.disabled():
        print("\nsphere lights, " + text)
    assert (z_area <= 4).all(), z_area
    assert not (z_point <= 4).all(), "point mode draws the penumbra"
    assert binary.all() and (p == 0).any() and (p > 0).any()


@pytest.mark.gpu
def test_stage_behaviour(R, ctx, rooms):
    """G6: the setter's refusals by their text and its acceptance after reset; reset equals a new stage; two fresh runs give the same
    bits; area mode differs from point mode on the room with radii; the ReSTIR GI renderer hands the option to its DI half."""
    from tauray_amd import _lib
    size = (37, 19)
    scene, ss = rooms("radii", size)
    o = dict(candidates=4, spatial_samples=2, temporal_reuse=True, search_radius=6.0, rng_seed=5)
    a, ha = T._frames(R, ctx, ss, size, [0, 1], 3, sphere_lights="area", **o)
    b, hb = T._frames(R, ctx, ss, size, [0, 1], 3, sphere_lights="area", **o)
    assert (_bits(a) == _bits(b)).all() and ha.tobytes() == hb.tobytes(), "two fresh runs differ"
    p, hp = T._frames(R, ctx, ss, size, [0, 1], 3, **o)
    assert not (_bits(a) == _bits(p)).all(), "area mode changes nothing on the room with radii"
    assert np.isfinite(a).all()
    st = R.RestirDiStage(ctx, ss, size, 2, R.restir_di_options(**o))
    assert st.options["sphere_lights"] == "point"
    for mode in (-1, 2):
        assert st._fn("set_sphere_lights")(st.h, mode) != 0
        assert f"trhip_restir_di_set_sphere_lights: mode {mode} is outside 0..1" in _lib.lib().trhip_last_error().decode()
    st.set_sphere_lights("area")
    c = T._frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    st.set_sphere_lights("area")      # no change: accepted
    with pytest.raises(R.TrhipError) as e:
        st.set_sphere_lights("point")
    assert "trhip_restir_di_set_sphere_lights: the stage holds history of the area mode: call trhip_restir_di_reset first" in str(e.value)
    assert st.options["sphere_lights"] == "area"
    st.reset()
    d = T._frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    assert (_bits(c) == _bits(a[:2])).all() and (_bits(d) == _bits(a[:2])).all(), "reset does not equal a new stage"
    st.reset()
    st.set_sphere_lights("point")
    e2 = T._frames(R, ctx, ss, size, [0, 1], 2, stage=st)
    assert (_bits(e2) == _bits(p[:2])).all()
    with pytest.raises(R.TrhipError) as e:
        st.set_sphere_lights("area")
    assert "the stage holds history of the point mode" in str(e.value)
    st.close()
    gi = R.RestirGiRenderer(ctx, ss, scene, size, R.restir_gi_options(spatial_samples=1, search_radius=8.0), R.restir_di_options(sphere_lights="area", **o))
    assert gi.direct.options["sphere_lights"] == "area"
    gi.render()
    assert np.isfinite(gi.download("display")).all()
    gi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("renderer, which", [("restir-di", "animation"), ("restir-di", "still"), ("restir-gi", "still")])
def test_both_hosts_write_the_same_bits(R, ctx, tmp_path, renderer, which):
    """G6: tauray_hip --restir-sphere-lights=area against the Python renderer, two frames at 64 x 36 as .raw, bit for bit:
    animated_lamp.glb - animated.glb with a radius of 0.15 on its lamp (TR_data) - under --animation, the temporal re-evaluation of
    world-fixed sphere points over moving geometry, and test.glb, whose light has a radius of 0.1, for both renderers that take the
    option - there the first frame differs from point mode's."""
    from tauray_amd.gltf import load_glb
    from tauray_amd.animation import SceneAnimator
    size, frames = (64, 36), 2
    glb = os.path.join(GOLDEN, "animated_lamp.glb" if which == "animation" else "test.glb")
    prefix = str(tmp_path / "cpp")
    args = [CLI, glb, "--renderer=" + renderer, "--restir=2,1,16,16,on", "--restir-sphere-lights=area", f"--width={size[0]}", f"--height={size[1]}", f"--frames={frames}",
            "--filetype=raw", "--format=rgba32", "--rng-seed=3", "--headless=" + prefix]
    if which == "animation":
        args.append("--animation")
    if renderer == "restir-gi":
        args.append("--restir-gi=2,16,8,on")
    p = subprocess.run(args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    scene = load_glb(glb, *size)
    assert (scene.point_lights["radius"] != 0).any()
    ss = R.SceneStage(ctx, scene)
    animator = None
    if which == "animation":
        animator = SceneAnimator(scene)
        animator.play("")
    mrd = scene_min_ray_dist(R, scene)
    di = dict(candidates=2, spatial_samples=1, search_radius=16.0, max_confidence=16.0, temporal_reuse=True, rng_seed=3, min_ray_dist=mrd)
    gi = R.restir_gi_options(spatial_samples=2, search_radius=16.0, max_confidence=8.0, temporal_reuse=True, rng_seed=3, min_ray_dist=mrd)

    def make(mode):
        o = R.restir_di_options(sphere_lights=mode, **di)
        return R.RestirDiRenderer(ctx, ss, scene, size, o) if renderer == "restir-di" else R.RestirGiRenderer(ctx, ss, scene, size, gi, o)
    rr = make("area")
    first = None
    for f in range(frames):
        if animator:
            ss.animate(animator, 0 if f == 0 else round(1000000.0 / 60.0), refit=(f % 3 != 2))
        rr.render()
        img = rr.download("display")
        first = img if first is None else first
        assert np.isfinite(img).all() and img[..., :3].max() > 0
        got = _raw(f"{prefix}{f}.raw", (size[1], size[0], 4))
        differing = int((_bits(got) != _bits(img[0])).any(-1).sum())
        assert differing == 0, f"{renderer}, {which}, frame {f}: {differing} of {size[0] * size[1]} pixels differ"
    rr.close()
    if which == "still":
        assert (scene.point_lights["radius"] != 0).any()
        rp = make("point")
        rp.render()
        assert not (_bits(rp.download("display")) == _bits(first)).all(), "the option changes nothing on a scene whose light has a radius"
        rp.close()
