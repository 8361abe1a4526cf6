"""CPU-side checks of the drop-in boundary: libtrhip.so loads and exports every symbol declared in
include/trhip.h, struct layouts match the header, the product fails loudly without a GPU, and the host
mirror (loader, camera packing, alias table) behaves like the reference's host code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "trhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trhip_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from tauray_amd import _lib
    L = _lib.lib()
    names = _declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), f"libtrhip.so does not export {n}"
    assert sorted(_lib.SYMBOLS) == names, "python binding and header disagree on the entry points"


def test_build_id_is_the_one_the_makefile_generated():
    """trhip_build_id: 64 bits of SHA-256 over the library's sources and compile flags (csrc/Makefile -> build_id.inc), mixed into a
    stage's program identity so that the ranks of a job notice two different builds of libtrhip.so (include/trhip.h)."""
    from tauray_amd import _lib
    inc = os.path.join(ROOT, "tauray_amd", "csrc", "build_id.inc")
    got = _lib.lib().trhip_build_id()
    assert got != 0
    if os.path.exists(inc) and os.path.getmtime(inc) <= os.path.getmtime(_lib.LIB_PATH):
        want = int(re.search(r"0x([0-9a-f]+)ull", open(inc).read()).group(1), 16)
        assert got == want, "libtrhip.so is not the build build_id.inc describes"


def test_struct_layouts_match_header():
    from tauray_amd import _lib
    assert C.sizeof(_lib.PtOptionsC) == 24 * 4
    assert C.sizeof(_lib.DistributionC) == 24          # distribution_data_buffer is 24 bytes too (rt_camera_stage.cc:17-24)
    assert C.sizeof(_lib.CountersC) == 7 * 8
    assert C.sizeof(_lib.TimingsC) == 10 * 4
    assert C.sizeof(_lib.TonemapInfoC) == 16
    assert C.sizeof(_lib.AccelInfoC) == 48
    assert C.sizeof(_lib.PtTargetsC) == 9 * 8
    from oracle import binding as B
    assert C.sizeof(B.PtOptionsC) == C.sizeof(_lib.PtOptionsC)
    assert C.sizeof(B.PtTargetsC) == C.sizeof(_lib.PtTargetsC)
    assert [f[0] for f in B.PtOptionsC._fields_] == [f[0] for f in _lib.PtOptionsC._fields_]


def test_no_silent_cpu_fallback():
    """Without a GPU the product must fail loudly (the oracle is never a fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tauray_amd import renderer as R
    with pytest.raises(R.TrhipError) as e:
        R.Context(0)
    assert "HIP" in str(e.value) or "device" in str(e.value)
    import tauray_amd
    src = ""
    for root, _, files in os.walk(os.path.dirname(tauray_amd.__file__)):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src += open(os.path.join(root, f), errors="replace").read()
    assert "from oracle" not in src and "import oracle" not in src and "liboracle" not in src, "product code references the oracle"


def test_glb_loader_flattening(test_glb_512):
    d = test_glb_512
    assert d.triangle_count == 81364 and len(d.instances) == 8
    assert list(d.spans["triangle_count"]) == [4, 2, 2, 2, 14280, 62976, 4096, 2]      # Cube x4, Teapot, Suzanne, Torus, Plane
    assert list(d.instances["light_base_id"]) == [-1, -1, -1, -1, -1, -1, 0, -1]
    assert d.tri_light_count == 4096
    assert list(d.potentially_transparent()) == [False] * 5 + [True, False, True]      # transmissive Suzanne, alpha-blended plane
    assert len(d.point_lights) == 1 and len(d.directional_lights) == 1
    sl = d.point_lights[0]
    assert sl["radius"] == pytest.approx(0.1) and sl["dir_cutoff"] == pytest.approx(np.cos(0.1745329201221466))
    assert np.allclose(sl["color"], np.array([0.5349318981170654, 1, 0.4066522419452667]) * 1000 / (4 * np.pi), rtol=1e-6)
    assert d.directional_lights[0]["dir_cutoff"] == pytest.approx(np.cos(0.09966865181922913), rel=1e-6)
    cam = d.cameras[0]
    assert cam.fov == pytest.approx(45.0, abs=1e-4) and cam.aspect == 1.0
    assert np.allclose(cam.transform[:3, 3], [0, 0, 6.828], atol=1e-5)
    # teapot: no uv / tangent in the file -> tangents generated (NaN-free not guaranteed by the reference either)
    m = d.instances["mat"]
    assert m["transmittance"][5] == 1.0 and m["albedo_tex_id"][7] == 0 and m["metallic_roughness_factor"][4, 0] == 1.0


def test_camera_packing_and_grid(test_glb_512):
    from tauray_amd import scene as S
    cam = test_glb_512.cameras[0]
    data = cam.pack()[0]
    view = S.from_glm(data["view"]); inv = S.from_glm(data["view_inverse"])
    assert np.allclose(view @ inv, np.eye(4), atol=1e-6)
    proj_inv = S.from_glm(data["proj_inverse"])
    assert np.allclose(proj_inv @ cam.projection_matrix(), np.eye(4), atol=1e-5)
    assert np.allclose(data["origin"], [0, 0, 6.828, 1], atol=1e-5)
    # light-field grid of src/tauray.cc:680-727: 9x5 views, spacing 0.02, recentering distance 5
    grid = S.generate_camera_grid(cam, 9, 5, 0.02, 0.02, 5.0)
    assert len(grid) == 45
    xs = sorted({round(float((np.linalg.inv(cam.transform) @ g.transform)[0, 3]), 6) for g in grid})
    assert len(xs) == 9 and xs[0] == pytest.approx(-0.08) and xs[-1] == pytest.approx(0.08)
    centre = grid[22]
    assert centre.fov_offset == pytest.approx((0.0, 0.0), abs=1e-9)
    corner = grid[0]   # x = -0.08, y = +0.04 -> pan = -pos / (tan(fov/2) * 5)
    t = np.tan(np.radians(cam.fov) / 2)
    assert corner.fov_offset[0] == pytest.approx(0.08 / (t * cam.aspect * 5), rel=1e-6)
    assert corner.fov_offset[1] == pytest.approx(-0.04 / (t * 5), rel=1e-6)


def test_alias_table_is_a_valid_distribution():
    from tauray_amd.scene import build_alias_table
    rng = np.random.default_rng(2)
    env = rng.uniform(0.0, 1.0, size=(8, 16, 4)).astype(np.float32) ** 4
    env[2, 3, :3] = 50.0
    at = build_alias_table(env)
    n = 8 * 16
    # reconstruct each texel's selection probability from the alias table
    p = np.zeros(n)
    for i in range(n):
        q = (int(at["probability"][i]) + 1) / 2.0 ** 32 if at["probability"][i] != 0xFFFFFFFF else 1.0
        p[i] += q / n
        p[int(at["alias_id"][i])] += (1 - q) / n
    assert p.sum() == pytest.approx(1.0, abs=1e-6)
    lum = env[..., 0] * 0.2126 + env[..., 1] * 0.7152 + env[..., 2] * 0.0722
    ys = np.arange(8)
    solid = 2 * np.pi * (np.cos(np.pi * ys / 8) - np.cos(np.pi * (ys + 1) / 8)) / 16
    imp = (lum * solid[:, None]).reshape(-1)
    assert np.allclose(p, imp / imp.sum(), atol=2e-4)
    # pdf integrates to ~1 over the sphere
    sin_t = np.sin((ys + 0.5) / 8 * np.pi)
    texel_sa = (2 * np.pi / 16) * (np.pi / 8) * sin_t
    assert (at["pdf"].reshape(8, 16) * texel_sa[:, None]).sum() == pytest.approx(1.0, rel=0.05)


def test_procedural_scenes_are_deterministic():
    from tauray_amd import scenes
    a = scenes.sponza_class(seed=1, target_tris=30000, width=64, height=36)
    b = scenes.sponza_class(seed=1, target_tris=30000, width=64, height=36)
    c = scenes.sponza_class(seed=2, target_tris=30000, width=64, height=36)
    assert scenes.scene_hash(a) == scenes.scene_hash(b) != scenes.scene_hash(c)
    assert 15000 < a.triangle_count < 60000
    assert a.envmap is not None and len(a.directional_lights) == 1 and a.tri_light_count == 4
    frac_alpha = a.spans["triangle_count"][a.potentially_transparent()].sum() / a.triangle_count
    assert 0.01 < frac_alpha < 0.15


def test_load_balancer_follows_the_reference():
    """load_balancer (src/load_balancer.cc:12-52): EMA towards the measured speeds; a zero "path tracing" time makes the speed
    sum non-finite and the update is skipped instead of raising."""
    from tauray_amd.distribution import LoadBalancer
    lb = LoadBalancer(3)
    assert lb.workloads == pytest.approx([1 / 3] * 3)
    w = lb.update([1.0, 2.0, 4.0])
    speeds = np.array([1 / 3, 1 / 6, 1 / 12])
    assert w == pytest.approx(list(np.array([1 / 3] * 3) * 0.9 + speeds / speeds.sum() * 0.1))
    assert sum(w) == pytest.approx(1.0)
    before = list(w)
    assert lb.update([1.0, 0.0, 2.0]) == before          # inf speed: skipped
    lb2 = LoadBalancer(2, [1.0, 0.0])
    assert lb2.workloads == [1.0, 0.0]
    assert lb2.update([1.0, 0.0]) == [1.0, 0.0]           # 0 / 0 = NaN: skipped
    assert LoadBalancer(3, [2.0, 2.0]).workloads == pytest.approx([0.5, 0.5, 0.0])


def test_headers_are_plain_c(tmp_path):
    """The boundary is a C ABI: include/trhip.h and include/trhip_comm.h compile as C99 with -pedantic, without a warning, and a C program
    links against the two libraries (what a cgo / JNI / Rust-FFI binding of the reference would sit on)."""
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text('#include "trhip.h"\n#include "trhip_comm.h"\n#include <stdio.h>\n'
                   "int main(void) {\n    trhip_pt_options o; trhip_distribution d; trhip_scene_desc s; trhip_counters c;\n"
                   "    (void)o; (void)d; (void)s; (void)c;\n"
                   '    printf("%u %u %u [%s]\\n", (unsigned)sizeof(o), (unsigned)sizeof(d), (unsigned)sizeof(trhip_accel_info), trhip_last_error());\n'
                   "    return trhip_comm_size(0);\n}\n")
    exe = str(tmp_path / "abi")
    lib = os.path.join(ROOT, "tauray_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src),
                        "-L" + lib, "-ltrhip", "-ltrhip_comm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[:3] == ["96", "24", "48"], out.stdout + out.stderr


def test_frame_schedule_without_a_device(tmp_path):
    """tests/pt_schedule_check.cc: the path tracer's frame schedule (csrc/pt_schedule.h: plan_frame, the enqueue order, the switches and the rule
    for the caller's stream class) against values worked out by hand, a stand-alone program built with the address and undefined-behaviour
    sanitizers.  The header needs no HIP: plain g++, no library, no device."""
    import subprocess
    exe = str(tmp_path / "pt_schedule_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "pt_schedule_check.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) == (0, "ok"), r.stdout + r.stderr
