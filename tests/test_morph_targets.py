"""glTF morph targets (trhip_scene_set_morph_targets / trhip_scene_morph, tauray_amd/csrc/morph.h).

CPU: both loaders on tests/golden/morph.glb (the C++ one through tests/morph_check.cc, built with the host sanitizers), the weights tracks
of both players, the numpy model of morph.h (tests/morph_model.py), the ABI and the refusals the arguments alone decide.  GPU: k_morph
against the float32 model bit for bit, morph ahead of skinning, frames of a morphed scene against the same scene uploaded with the model's
vertices, instancing, and both hosts playing morph.glb."""
import copy
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import morph_model as M
from conftest import GOLDEN, ROOT

GLB = os.path.join(GOLDEN, "morph.glb")
CLI = os.path.join(ROOT, "tauray_amd", "tauray_hip")
BT = 256                     # lanes per block of k_morph (bvh_build.hip)
ALL, PER_MESH = 0, 1
f32 = np.float32


@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


@pytest.fixture(scope="module")
def ctx2(R):
    """A second handle: a device handle holds one scene, and some tests need a morphed scene and a fresh upload side by side."""
    return R.Context(0)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/morph_check.cc with the address and undefined-behaviour sanitizers: a stand-alone program, no device."""
    exe = str(tmp_path_factory.mktemp("morph_check") / "morph_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTAURAY_HIP_WITH_ZLIB",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "morph_check.cc"), "-o", exe,
                    "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"],
                   check=True)
    return exe


def _run(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr      # a sanitizer report goes to stderr
    return p.stdout.strip().split("\n")


def _bits(line, name):
    words = line.split()
    assert words[0] == name and int(words[1]) == len(words) - 2, line[:80]
    return np.array([int(w, 16) for w in words[2:]], dtype=np.uint32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _glb_json(path):
    d = open(path, "rb").read()
    n = struct.unpack_from("<I", d, 12)[0]
    return json.loads(d[20:20 + n]), d[:12], d[20 + n:]


# =========================================================================================================================== CPU
def test_both_loaders_read_the_same_targets(check_exe):
    from tauray_amd.gltf import load_glb, _Glb
    sc = load_glb(GLB, 48, 32)
    out = _run(check_exe, "load", GLB)
    n = len(sc.instances)
    assert n == 3 and [tuple(int(x) for x in l.split()[1:]) for l in out[:n]] == [tuple(int(x) for x in s) for s in sc.spans]
    assert out[n] == f"morphed {len(sc.morphed)}" and len(sc.morphed) == 3
    for k, mm in enumerate(sc.morphed):
        head, w, p, nr, tg = out[n + 1 + 5 * k:n + 6 + 5 * k]
        assert head == f"mesh {mm.instance} {mm.node} {len(mm.position_deltas)}"
        assert np.array_equal(_bits(w, "weights"), _u32(mm.weights))
        assert np.array_equal(_bits(p, "position"), _u32(mm.position_deltas))
        assert np.array_equal(_bits(nr, "normal"), _u32(mm.normal_deltas) if mm.normal_deltas is not None else np.zeros(0, np.uint32))
        assert np.array_equal(_bits(tg, "tangent"), _u32(mm.tangent_deltas) if mm.tangent_deltas is not None else np.zeros(0, np.uint32))
    left, right, strip = sc.morphed
    # two nodes of one mesh: spans and default weights of their own (mesh.weights / node.weights), the same planes
    assert (left.instance, right.instance) == (0, 1) and sc.spans[0]["vertex_offset"] != sc.spans[1]["vertex_offset"]
    assert left.weights.tolist() == [0.5, 0.25, 0.0] and right.weights.tolist() == [0.0, 1.0, 0.75] and strip.weights.tolist() == [0.5]
    assert np.array_equal(left.position_deltas, right.position_deltas) and left.position_deltas.shape == (3, 81, 3)
    # a target that lacks an attribute others carry has a zero plane for it; the strip has no normal or tangent target at all
    assert not left.normal_deltas[:2].any() and left.normal_deltas[2].any() and not left.tangent_deltas[:2].any() and left.tangent_deltas[2].any()
    assert strip.normal_deltas is None and strip.tangent_deltas is None and [s.instance for s in sc.skinned] == [2]
    # the sparse accessors (over zeros, over a bufferView) equal their dense twins, and it is they that the targets name
    g = _Glb(GLB)
    mesh = g.json["meshes"][0]
    twins = {int(k): v for k, v in mesh["extras"]["dense_twins"].items()}
    targets = mesh["primitives"][0]["targets"]
    assert set(twins) == {targets[1]["POSITION"], targets[2]["NORMAL"]} and all("sparse" in g.json["accessors"][a] for a in twins)
    assert "bufferView" not in g.json["accessors"][targets[1]["POSITION"]] and "bufferView" in g.json["accessors"][targets[2]["NORMAL"]]
    for sparse, dense in twins.items():
        assert np.array_equal(g.accessor(sparse).view(np.uint32), g.accessor(dense).view(np.uint32)) and g.accessor(dense).any()
    assert np.array_equal(left.position_deltas[1], g.accessor(twins[targets[1]["POSITION"]])) and np.array_equal(left.normal_deltas[2], g.accessor(twins[targets[2]["NORMAL"]]))
    # the uploaded vertices are the file's base attributes
    assert np.array_equal(sc.vertices["pos"][:81], g.accessor(mesh["primitives"][0]["attributes"]["POSITION"]))
    # files without targets
    for name in ("test.glb", "skinned.glb", "animated.glb"):
        assert load_glb(os.path.join(GOLDEN, name), 48, 32).morphed == []
        assert _run(check_exe, "load", os.path.join(GOLDEN, name))[-1] == "morphed 0"


def test_unreadable_sparse_accessors_are_errors(check_exe, tmp_path):
    from tauray_amd.gltf import load_glb
    doc, head, rest = _glb_json(GLB)
    sparse = doc["meshes"][0]["primitives"][0]["targets"][1]["POSITION"]
    for what, change, text in (("index", lambda a: a["sparse"].update(count=a["sparse"]["count"], indices=dict(a["sparse"]["indices"], componentType=5126)), "sparse indices must be unsigned integers"),
                               ("count", lambda a: a["sparse"].update(count=a["count"] + 1), "sparse count exceeds the accessor"),
                               ("values", lambda a: a["sparse"].pop("values"), "sparse accessor needs indices and values"),
                               ("range", lambda a: a.update(count=5), "sparse")):
        d = copy.deepcopy(doc)
        change(d["accessors"][sparse])
        js = json.dumps(d, separators=(",", ":")).encode()
        js += b" " * ((-len(js)) % 4)
        path = str(tmp_path / f"{what}.glb")
        open(path, "wb").write(head[:8] + struct.pack("<I", 12 + 8 + len(js) + len(rest)) + struct.pack("<II", len(js), 0x4E4F534A) + js + rest)
        with pytest.raises(ValueError) as e:
            load_glb(path, 48, 32)
        assert text in str(e.value)
        p = subprocess.run([check_exe, "load", path], capture_output=True, text=True)
        assert p.returncode == 1 and text in p.stderr, p.stderr


def test_weights_tracks_of_both_players(check_exe):
    from tauray_amd.animation import SceneAnimator, LINEAR, STEP, CUBICSPLINE
    from tauray_amd.gltf import load_glb
    sc = load_glb(GLB, 48, 32)
    clips = {n: sc.animations[n]["morph"] for n in (0, 1, 2)}
    assert [clips[n].weights.interpolation for n in (0, 1, 2)] == [LINEAR, STEP, CUBICSPLINE]
    assert [clips[n].weights.data.shape for n in (0, 1, 2)] == [(3, 3), (3, 3), (3, 1)] and clips[2].weights.in_tangent.shape == (3, 1)
    assert [clips[n].loop_time for n in (0, 1, 2)] == [1000000, 750000, 1000000]      # the weights track counts: these clips have no other
    # by hand: before the clip, at keys, between keys, after the clip (ticks are microseconds)
    #   LINEAR  keys (0,0,0) (1,.5,0) (.25,0,1) at 0, .5, 1 s
    #   STEP    keys (0,1,.75) (1,0,0) (0,0,1.5) at 0, .25, .75 s
    #   CUBIC   p(t) = (2t^3-3t^2+1) p0 + (t^3-2t^2+t) dt m0 + (-2t^3+3t^2) p1 + (t^3-t^2) dt m1, dt = 0.5 s:
    #           0 -> .5 s: p0 = 0, m0 = 2, p1 = 1, m1 = -1; at t = .5: .125 + .5 + .0625 = .6875
    #           .5 -> 1 s: p0 = 1, m0 = 1, p1 = -.5, m1 = .5; at t = .5: .5 + .0625 - .25 - .03125 = .28125
    times = [-1, 0, 125000, 250000, 500000, 625000, 750000, 1000000, 2000000]
    want = {0: [[0, 0, 0], [0, 0, 0], [.25, .125, 0], [.5, .25, 0], [1, .5, 0], [.8125, .375, .25], [.625, .25, .5], [.25, 0, 1], [.25, 0, 1]],
            1: [[0, 1, .75], [0, 1, .75], [0, 1, .75], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1.5], [0, 0, 1.5], [0, 0, 1.5]],
            2: [[0], [0], None, [.6875], [1], None, [.28125], [-.5], [-.5]]}
    for n in (0, 1, 2):
        out = _run(check_exe, "sample", GLB, n, "morph", *times)
        assert out[0] == f"loop_time {clips[n].loop_time}"
        for t, line, w in zip(times, out[1:], want[n]):
            py = clips[n].weights.sample(t)
            cpp = np.array([float(x) for x in line.split()])
            assert np.array_equal(py, cpp), (n, t, py, cpp)      # the two players, bit for bit (doubles)
            if w is not None:
                assert np.abs(py - np.array(w)).max() <= 1e-7, (n, t, py, w)      # float32 ratio and spline coefficients
    # the players: four updates at 4 frames per second; the first applies time 0, the STEP clip ends before the fourth
    an = SceneAnimator(sc)
    an.play("")
    played = _run(check_exe, "play", GLB, 4, 4)
    by_hand = [[[0, 0, 0], [0, 1, .75], [0]], [[.5, .25, 0], [1, 0, 0], [.6875]], [[1, .5, 0], [1, 0, 0], [1]], [[.625, .25, .5], [1, 0, 0], [.28125]]]
    for f in range(4):
        an.update(0 if f == 0 else 250000)
        for k, mm in enumerate(sc.morphed):
            w = sc.morph_weights(mm)
            assert w.dtype == np.float32 and np.array_equal(_bits(played[3 * f + k], "weights"), _u32(w)), (f, k)
            assert np.abs(w - np.array(by_hand[f][k], f32)).max() <= 1e-7, (f, k, w)


@pytest.mark.parametrize("seed, vertices, targets, normals, tangents", [(1, 1, 1, True, True), (2, 255, 3, True, False), (3, 257, 9, False, True), (4, 775, 9, True, True),
                                                                         (5, 64, 3, False, False)])
def test_model_float32_against_float64(seed, vertices, targets, normals, tangents):
    v, dpos, dnrm, dtan = M.random_mesh(seed, vertices, targets, normals, tangents)
    rng = np.random.default_rng(seed + 100)
    w = rng.uniform(-1.5, 2.0, targets).astype(f32)
    w[rng.integers(0, targets)] = 0 if targets > 1 else w[0]
    a, b = M.morph(v, w, dpos, dnrm, dtan), M.morph(v, w, dpos, dnrm, dtan, dtype=np.float64)
    active = len(M.active_list(w))
    eps = float(np.finfo(f32).eps)
    # each of the 2 k operations of the accumulation loses half an ulp of a value no larger than the sum of the magnitudes
    mag = np.abs(v["pos"]).max() + sum(abs(float(x)) for x in w) * 0.3
    assert np.abs(a["pos"].astype(np.float64) - b["pos"]).max() <= active * eps * mag
    # normalisation: the accumulated error relative to the length (at least 1 - 0.3 sum|w| is not guaranteed: measure it), + sqrt, division
    for name, plane, sl in (("normal", dnrm, slice(None)), ("tangent", dtan, slice(0, 3))):
        x, y = a[name][:, sl].astype(np.float64), b[name][:, sl]
        if plane is None:
            assert np.array_equal(a[name], v[name])
            continue
        acc = v[name][:, sl].astype(np.float64) + sum(float(wk) * plane[k].astype(np.float64) for k, wk in M.active_list(w))
        length = np.linalg.norm(acc, axis=1)
        bound = (2 * active * eps * (1 + sum(abs(float(x)) for x in w) * 0.3) / length + 4 * eps)[:, None]      # sqrt(3) < 2 components' worth
        assert (np.abs(x - y) <= bound).all(), name
        # a normalised direction has unit length to 2 ulp
        unit = np.sqrt((x * x).sum(axis=1))
        assert np.abs(unit - 1.0).max() <= 2 * eps, name
    assert np.array_equal(a["uv"], v["uv"]) and np.array_equal(a["tangent"][:, 3], v["tangent"][:, 3])


def test_model_zero_weights_and_zero_length():
    v, dpos, dnrm, dtan = M.random_mesh(7, 300, 4)
    v["pos"][0] = (-0.0, 0.0, -0.0)
    out = M.morph(v, np.zeros(4, f32), dpos, dnrm, dtan)
    assert out.tobytes() == v.tobytes()                       # the base, bit for bit: -0 stays -0
    assert M.active_list([0.0, -0.0, 2.0, 0.0]) == [(2, f32(2.0))]      # -0 is a zero weight
    # a normal that the targets cancel keeps the base normal; the position still moves
    dnrm[1] = -v["normal"]
    out = M.morph(v, np.array([0, 1, 0, 0], f32), dpos, dnrm, dtan)
    assert np.array_equal(out["normal"], v["normal"]) and not np.array_equal(out["pos"], v["pos"])
    # an order that matters is pinned: the list is walked in ascending target order
    w = np.array([1e8, 1.0, -1e8, 0], f32)
    d = np.ones((4, 300, 3), f32)
    assert np.array_equal(M.morph(v, w, d)["pos"], ((v["pos"] + f32(1e8)) + f32(1.0)) + f32(-1e8))


def test_entry_points_declared_exported_and_bound(tmp_path):
    from tauray_amd import _lib
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    src = tmp_path / "sig.c"
    src.write_text('#include "trhip.h"\n'
                   "int (*set_targets)(trhip_device*, uint32_t, uint32_t, const float*, const float*, const float*, uint32_t) = trhip_scene_set_morph_targets;\n"
                   "int (*morph)(trhip_device*, uint32_t, const float*, uint32_t) = trhip_scene_morph;\nint main(void) { return 0; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sig.o")])
    L = _lib.lib()
    for name, args in (("trhip_scene_set_morph_targets", 7), ("trhip_scene_morph", 4)):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(L, name)
        assert _lib.SYMBOLS[name][0] is C.c_int and len(_lib.SYMBOLS[name][1]) == args
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tauray_amd", "libtrhip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        assert re.search(r"\bT trhip_scene_set_morph_targets$", nm.stdout, re.M) and re.search(r"\bT trhip_scene_morph$", nm.stdout, re.M)
    assert os.path.exists(os.path.join(ROOT, "tauray_amd", "csrc", "morph.h"))


def _refusal(call, *args):
    from tauray_amd import _lib
    assert call(*args) != 0
    return _lib.lib().trhip_last_error().decode()


def test_refusals_the_arguments_decide():
    """What needs no device to be refused is refused before the device is looked at: these run with a null handle."""
    from tauray_amd import _lib
    L = _lib.lib()
    d = np.zeros((2, 4, 3), f32)
    bad = d.copy()
    bad[1, 2, 1] = np.inf
    nan = d.copy()
    nan[0, 0, 0] = np.nan
    p = lambda a: a.ctypes.data
    assert "target_count is 0" in _refusal(L.trhip_scene_set_morph_targets, None, 0, 0, p(d), None, None, 4)
    assert "null position deltas" in _refusal(L.trhip_scene_set_morph_targets, None, 0, 2, None, None, None, 4)
    assert "non-finite delta" in _refusal(L.trhip_scene_set_morph_targets, None, 0, 2, p(bad), None, None, 4)
    assert "non-finite delta" in _refusal(L.trhip_scene_set_morph_targets, None, 0, 2, p(d), p(nan), None, 4)
    assert "non-finite delta" in _refusal(L.trhip_scene_set_morph_targets, None, 0, 2, p(d), None, p(bad), 4)
    assert "null trhip_device" in _refusal(L.trhip_scene_set_morph_targets, None, 0, 2, p(d), None, None, 4)
    w = np.array([0.5, np.nan], f32)
    assert "non-finite weight" in _refusal(L.trhip_scene_morph, None, 0, p(w), 2)
    assert "non-finite weight" in _refusal(L.trhip_scene_morph, None, 0, p(np.array([np.inf], f32)), 1)
    assert "null trhip_device" in _refusal(L.trhip_scene_morph, None, 0, p(np.array([0.5], f32)), 1)


# =========================================================================================================================== GPU
VERTEX_COUNTS = (1, BT - 1, BT, BT + 1, 3 * BT + 7)
TARGET_COUNTS = (1, 3, 9)
WEIGHTS = {1: [-0.75], 3: [1.5, 0.0, -0.25], 9: [0.0, 2.0, -1.25, 0.0, 0.5, 1.0, -0.0, 0.125, 3.0]}


def _strip_indices(n):
    """Triangles over n vertices: a strip, or one degenerate triangle for fewer than three."""
    if n < 3:
        return np.zeros(3, np.uint32)
    i = np.arange(n - 2, dtype=np.uint32)
    return np.stack([i, i + 1, i + 2], axis=1).reshape(-1)


def _scene(meshes, models=None):
    """A SceneDesc of one instance per (vertices, indices) mesh, a point light and a camera on +z looking at the origin."""
    from tauray_amd import scene as S
    inst, spans, voff, ioff = [], [], 0, 0
    for k, (v, idx) in enumerate(meshes):
        mat = S.make_material(albedo=(0.3 + 0.1 * (k % 5), 0.6, 0.8 - 0.1 * (k % 4), 1), metallic=0.0, roughness=0.6, double_sided=True)
        inst.append(S.make_instance(np.eye(4) if models is None else models[k], mat))
        spans.append((voff, len(v), ioff, len(idx) // 3))
        voff, ioff = voff + len(v), ioff + len(idx)
    cam = S.Camera(transform=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0], [0, 0, 0, 1.0]]), fov=40.0, near=0.1, far=100.0)
    cam.set_aspect(1.5)
    sc = S.SceneDesc(instances=np.concatenate(inst), spans=np.array(spans, dtype=S.MESH_SPAN), vertices=np.concatenate([m[0] for m in meshes]),
                     indices=np.concatenate([m[1] for m in meshes]).astype(np.uint32),
                     point_lights=S.make_point_light(np.array([20.0, 19.0, 18.0]), (0.5, 2.0, 3.0), 0.0), cameras=[cam])
    return sc.finalize(True)


@pytest.fixture(scope="module")
def kernel_cases(R):
    """One scene with a mesh per (vertex count, target count, planes) case, uploaded once to a handle of its own."""
    ctx = R.Context(0)
    cases, meshes = [], []
    for vc in VERTEX_COUNTS:
        for tc in TARGET_COUNTS:
            for planes in (True, False):
                v, dpos, dnrm, dtan = M.random_mesh(1000 * vc + 10 * tc + planes, vc, tc, planes, planes)
                cases.append((vc, tc, planes, v, dpos, dnrm, dtan))
                meshes.append((v, _strip_indices(vc)))
    return R.SceneStage(ctx, _scene(meshes)), cases


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(VERTEX_COUNTS) * len(TARGET_COUNTS) * 2))
def test_k_morph_is_the_float32_model_bit_for_bit(kernel_cases, case):
    ss, cases = kernel_cases
    vc, tc, planes, v, dpos, dnrm, dtan = cases[case]
    assert ss.vertices(case).tobytes() == v.tobytes()
    ss.set_morph_targets(case, dpos, dnrm, dtan)
    w = np.array(WEIGHTS[tc], f32)
    ss.morph(case, w, refit=None)
    got, want = ss.vertices(case), M.morph(v, w, dpos, dnrm, dtan)
    assert len(got) == vc and not np.array_equal(want["pos"], v["pos"])
    assert got.tobytes() == want.tobytes(), (vc, tc, planes)          # every byte of every vertex: pos, normal, uv, tangent
    assert planes == (not np.array_equal(want["normal"], v["normal"])) == (not np.array_equal(want["tangent"], v["tangent"]))
    ss.morph(case, w, refit=None)                                     # again: the same bits (the base is not the destination)
    assert ss.vertices(case).tobytes() == want.tobytes()
    ss.morph(case, np.zeros(tc, f32), refit=None)                     # all-zero weights: the base, verbatim
    assert ss.vertices(case).tobytes() == v.tobytes()
    if case + 1 < len(cases):                                         # the neighbours in the vertex array are untouched
        assert ss.vertices(case + 1).tobytes() == cases[case + 1][3].tobytes()


@pytest.mark.gpu
def test_refusals_on_the_device(R, ctx):
    from tauray_amd.scene import SKIN
    v, dpos, dnrm, dtan = M.random_mesh(11, 40, 2)
    ss = R.SceneStage(ctx, _scene([(v, _strip_indices(40)), (v.copy(), _strip_indices(40))]))

    def refused(text, fn, *a, **kw):
        with pytest.raises(R.TrhipError) as e:
            fn(*a, **kw)
        assert text in str(e.value), str(e.value)
    refused("trhip_scene_set_morph_targets: instance out of range", ss.set_morph_targets, 2, dpos)
    refused("trhip_scene_set_morph_targets: vertex_count differs from the instance's mesh", ss.set_morph_targets, 0, dpos[:, :39])
    refused("trhip_scene_set_morph_targets: target_count is 0", ss.set_morph_targets, 0, dpos[:0])
    bad = dpos.copy()
    bad[1, 39, 2] = np.nan
    refused("trhip_scene_set_morph_targets: non-finite delta", ss.set_morph_targets, 0, bad)
    refused("trhip_scene_morph: instance has no morph targets", ss.morph, 0, np.ones(2, f32))
    refused("trhip_scene_morph: instance has no morph targets", ss.morph, 7, np.ones(2, f32))
    ss.set_morph_targets(0, dpos, dnrm, dtan)
    refused("trhip_scene_morph: 3 weights for 2 targets", ss.morph, 0, np.ones(3, f32))
    refused("trhip_scene_morph: non-finite weight", ss.morph, 0, np.array([1, np.inf], f32))
    refused("trhip_scene_morph: instance has no morph targets", ss.morph, 1, np.ones(2, f32))
    skins = np.zeros(40, dtype=SKIN)
    skins["weights"][:, 0] = 1
    refused("trhip_scene_set_skin: the instance has morph targets", ss.set_skin, 0, skins)
    ss.set_skin(1, skins)                                             # the other instance: skin first, then targets
    ss.set_morph_targets(1, dpos)
    assert ss.vertices(0).tobytes() == v.tobytes()                    # nothing refused changed anything
    ss.set_scene(ss.scene)                                             # an upload clears the slots
    refused("trhip_scene_morph: instance has no morph targets", ss.morph, 0, np.ones(2, f32))
    ss.set_skin(0, skins)


@pytest.mark.gpu
def test_morph_then_skin(R, ctx, ctx2):
    """trhip_scene_morph writes a skinned instance's bind pose, and the scene changes at the next trhip_scene_skin: the result is the bits
    of a skin whose source is the model's morphed vertices."""
    from tauray_amd.scene import SKIN
    vc = BT + 37
    v, dpos, dnrm, dtan = M.random_mesh(21, vc, 3)
    rng = np.random.default_rng(22)
    skins = np.zeros(vc, dtype=SKIN)
    skins["joints"][:, 1] = 1
    skins["weights"][:, 0] = rng.uniform(0, 1, vc)
    skins["weights"][:, 1] = f32(1) - skins["weights"][:, 0]
    joints = np.stack([np.eye(4), np.eye(4)]).astype(f32)
    joints[0, :3, 3] = (0.25, -0.125, 0.5)
    joints[1, :3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.25]]
    w = np.array([0.75, 0.0, -1.5], f32)
    a = R.SceneStage(ctx, _scene([(v, _strip_indices(vc))]))
    a.set_skin(0, skins)
    a.set_morph_targets(0, dpos, dnrm, dtan)
    a.morph(0, w, refit=None)
    assert a.vertices(0).tobytes() == v.tobytes()                     # not yet: glTF skins what it morphed
    a.skin(0, joints, refit=None)
    got = a.vertices(0)
    b = R.SceneStage(ctx2, _scene([(v, _strip_indices(vc))]))
    b.set_skin(0, skins, source=M.morph(v, w, dpos, dnrm, dtan))
    b.skin(0, joints, refit=None)
    assert got.tobytes() == b.vertices(0).tobytes()
    b.set_skin(0, skins)
    b.skin(0, joints, refit=None)
    assert got.tobytes() != b.vertices(0).tobytes()                   # and the morph mattered


def _grid(n, seed):
    """An n x n sheet in the xy plane facing +z with seeded targets that keep it a height field."""
    from tauray_amd.scene import VERTEX
    rng = np.random.default_rng(seed)
    u, vv = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    v = np.zeros(n * n, dtype=VERTEX)
    v["pos"] = np.stack([u.reshape(-1), vv.reshape(-1), np.zeros(n * n)], axis=1)
    v["normal"] = (0, 0, 1)
    v["tangent"] = (1, 0, 0, 1)
    v["uv"] = v["pos"][:, :2] * 0.5 + 0.5
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    idx = np.stack([a, a + 1, a + n, a + 1, a + n + 1, a + n], axis=1).reshape(-1).astype(np.uint32)
    dpos = np.zeros((3, n * n, 3), f32)
    dpos[:, :, 2] = rng.uniform(-0.4, 0.4, (3, n * n))
    dnrm = rng.uniform(-0.5, 0.5, (3, n * n, 3)).astype(f32)
    dnrm[:, :, 2] = 0
    dtan = rng.uniform(-0.5, 0.5, (3, n * n, 3)).astype(f32)
    return v, idx, dpos, dnrm, dtan


def _views(R, ctx, ss, scene, size):
    """World position, world normal and a path-traced 1-spp frame."""
    from test_gpu_parity import _render_hip
    from test_accel_strategies import _dup
    out = []
    for fid in (R.FEATURE_WORLD_POS, R.FEATURE_WORLD_NORMAL):
        buf = ctx.alloc(size[0] * size[1] * 16).zero()
        R.FeatureStage(ctx, ss, fid, _dup(size)).run(buf)
        out.append(buf.download((size[1], size[0], 4)))
    out.append(_render_hip(R, ctx, ss, scene, size, max_bounces=3))
    return out


def _same_views(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [ALL, PER_MESH])
def test_frames_of_a_morphed_scene(R, ctx, ctx2, strategy):
    """A morphed scene renders the bits of the same scene uploaded with the model's vertices: after a refit, after a rebuild, and after a
    second morph with other weights.  The sheet has a rigid neighbour and sits under a transform, so that the two-level structure has work."""
    size = (48, 32)
    v, idx, dpos, dnrm, dtan = _grid(13, 31)
    wall, wall_idx, _, _, _ = _grid(3, 32)
    place = np.array([[1.0, 0, 0, -0.25], [0, 1.0, 0, 0.125], [0, 0, 1.0, 0.0], [0, 0, 0, 1.0]])
    back = np.array([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, -1.5], [0, 0, 0, 1.0]])

    def uploaded(vertices, where):
        sc = _scene([(vertices, idx), (wall, wall_idx)], [place, back])
        return R.SceneStage(where, sc, as_strategy=strategy), sc
    ss, sc = uploaded(v, ctx)
    base = _views(R, ctx, ss, sc, size)
    assert np.isfinite(base[0][..., 0]).mean() > 0.5
    ss.set_morph_targets(0, dpos, dnrm, dtan)
    for w, refit in (([1.0, -0.5, 0.0], True), ([1.0, -0.5, 0.0], False), ([0.0, 0.75, 1.25], True)):
        w = np.array(w, f32)
        ss.morph(0, w, refit=refit)
        want_v = M.morph(v, w, dpos, dnrm, dtan)
        assert ss.vertices(0).tobytes() == want_v.tobytes()
        got = _views(R, ctx, ss, sc, size)
        fresh, fresh_sc = uploaded(want_v, ctx2)
        want = _views(R, ctx2, fresh, fresh_sc, size)
        assert _same_views(got, want), (strategy, w, refit)
        assert not any(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, base)), "the morph has to show in every view"
    if strategy == PER_MESH:      # dynamic without a mark: the sheet has a BLAS of its own, and a morph refits that one alone
        ss.morph(0, np.array([0.5, 0.5, 0.5], f32), refit=True)
        assert ss.layout()["blas_updated"] == 1


@pytest.mark.gpu
def test_instances_of_a_morphed_mesh(R, ctx):
    from tauray_amd.gltf import load_glb
    sc = load_glb(GLB, 48, 32)
    ss = R.SceneStage(ctx, sc)
    left, right, strip = sc.morphed
    base = sc.vertices[:81]
    assert np.array_equal(sc.vertices[81:162], base)
    want = [M.morph(base, mm.weights, mm.position_deltas, mm.normal_deltas, mm.tangent_deltas) for mm in (left, right)]
    got = [ss.vertices(0), ss.vertices(1)]
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()      # the default weights, applied at set-up
    assert got[0].tobytes() != got[1].tobytes() and got[0].tobytes() != base.tobytes()           # two shapes, neither the base
    # ... and they render as two shapes: the depth of the left sheet's pixels is not that of the right sheet's (unmorphed, both are z = 0)
    from test_accel_strategies import _dup
    buf = ctx.alloc(48 * 32 * 16).zero()
    R.FeatureStage(ctx, ss, R.FEATURE_WORLD_POS, _dup((48, 32))).run(buf)
    z = buf.download((32, 48, 4))[..., 2]
    lz, rz = z[:, :16], z[:, 32:]
    assert np.isfinite(lz).sum() > 50 and np.isfinite(rz).sum() > 50 and np.nanmax(np.abs(lz)) > 0.05 and np.nanmax(np.abs(rz)) > 0.05
    assert not np.array_equal(lz, rz, equal_nan=True)
    strip_before = ss.vertices(2)
    ss.morph(0, np.array([0.0, 0.0, 1.0], f32), refit=True)
    assert ss.vertices(1).tobytes() == got[1].tobytes() and ss.vertices(2).tobytes() == strip_before.tobytes()
    assert ss.vertices(0).tobytes() == M.morph(base, [0, 0, 1], left.position_deltas, left.normal_deltas, left.tangent_deltas).tobytes()
    # the strip: morphed, then skinned by the rest pose
    assert strip_before.tobytes() != sc.vertices[162:].tobytes()


@pytest.mark.gpu
def test_both_hosts_play_the_weights(R, ctx, tmp_path):
    """`tauray_hip morph.glb --animation --framerate=4 --frames=3` against SceneAnimator + SceneStage.animate: the same three frames, bit
    for bit; and frame 0 is not the frame of the file without its targets."""
    from tauray_amd.animation import SceneAnimator
    from tauray_amd.gltf import load_glb
    from test_accel_strategies import _dup
    W, H = 48, 32
    prefix = str(tmp_path / "m")
    subprocess.check_call([CLI, GLB, f"--width={W}", f"--height={H}", "--max-ray-depth=3", "--animation", "--framerate=4", "--frames=3", "--filetype=raw",
                           "--format=rgba32", f"--headless={prefix}"])

    def play(path, frames):
        scene = load_glb(path, W, H)
        ss = R.SceneStage(ctx, scene)
        an = SceneAnimator(scene)
        an.play("")
        pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, max_bounces=3), _dup((W, H)))
        color, disp = ctx.alloc(W * H * 16).zero(), ctx.alloc(W * H * 16)
        out = []
        for frame in range(frames):
            ss.animate(an, 0 if frame == 0 else 250000, refit=(frame % 3 != 2))      # the command line rebuilds every third frame
            pt.reset_accumulated_samples()
            pt.run(color)
            R.TonemapStage(ctx).run(color, disp, W, H)
            out.append(disp.download((H, W, 4)))
        pt.close()
        return out
    ref = play(GLB, 3)
    for frame in range(3):
        got = np.fromfile(f"{prefix}{frame}.raw", dtype=np.float32).reshape(H, W, 4)
        assert np.array_equal(got.view(np.uint32), ref[frame].view(np.uint32)), frame
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])
    doc, head, rest = _glb_json(GLB)
    for mesh in doc["meshes"]:
        mesh.pop("weights", None)
        for p in mesh["primitives"]:
            p.pop("targets")
    for node in doc["nodes"]:
        node.pop("weights", None)
    doc.pop("animations")
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    plain = str(tmp_path / "plain.glb")
    open(plain, "wb").write(head[:8] + struct.pack("<I", 12 + 8 + len(js) + len(rest)) + struct.pack("<II", len(js), 0x4E4F534A) + js + rest)
    assert not np.array_equal(play(plain, 1)[0], ref[0])
