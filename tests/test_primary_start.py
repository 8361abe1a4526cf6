"""The primary start (trhip_pt_set_primary_start): under AUTO a pass launches no k_raygen - the closest-hit launch of
bounce 0 derives every path's start from its launch id and stores the path state - and the lanes' counters are zeroed by the resolve launch
of the pass before.  Frames must not depend on the mode: every comparison here is byte equality of the colour target and of the fused
tonemapped display between AUTO and OFF in one process, on frames small enough that what can go wrong is indexing, validity, sampler
state and the hand-over of the counters."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, OFF = 0, 1
NAMES = ("trhip_pt_set_primary_start", "trhip_pt_get_primary_start", "trhip_sh_get_primary_start")


# ---------------------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_entry_points_declared_exported_and_bound(tmp_path):
    from tauray_amd import _lib, renderer
    header = open(os.path.join(ROOT, "include", "trhip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    for m, v in (("TRHIP_PRIMARY_START_AUTO", 0), ("TRHIP_PRIMARY_START_OFF", 1)):
        assert re.search(r"#define %s %d\b" % (m, v), header), m
    assert (_lib.PRIMARY_START_AUTO, _lib.PRIMARY_START_OFF) == (AUTO, OFF)
    src = tmp_path / "sz.c"
    src.write_text('#include "trhip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(trhip_primary_start_info), offsetof(trhip_primary_start_info, in_effect), offsetof(trhip_primary_start_info, last_frame)); '
                   'return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_effect, off_last = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_lib.PrimaryStartInfoC) == 16
    assert off_effect == _lib.PrimaryStartInfoC.in_effect.offset and off_last == _lib.PrimaryStartInfoC.last_frame.offset
    for attr in ("set_primary_start", "primary_start"):
        assert callable(getattr(renderer.PathTracerStage, attr)), attr
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tauray_amd", "libtrhip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"{name} is not exported"


# ---------------------------------------------------------------------------------------------------------------------------------
# on the GPU

@pytest.fixture(scope="module")
def R():
    from tauray_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    return R.Context(0)


_SCENES = {}


def _glb(R, ctx, size):
    """test.glb (a glass object among opaque ones, a sphere light) with its camera at `size`, and its scene stage: built once per size"""
    if size not in _SCENES:
        from tauray_amd.gltf import load_glb
        sc = load_glb(os.path.join(GOLDEN, "test.glb"), *size)
        _SCENES[size] = (sc, R.SceneStage(ctx, sc))
    return _SCENES[size]


def _dup(size):
    from tauray_amd.distribution import DistributionParams, DISTRIBUTION_DUPLICATE
    return DistributionParams(tuple(size), DISTRIBUTION_DUPLICATE, 0, 1, True)


def _sequence(R, ctx, ss, scene, size, modes, dist=None, views=1, batch=1, lanes=0, ieee=None, specialize=None, before=None, expect=None, **kw):
    """Renders len(modes) frames on one stage, frame f under modes[f]; `before[f]`(pt) runs ahead of frame f.  Returns the frames as
    (colour, display) byte arrays, and the stage's counters.  expect: what the stage must report for an AUTO frame (True: the primary
    start ran); a list gives it frame by frame."""
    from tauray_amd import _lib
    from tauray_amd.distribution import get_distribution_target_size
    from tauray_amd.renderer import TONEMAP_FILMIC
    dist = dist or _dup(size)
    tw, th = get_distribution_target_size(dist)
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(scene, **kw), dist)
    if lanes:
        pt.set_lanes(lanes)
    if ieee is not None:
        pt.set_shading_arithmetic(ieee)
    if specialize is not None:
        pt.set_specialization(specialize)
    if batch > 1:
        pt.set_frame_batch(batch)
    layers = views * batch
    color = ctx.alloc(layers * tw * th * 16).zero()
    display = ctx.alloc(layers * tw * th * 16).zero()
    pt.set_fused_tonemap(display, _lib.TonemapInfoC(TONEMAP_FILMIC, 1.0, 2.2, 0))
    pt.reset_counters()
    frames = []
    for f, mode in enumerate(modes):
        pt.set_primary_start(mode)
        if before and before.get(f):
            before[f](pt)
        want = bool(expect[f] if isinstance(expect, (list, tuple)) else expect) and mode == AUTO
        assert pt.primary_start()["in_effect"] == want, (f, mode, pt.primary_start())
        pt.run(color, layers)
        frames.append((color.download((layers, th, tw, 4)).view(np.uint32).copy(), display.download((layers, th, tw, 4)).view(np.uint32).copy()))
        assert pt.primary_start()["last_frame"] == int(want), (f, mode, pt.primary_start())
    c = pt.counters()
    pt.close()
    assert c["stack_overflows"] == 0
    return frames, c


# the options that keep a stage on the command-line option set - the set the primary launch exists for; any other option set is an "off" condition
CLI_KEYS = {"max_bounces", "samples_per_pixel", "samples_per_pass", "rng_seed"}


def _same(R, ctx, ss, scene, size, what, n_frames=1, expect=None, **kw):
    """n_frames under OFF, then the same frames under AUTO: same bytes, same ray counts.  Returns the frames.
    expect: whether AUTO must be in effect; by default, whether the stage renders the command-line option set with its ahead-of-time kernels."""
    if expect is None:
        other = {k for k, v in kw.items() if not (k in ("sampler", "film", "depth_of_field") and v == 0)}
        expect = not (other - CLI_KEYS - {"dist", "views", "batch", "lanes", "ieee", "specialize", "before"})
    off, c_off = _sequence(R, ctx, ss, scene, size, [OFF] * n_frames, expect=expect, **kw)
    auto, c_auto = _sequence(R, ctx, ss, scene, size, [AUTO] * n_frames, expect=expect, **kw)
    assert (off[0][0].view(np.float32)[..., :3] > 0).any(), what         # not a black frame (one bounce shows the emitters only)
    for f in range(n_frames):
        for k, name in ((0, "color"), (1, "display")):
            assert np.array_equal(off[f][k], auto[f][k]), f"{what}: frame {f}, {name}: {int((off[f][k] != auto[f][k]).any(-1).sum())} pixels differ"
    for k in ("closest_rays", "shadow_rays"):
        assert c_off[k] == c_auto[k], (what, k, c_off[k], c_auto[k])
    assert c_off["closest_rays"] > 0, what
    return auto


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(70, 33), (96, 64)])
def test_partial_chunk(R, ctx, size):
    """A frame that is not a multiple of 64 paths and not whole 8x8 tiles, and one that is: test.glb at 4 bounces (the glass object's
    any-hit seed comes out of the start from bounce 1 on)."""
    sc, ss = _glb(R, ctx, size)
    _same(R, ctx, ss, sc, size, f"test.glb {size}", max_bounces=4)


@pytest.mark.gpu
@pytest.mark.parametrize("film", [0, 1, 2])
@pytest.mark.parametrize("dof", [0, 1])
def test_film_and_lens(R, ctx, film, dof):
    """Point film without a lens is the command-line set: AUTO is in effect and must render OFF's bytes.  Every other case here is an "off"
    condition - box and Blackman-Harris film, depth of field: the stage must report the stored start under AUTO and render the same bytes.
    (The primary launch exists for the command-line set only; no launched kernel runs path_start's film and lens code but k_raygen.)"""
    sc, ss = _glb(R, ctx, (70, 33))
    _same(R, ctx, ss, sc, (70, 33), f"film {film} dof {dof}", max_bounces=3, film=film, depth_of_field=dof)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", [0, 1, 2, 3])
def test_samplers(R, ctx, sampler):
    """Uniform random is the command-line set: AUTO in effect, OFF's bytes.  Sobol-Owen and Sobol-Z2 / Z3 are "off" conditions: the stage
    reports the stored start under AUTO and renders the same bytes (a check of the report, not of path_start's samplers in the trace kernel)."""
    sc, ss = _glb(R, ctx, (70, 33))
    _same(R, ctx, ss, sc, (70, 33), f"sampler {sampler}", n_frames=2, max_bounces=4, sampler=sampler)


@pytest.mark.gpu
def test_programs(R, ctx):
    """The command-line set in both arithmetics: the mode is in effect.  A run-time compiled option set and the general kernels are "off"
    conditions: they keep the stored start (their ray generation is specialised or general with them), and these cases check that they say so,
    not the primary launch.  First-hit targets render the same under both modes."""
    sc, ss = _glb(R, ctx, (70, 33))
    for ieee in (False, True):
        _same(R, ctx, ss, sc, (70, 33), f"command-line set, ieee={ieee}", max_bounces=4, ieee=ieee)
    for kw in (dict(sampler=1), dict(film=2, film_radius=1.0)):
        pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=4, **kw), _dup((70, 33)))
        assert pt.program()["kind"] == "compiled", pt.program()
        pt.set_specialization(False)
        assert pt.program()["kind"] == "general", pt.program()
        pt.close()
        _same(R, ctx, ss, sc, (70, 33), f"compiled option set {kw}", max_bounces=4, **kw)
        _same(R, ctx, ss, sc, (70, 33), f"general kernels {kw}", max_bounces=4, specialize=False, **kw)
    # first-hit targets: the same colour and the same albedo / instance ids in both modes (k_first_hit_gbuffer reads the stored `misc`)
    frames = {}
    for mode in (OFF, AUTO):
        pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=4), _dup((70, 33)))
        pt.set_primary_start(mode)
        bufs = {n: ctx.alloc(70 * 33 * 4 * ch).zero() for n, ch in (("color", 4), ("albedo", 4), ("instance_id", 1))}
        pt.run_targets(bufs)
        info = pt.primary_start()
        assert info["last_frame"] == int(mode == AUTO), info
        frames[mode] = [bufs["color"].download((33, 70, 4)).view(np.uint32), bufs["albedo"].download((33, 70, 4)).view(np.uint32),
                        bufs["instance_id"].download((33, 70), np.int32)]
        pt.close()
    for a, b in zip(frames[OFF], frames[AUTO]):
        assert np.array_equal(a, b)
    assert (frames[OFF][2] >= 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2])
def test_bounces(R, ctx, bounces):
    """One bounce: the first launch is the last (no terminal query).  Two: the terminal launch reads the seed the first launch stored."""
    sc, ss = _glb(R, ctx, (70, 33))
    _same(R, ctx, ss, sc, (70, 33), f"{bounces} bounce(s)", max_bounces=bounces)
    from tauray_amd import scenes
    sc2 = scenes.sponza_class(3, 20_000, 0, 96, 64)          # no sphere light: the terminal query is in effect at two bounces
    _same(R, ctx, R.SceneStage(ctx, sc2), sc2, (96, 64), f"sponza_class, {bounces} bounce(s)", max_bounces=bounces)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_lanes(R, ctx, lanes):
    """One lane and four; from the second frame on the four lanes of a frame this short are enqueued in step (OFF: one merged k_raygen)."""
    sc, ss = _glb(R, ctx, (70, 33))
    _same(R, ctx, ss, sc, (70, 33), f"{lanes} lane(s)", n_frames=3, max_bounces=4, lanes=lanes)


@pytest.mark.gpu
def test_shards(R, ctx):
    """Rank 1 of 2 with scanline and with shuffled strips (launch ids without a pixel, an id offset per lane), and two viewports: same bytes
    in both modes, and the pixels of the unsharded frame."""
    from tauray_amd import distribution as D
    from tauray_amd.scene import generate_camera_grid
    import copy
    W, H = 70, 33
    sc, ss = _glb(R, ctx, (W, H))
    full = _same(R, ctx, ss, sc, (W, H), "whole frame", max_bounces=3)[0][0][0]
    for strategy in (D.DISTRIBUTION_SCANLINE, D.DISTRIBUTION_SHUFFLED_STRIPS):
        d = D.get_device_distribution_params((W, H), strategy, 1 / 2, 1 / 2, 1, 2, False)
        tw, th = D.get_distribution_target_size(d)
        for lanes in (1, 4):
            part = _same(R, ctx, ss, sc, (W, H), f"rank 1 of 2, strategy {strategy}, {lanes} lanes", dist=d, lanes=lanes, max_bounces=3)[0][0][0]
            if strategy == D.DISTRIBUTION_SCANLINE:
                ys = np.arange(th) * d.count + d.index
                ys, xs, ok = np.repeat(ys, tw), np.tile(np.arange(tw), th), np.repeat(ys < H, tw)
            else:
                b = D.calculate_shuffled_strips_b((W, H))
                j = np.array([D.permute_region_id(d.index + int(q), d.size, b) if q < d.count else W * H for q in range(tw * th)])
                ok = j < W * H
                j = np.where(ok, j, 0)
                ys, xs = j // W, j % W
            assert np.array_equal(part.reshape(-1, 4)[ok], full[np.where(ok, ys, 0)[ok], xs[ok]]), f"strategy {strategy}, {lanes} lanes: not the unsharded frame's pixels"
    sc2 = copy.copy(sc)
    sc2.cameras = generate_camera_grid(sc.cameras[0], 2, 1, 0.2, 0.2, 5.0)
    two = _same(R, ctx, R.SceneStage(ctx, sc2), sc2, (W, H), "two viewports", views=2, lanes=4, max_bounces=3)[0][0]
    assert not np.array_equal(two[0], two[1])


@pytest.mark.gpu
def test_counter_hand_over(R, ctx):
    """Who zeroes a lane's queue lengths and cursors changes with the mode: consecutive frames, a reset, several one-sample passes per
    frame, two frames per launch, and a stage that changes its mode between frames all render what they render under OFF."""
    sc, ss = _glb(R, ctx, (70, 33))
    size = (70, 33)
    for lanes in (1, 4):
        _same(R, ctx, ss, sc, size, f"three frames, {lanes} lanes", n_frames=3, max_bounces=4, lanes=lanes)
        reset = {2: lambda pt: (pt.reset_accumulated_samples(), pt.reset_sample_counter())}
        _same(R, ctx, ss, sc, size, f"a frame after a reset, {lanes} lanes", n_frames=3, max_bounces=4, lanes=lanes, before=reset)
        fresh = {f: (lambda pt: pt.reset_accumulated_samples()) for f in range(4)}
        ref = _same(R, ctx, ss, sc, size, f"two frames per launch, {lanes} lanes", n_frames=2, max_bounces=4, lanes=lanes, batch=2, before=fresh)
        # a stage switched AUTO -> OFF -> AUTO -> AUTO between frames: the frames of a stage that never switched
        plain = _sequence(R, ctx, ss, sc, size, [OFF] * 4, max_bounces=4, lanes=lanes)[0]
        mixed = _sequence(R, ctx, ss, sc, size, [AUTO, OFF, AUTO, AUTO], expect=True, max_bounces=4, lanes=lanes)[0]
        for f in range(4):
            assert np.array_equal(plain[f][0], mixed[f][0]) and np.array_equal(plain[f][1], mixed[f][1]), (lanes, f)
        assert ref[0][0].shape[0] == 2
    # The lane count changes across a mode change: the lanes a stage has not run yet hold counters nobody has zeroed (the buffer is not
    # cleared when it is allocated; a probe stage that ran four lanes and was closed first leaves its own behind for the allocator to hand out).
    from tauray_amd.scene import ShGrid
    sh = R.ShPathTracerStage(ctx, ss, ShGrid(resolution=(4, 2, 4)), dict(max_bounces=4, samples_per_probe=64, sh_order=1))
    sh.set_lanes(4)
    sh.run()
    sh.counters()
    sh.close()
    one_then_four = lambda first: {0: lambda pt: (first(pt), pt.set_lanes(1)), 1: lambda pt: (pt.set_profiling(False, False), pt.set_lanes(4))}
    for what, first, modes, expect in (("a timed frame on one lane, then AUTO on four", lambda pt: pt.set_profiling(detailed_timing=True), [AUTO, AUTO, AUTO], [False, True, True]),
                                       ("a counted frame on one lane, then AUTO on four", lambda pt: pt.set_profiling(count_work=True), [AUTO, AUTO, AUTO], [False, True, True]),
                                       ("OFF on one lane, then AUTO on four", lambda pt: None, [OFF, AUTO, AUTO], True)):
        plain = _sequence(R, ctx, ss, sc, size, [OFF] * 3, max_bounces=4, before=one_then_four(first))[0]
        mixed = _sequence(R, ctx, ss, sc, size, modes, expect=expect, max_bounces=4, before=one_then_four(first))[0]
        for f in range(3):
            assert np.array_equal(plain[f][0], mixed[f][0]) and np.array_equal(plain[f][1], mixed[f][1]), (what, f)
    # ... and four lanes, then two, then four again
    lanes_424 = {0: lambda pt: pt.set_lanes(4), 1: lambda pt: pt.set_lanes(2), 2: lambda pt: pt.set_lanes(4)}
    plain = _sequence(R, ctx, ss, sc, size, [OFF] * 3, max_bounces=4, before=lanes_424)[0]
    mixed = _sequence(R, ctx, ss, sc, size, [AUTO, OFF, AUTO], expect=True, max_bounces=4, before=lanes_424)[0]
    for f in range(3):
        assert np.array_equal(plain[f][0], mixed[f][0]) and np.array_equal(plain[f][1], mixed[f][1]), ("4-2-4 lanes", f)
    # three one-sample passes per frame: sample lanes by default, one lane after the other with set_lanes
    for lanes in (0, 1, 4):
        _same(R, ctx, ss, sc, size, f"three passes, lanes={lanes}", n_frames=2, max_bounces=4, lanes=lanes, samples_per_pixel=3, samples_per_pass=1)


@pytest.mark.gpu
def test_conditions(R, ctx):
    """Where k_raygen does more than start paths, or is what gets measured, the stored start runs under AUTO too - and says so."""
    sc, ss = _glb(R, ctx, (70, 33))
    size = (70, 33)
    _same(R, ctx, ss, sc, size, "two samples per pass", expect=False, max_bounces=3, samples_per_pixel=2, samples_per_pass=2)
    _same(R, ctx, ss, sc, size, "work counting", expect=False, max_bounces=3, before={0: lambda pt: pt.set_profiling(count_work=True)})
    _same(R, ctx, ss, sc, size, "detailed timing", expect=False, max_bounces=3, before={0: lambda pt: pt.set_profiling(detailed_timing=True)})
    # a stage that leaves a condition: the mode comes into effect on the next frame
    off = _sequence(R, ctx, ss, sc, size, [OFF, OFF], max_bounces=3)[0]
    pt_steps = {0: lambda pt: pt.set_profiling(count_work=True), 1: lambda pt: pt.set_profiling(count_work=False)}
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=3), _dup(size))
    color = ctx.alloc(size[0] * size[1] * 16).zero()
    got = []
    for f in range(2):
        pt_steps[f](pt)
        assert pt.primary_start()["in_effect"] == (f == 1)
        pt.run(color)
        got.append(color.download((1, size[1], size[0], 4)).view(np.uint32).copy())
        assert pt.primary_start()["last_frame"] == f
    pt.close()
    for f in range(2):
        assert np.array_equal(got[f], off[f][0]), f
    # the direct stage has its own schedule, the probe stage its own ray generation: both render with the stored start and report it
    d = R.DirectStage(ctx, ss, R.options_for_scene(sc, max_bounces=3), _dup(size))
    assert d.primary_start()["in_effect"] is False and d.primary_start()["last_frame"] == -1
    d.run(ctx.alloc(size[0] * size[1] * 16).zero())
    assert d.primary_start()["last_frame"] == 0, d.primary_start()
    d.close()
    from tauray_amd.scene import ShGrid
    sh = R.ShPathTracerStage(ctx, ss, ShGrid(resolution=(2, 1, 2)), dict(max_bounces=2, samples_per_probe=16, sh_order=1))
    assert sh.primary_start()["in_effect"] is False and sh.primary_start()["last_frame"] == -1
    sh.run()
    assert sh.primary_start()["last_frame"] == 0, sh.primary_start()
    # a two-level structure: the primary launch walks the all-merged one only
    ss2 = R.SceneStage(ctx, sc, as_strategy=1)
    _same(R, ctx, ss2, sc, size, "two-level structure", expect=False, max_bounces=3)
    with pytest.raises(R.TrhipError, match="unknown mode"):
        R.PathTracerStage(ctx, ss, R.options_for_scene(sc, max_bounces=3), _dup(size)).set_primary_start(2)


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_primary_start as T
from tauray_amd import renderer as R
ctx = R.Context(0)
size = (70, 33)
sc, ss = T._glb(R, ctx, size)
kw = dict(max_bounces=4, sampler=int(sys.argv[2]))
if sys.argv[3] == "error":
    pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, **kw), T._dup(size))
    try:
        pt.run(ctx.alloc(size[0] * size[1] * 16).zero())
        print("RENDERED")
    except R.TrhipError as e:
        print("ERROR", e)
    pt.set_primary_start(T.OFF)          # a mode that was set wins over the environment
    pt.run(ctx.alloc(size[0] * size[1] * 16).zero())
    print("SETTER WINS")
    sys.exit(0)
pt = R.PathTracerStage(ctx, ss, R.options_for_scene(sc, **kw), T._dup(size))       # no mode set: the environment decides
print("IN_EFFECT", int(pt.primary_start()["in_effect"]), "KIND", pt.program()["kind"])
pt.close()
T._same(R, ctx, ss, sc, size, "child", n_frames=3, expect=kw["sampler"] == 0, **kw)
print("SAME")
"""


def _child(env, sampler=0, what="same"):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(sampler), what], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("env,sampler,kind", [({"TRHIP_SPECIALIZE": "0"}, 1, "general"), ({"TRHIP_LANES": "1", "TRHIP_LANES_MIN_PATHS": "1"}, 0, "cli"),
                                              ({"TRHIP_LANES": "4", "TRHIP_LANES_MIN_PATHS": "1"}, 0, "cli"), ({"TRHIP_PRIMARY_START": "Off"}, 0, "cli")])
def test_process_wide_switches(env, sampler, kind):
    """The general kernels of a process (TRHIP_SPECIALIZE=0), one and four lanes chosen by the environment, and TRHIP_PRIMARY_START=off for a
    stage on which no mode was set (a setter still wins)."""
    out = _child(env, sampler)
    assert "SAME" in out and f"KIND {kind}" in out, out
    assert f"IN_EFFECT {1 if kind == 'cli' and 'TRHIP_PRIMARY_START' not in env else 0}" in out, out


@pytest.mark.gpu
def test_unknown_environment_value_fails_the_render():
    out = _child({"TRHIP_PRIMARY_START": "on"}, what="error")
    assert "ERROR" in out and "TRHIP_PRIMARY_START" in out and "RENDERED" not in out and "SETTER WINS" in out, out
