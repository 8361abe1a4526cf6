"""The policy of the post-processing chain (plan_post_processing in tauray_amd/renderer.py, post_processing_renderer::make_plan in
include/tauray_hip.hh): all 32 on/off combinations of denoiser, spatial reprojection, temporal reprojection, taa and a Looking Glass output on
one device, 8 viewports, 3 of them sources.  The table below is what the renderers' constructors decided before the chain had an owner; no
device is needed."""
import itertools
import os
import subprocess

import pytest

from tauray_amd import renderer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BMFR_TARGETS = ("diffuse", "albedo", "normal", "pos", "screen_motion", "instance_id")
TAA_TARGETS = ("screen_motion", "pos", "instance_id")
SPATIAL_TARGETS = ("normal", "pos", "instance_id")
TEMPORAL_TARGETS = SPATIAL_TARGETS + ("screen_motion",)

# (denoiser, spatial, temporal, taa, looking glass) -> (stages in order, targets besides colour, frame order, fused tonemap possible)
LEGAL = {
    (0, 0, 0, 0, 0): (("tonemap",), (), False, True),
    (0, 0, 0, 0, 1): (("tonemap", "looking_glass"), (), False, False),
    (0, 0, 0, 1, 0): (("tonemap", "taa"), TAA_TARGETS, True, False),
    (0, 0, 0, 1, 1): (("tonemap", "taa", "looking_glass"), TAA_TARGETS, True, False),
    (0, 0, 1, 0, 0): (("temporal", "tonemap"), TEMPORAL_TARGETS, True, False),
    (0, 0, 1, 0, 1): (("temporal", "tonemap", "looking_glass"), TEMPORAL_TARGETS, True, False),
    (0, 1, 0, 0, 0): (("gbuffer+spatial", "tonemap"), SPATIAL_TARGETS, True, False),
    (0, 1, 0, 0, 1): (("gbuffer+spatial", "tonemap", "looking_glass"), SPATIAL_TARGETS, True, False),
    (0, 1, 1, 0, 0): (("temporal", "gbuffer+spatial", "tonemap"), TEMPORAL_TARGETS, True, False),
    (0, 1, 1, 0, 1): (("temporal", "gbuffer+spatial", "tonemap", "looking_glass"), TEMPORAL_TARGETS, True, False),
    (1, 0, 0, 0, 0): (("bmfr", "tonemap"), BMFR_TARGETS, True, False),
    (1, 0, 0, 0, 1): (("bmfr", "tonemap", "looking_glass"), BMFR_TARGETS, True, False),
    (1, 0, 0, 1, 0): (("bmfr", "tonemap", "taa"), BMFR_TARGETS, True, False),
    (1, 0, 0, 1, 1): (("bmfr", "tonemap", "taa", "looking_glass"), BMFR_TARGETS, True, False),
}
ROWS = list(itertools.product((0, 1), repeat=5))
VIEWPORTS, SOURCES = 8, [0, 3, 6]


def _refusal(row):
    """The words of the refusal, the same in both hosts: reprojection meets the denoiser first, then taa."""
    d, s, t, a, l = row
    return "a chain of reprojection and a denoiser is not built" if d else "a chain of reprojection and taa is not built"


def _chain(row):
    d, s, t, a, l = row
    from tauray_amd.looking_glass import LookingGlassCalibration, LookingGlassOutput
    lkg = None
    if l:
        cal = LookingGlassCalibration(pitch=47.6, slope=-5.4, center=0.1, view_cone=40.0, invert=False, dpi=338.0, screen_w=96, screen_h=128)
        lkg = LookingGlassOutput(calibration=cal, viewports=VIEWPORTS)
    return dict(denoiser="bmfr" if d else None, spatial_reprojection=SOURCES if s else None, temporal_reprojection=0.5 if t else 0.0,
                taa=8 if a else 0, looking_glass=lkg)


def test_the_table_is_the_whole_table():
    assert len(ROWS) == 32 and len(LEGAL) == 14 and set(LEGAL) <= set(ROWS)
    for d, s, t, a, l in LEGAL:      # any subset of {bmfr, taa, lkg}, or {spatial, temporal, both} with or without lkg
        assert not ((s or t) and (d or a))
    for row in set(ROWS) - set(LEGAL):
        d, s, t, a, l = row
        assert (s or t) and (d or a)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "".join(map(str, r)))
def test_python_plan(row):
    kw = dict(_chain(row), device_count=1, shard="pixels", viewports=VIEWPORTS, accumulate=False, frames_per_launch=1, projection=0, path_tracer=True)
    if row not in LEGAL:
        with pytest.raises(ValueError, match=_refusal(row)):
            R.plan_post_processing(**kw)
        return
    stages, targets, frame_order, fused = LEGAL[row]
    plan = R.plan_post_processing(**kw)
    assert plan.stages == stages and set(plan.stages) <= set(R.POST_STAGES)
    assert sorted(plan.targets) == sorted(targets) and len(plan.targets) == len(targets)
    assert plan.frame_order is frame_order and plan.fused_tonemap is fused
    assert plan.output_layers == VIEWPORTS
    assert plan.viewport_list == (tuple(SOURCES) if row[1] else None)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "".join(map(str, r)))
def test_the_renderer_refuses_what_the_plan_refuses(row):
    """RtRenderer without a device: a ValueError is a refusal, any other exception means the constructor got past the refusals."""
    opt = R.make_options()
    try:
        R.RtRenderer(None, None, opt, (48, 64), viewports=VIEWPORTS, **_chain(row))
        outcome = "built"
    except ValueError as e:
        outcome = "refused"
        assert _refusal(row) in str(e)
    except Exception:      # noqa: BLE001 - no context, no scene: the constructor fails somewhere behind the refusals
        outcome = "legal"
    assert outcome == ("legal" if row in LEGAL else "refused")


def test_cpp_plan_is_the_same_plan(tmp_path):
    exe = str(tmp_path / "post_processing_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DTAURAY_HIP_WITH_ZLIB", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "post_processing_plan_check.cc"), "-L" + os.path.join(ROOT, "tauray_amd"), "-ltrhip", "-lz",
                           "-Wl,-rpath," + os.path.join(ROOT, "tauray_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(lines) == 32
    seen = set()
    for line in lines:
        f = line.split(" ", 6)
        row, kind = tuple(int(x) for x in f[:5]), f[5]
        seen.add(row)
        if row not in LEGAL:
            assert kind == "refused" and _refusal(row) in f[6], line
            continue
        assert kind == "plan", line
        stages, targets, frame_order, fused, layers = f[6].split(" ")
        want = LEGAL[row]
        assert tuple(stages.split(",")) == want[0], line
        assert sorted(t for t in targets.split(",") if t != "-") == sorted(want[1]), line
        assert (frame_order, fused, layers) == (str(int(want[2])), str(int(want[3])), str(VIEWPORTS)), line
        py = R.plan_post_processing(**_chain(row), viewports=VIEWPORTS)
        assert tuple(stages.split(",")) == py.stages and sorted(t for t in targets.split(",") if t != "-") == sorted(py.targets)
        assert (int(frame_order), int(fused), int(layers)) == (int(py.frame_order), int(py.fused_tonemap), py.output_layers)
    assert seen == set(ROWS)


def test_stage_skeleton_under_the_host_sanitizers(tmp_path):
    """tests/stage_host_check.cc: the stages' host skeleton and the host side of a viewport frame (stage_host.h), a stand-alone program built
    with the address and undefined-behaviour sanitizers.  The skeleton half needs a machine without a device and says so where there is one; the viewport-frame half runs first, anywhere."""
    exe = str(tmp_path / "stage_host_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "stage_host_check.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) in ((0, "ok"), (2, "stage_host_check: this check is for a machine without a device")), r.stdout + r.stderr
