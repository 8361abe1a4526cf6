"""The Looking Glass output of the reference (`--display=looking-glass`, src/looking_glass.{hh,cc}) without the device: the calibration of
a lenticular panel as `--lkg-calibration` gives it, the camera rig of looking_glass::setup_cameras (src/looking_glass.cc:62-88) and what
RtRenderer(looking_glass=...) takes.  The composition stage itself is renderer.LookingGlassStage (trhip_lkg_*, csrc/looking_glass.hip)."""
import math
from dataclasses import dataclass
from typing import List

import numpy as np

from . import scene as S


def _f32(x) -> float:
    return float(np.float32(x))


@dataclass
class LookingGlassCalibration:
    """looking_glass::device_metadata from options::calibration_data (src/looking_glass.cc:216-242).  The values are the float32 numbers the
    command line holds; corrected_pitch and tilt are evaluated at double from them and rounded to float32 once, in both hosts."""
    pitch: float
    slope: float
    center: float
    view_cone: float
    invert: bool
    dpi: float
    screen_w: int
    screen_h: int

    def __post_init__(self):
        for n in ("pitch", "slope", "center", "view_cone", "dpi"):
            setattr(self, n, _f32(getattr(self, n)))
        self.screen_w, self.screen_h, self.invert = int(self.screen_w), int(self.screen_h), bool(self.invert)
        if self.screen_w < 1 or self.screen_h < 1:
            raise ValueError("LookingGlassCalibration: the screen size must be positive")
        if not (self.dpi > 0.0) or self.slope == 0.0 or not all(math.isfinite(v) for v in (self.pitch, self.slope, self.center, self.view_cone, self.dpi)):
            raise ValueError("LookingGlassCalibration: DPI must be positive, the slope non-zero and every value finite")

    @property
    def corrected_pitch(self) -> float:
        return _f32(self.screen_w / self.dpi * self.pitch * math.sin(math.atan(abs(self.slope))))

    @property
    def tilt(self) -> float:
        return _f32(self.screen_h / (self.screen_w * self.slope))

    @property
    def size(self):
        return (self.screen_w, self.screen_h)

    def stage_options(self, viewports: int, record_view_indices: bool = False) -> dict:
        """The options of renderer.LookingGlassStage for a rig of `viewports` views."""
        return dict(viewport_count=int(viewports), pitch=self.corrected_pitch, tilt=self.tilt, center=self.center, invert=self.invert,
                    record_view_indices=record_view_indices)


# the fields of --lkg-calibration, in the reference's order (src/options.hh, options::calibration_data)
CALIBRATION_FIELDS = ("display_index", "pitch", "slope", "center", "fringe", "viewCone", "invView", "verticalAngle", "DPI", "screenW", "screenH",
                      "flipImageX", "flipImageY", "flipSubp")


def parse_struct_option(option: str, text: str, names) -> dict:
    """A struct option of the reference (TR_STRUCT_OPT): comma-separated numbers, positional in the order of `names` or name=value."""
    out, position = {}, 0
    for tok in text.split(","):
        if "=" in tok:
            name, tok = tok.split("=", 1)
            if name not in names:
                raise ValueError(f"{option}: {name} is not one of its fields")
        else:
            if position >= len(names):
                raise ValueError(f"{option}: more than {len(names)} values")
            name, position = names[position], position + 1
        try:
            out[name] = float(tok)
        except ValueError:
            raise ValueError(f"{option}: {name}={tok} is not a number") from None
    return out


def parse_calibration(text: str) -> LookingGlassCalibration:
    """`--lkg-calibration=display_index,pitch,slope,center,fringe,viewCone,invView,verticalAngle,DPI,screenW,screenH,flipImageX,flipImageY,
    flipSubp`: the fields the reference ignores (display_index, fringe, verticalAngle, the flips) are parsed and ignored."""
    v = dict(dict.fromkeys(CALIBRATION_FIELDS, 0.0), **parse_struct_option("--lkg-calibration", text, CALIBRATION_FIELDS))
    if not (1 <= v["screenW"] <= 16384) or not (1 <= v["screenH"] <= 16384):
        raise ValueError("--lkg-calibration: screenW and screenH must be in 1..16384")
    return LookingGlassCalibration(v["pitch"], v["slope"], v["center"], v["viewCone"], v["invView"] > 0.5, v["DPI"], int(v["screenW"]), int(v["screenH"]))


def parse_params(text: str, calibration: LookingGlassCalibration) -> "LookingGlassOutput":
    """`--lkg-params=viewports,midplane,depth,relative_dist` (48, 2, 2, 2)."""
    v = dict(dict(viewports=48.0, midplane=2.0, depth=2.0, relative_dist=2.0), **parse_struct_option("--lkg-params", text, ("viewports", "midplane", "depth", "relative_dist")))
    if not (1 <= v["viewports"] <= 255) or v["viewports"] != math.floor(v["viewports"]):
        raise ValueError("--lkg-params: viewports must be a whole number in 1..255 (the composition stage's limit)")
    if not all(v[n] >= 0.001 for n in ("midplane", "depth", "relative_dist")):
        raise ValueError("--lkg-params: midplane, depth and relative_dist must be at least 0.001")
    return LookingGlassOutput(calibration, int(v["viewports"]), v["midplane"], v["depth"], v["relative_dist"])


@dataclass
class LookingGlassOutput:
    """What RtRenderer(looking_glass=...) takes: the panel and the reference's --lkg-params (viewports, midplane, depth, relative_dist;
    defaults 48, 2, 2, 2)."""
    calibration: LookingGlassCalibration
    viewports: int = 48
    midplane: float = 2.0
    depth: float = 2.0
    relative_dist: float = 2.0
    record_view_indices: bool = False

    def __post_init__(self):
        self.viewports = int(self.viewports)
        if not (1 <= self.viewports <= 255):
            raise ValueError(f"LookingGlassOutput: {self.viewports} viewports: the composition stage takes 1..255")
        if not (self.relative_dist > 0.0):
            raise ValueError("LookingGlassOutput: relative_dist must be positive")


RIG_NEAR, RIG_FAR = 0.01, 300.0


def rig_view(i: int, viewports: int, midplane: float, depthiness: float, relative_dist: float, calibration: LookingGlassCalibration):
    """View i of looking_glass::setup_cameras: (vertical fov in degrees, aspect, pan.x, local position).  Evaluated at double, operation for
    operation as the C++ host does it (looking_glass_cameras of include/tauray_gltf.hh): both hosts then pack the same bytes."""
    vfov = 2.0 * math.atan(1.0 / (2.0 * relative_dist)) * 180.0 / math.pi
    aspect = calibration.screen_w / float(calibration.screen_h)
    offset = ((i + 0.5) / viewports) * 2.0 - 1.0
    angle = offset * calibration.view_cone * depthiness
    pan = -math.tan(angle * (math.pi / 180.0))
    # dir = P * (0, 0, 1, 1) with P the panned projection: (pan, 0, P[2][2] + P[2][3], -1); dir /= dir.z
    zc = -(RIG_FAR + RIG_NEAR) / (RIG_FAR - RIG_NEAR) + -(2.0 * RIG_FAR * RIG_NEAR) / (RIG_FAR - RIG_NEAR)
    position = (midplane * (pan / zc), midplane * (0.0 / zc), midplane * 1.0)
    return vfov, aspect, pan, position


def looking_glass_cameras(scene, viewports: int, midplane: float, depthiness: float, relative_dist: float,
                          calibration: LookingGlassCalibration) -> List[S.Camera]:
    """looking_glass::setup_cameras (src/looking_glass.cc:62-88): replaces the scene's cameras by the rig of `viewports` panned perspective
    cameras under the reference frame, which is the scene's first camera; `scene.camera_rig` keeps the views' local transforms, so that
    the rig follows the animation of that camera's node (animation.SceneAnimator).  Returns the new cameras."""
    if not scene.cameras:
        raise ValueError("looking_glass_cameras: the scene has no camera to hang the rig on")
    if viewports < 1:
        raise ValueError("looking_glass_cameras: the rig needs at least one view")
    # a scene that already carries a rig (a second renderer over the same scene) keeps its reference frame
    frame = np.asarray(scene.cameras[0].transform if getattr(scene, "camera_rig", None) is None else scene.camera_rig_frame, dtype=np.float64)
    cams, rig = [], []
    for i in range(viewports):
        vfov, aspect, pan, position = rig_view(i, viewports, midplane, depthiness, relative_dist, calibration)
        local = np.eye(4)
        local[:3, 3] = position
        cams.append(S.Camera(transform=frame @ local, projection=S.PROJ_PERSPECTIVE, fov=vfov, aspect=aspect, near=RIG_NEAR, far=RIG_FAR,
                             fov_offset=(pan, 0.0), closed_form_inverse=True))
        rig.append(local)
    scene.cameras = cams
    scene.camera_rig, scene.camera_rig_frame = rig, frame
    return cams
