#!/usr/bin/env python3
"""Time of the Looking Glass composition stage (trhip_lkg_*, csrc/looking_glass.hip) on the GPU, next to its floor on the same box:
  * 48 views of 420 x 560 to a 1536 x 2048 panel (pitch 52.57, slope -7.19, center 0.13, DPI 324, inverted)
  * 45 views of 768 x 432 to a 3840 x 2160 panel (pitch 49.825, slope 5.2, center 0.18, DPI 283, inverted)
Per case and per set of outputs (fp32 + 8 bit, fp32 alone, 8 bit alone): the stage's own event timer (device ms of one frame; median and
minimum of `--frames` frames after 5 warm-up frames on random views) and, as the floor, a device-to-device copy of the output's bytes
(trhip_copy_peer within the device), both also as host wall time per call of `--frames` calls back to back ending in a synchronise; the
rounds alternate stage and copy.  The stage reads 12 scattered floats per output pixel besides: the ratio says what they cost.
Also: the share of (pixel, channel) entries whose recorded view differs from the float64 model's, and from the float32 model's (0 by contract).

    python tools/looking_glass_probe.py [--out profiles/r14/looking_glass.txt] [--frames 50] [--rounds 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BEGIN, END = "== tools/looking_glass_probe.py", "== end of tools/looking_glass_probe.py"

CASES = [("48 views of 420x560 -> 1536x2048", 48, (420, 560), (52.57, -7.19, 0.13, 40.0, True, 324.0, 1536, 2048)),
         ("45 views of 768x432 -> 3840x2160", 45, (768, 432), (49.825, 5.2, 0.18, 40.0, True, 283.0, 3840, 2160))]


def write_section(path, text):
    """Replaces the probe's section of the file (or appends it)."""
    old = open(path).read() if os.path.exists(path) else ""
    section = BEGIN + "\n" + text + END + "\n"
    if BEGIN in old and END in old:
        head, rest = old.split(BEGIN, 1)
        new = head + section + rest.split(END + "\n", 1)[-1]
    else:
        new = old + ("\n" if old and not old.endswith("\n\n") else "") + section
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "looking_glass.txt"))
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    from tauray_amd import _lib
    from tauray_amd import renderer as R
    from tauray_amd.looking_glass import LookingGlassCalibration
    import looking_glass_model as M

    ctx = R.Context(0)
    L = _lib.lib()
    lines = [f"device: {ctx.info()}", f"{args.frames} frames per round, {args.rounds} rounds alternating stage and copy, 5 warm-up frames", ""]
    for label, n, view, cal_values in CASES:
        cal = LookingGlassCalibration(*cal_values)
        out_size = cal.size
        px = out_size[0] * out_size[1]
        rng = np.random.default_rng(1)
        views = rng.random((n, view[1], view[0], 4), dtype=np.float32)
        src = ctx.alloc(views.nbytes).upload(views)
        dst, dst8 = ctx.alloc(px * 16), ctx.alloc(px * 4)
        copy_src, copy_dst = ctx.alloc(px * 20).zero(), ctx.alloc(px * 20).zero()      # the floor copies between two buffers that hold every output set
        lines.append(f"{label}: views {views.nbytes / 2**20:.0f} MiB, output {px * 16 / 2**20:.0f} MiB fp32 + {px * 4 / 2**20:.0f} MiB 8 bit")
        # the recorded view indices against the models
        stage = R.LookingGlassStage(ctx, view, out_size, cal.stage_options(n, record_view_indices=True))
        stage.run(src, dst, dst8)
        ctx.sync()
        idx = stage.view_indices()[..., :3]
        stage.close()
        o = cal.stage_options(n)
        args5 = (n, o["pitch"], o["tilt"], o["center"], o["invert"])
        i32, i64 = M.view_indices(out_size, *args5, dtype=np.float32)[..., :3], M.view_indices(out_size, *args5, dtype=np.float64)[..., :3]
        lines.append(f"  view indices: stage != float32 model on {(idx != i32).mean():.3e} of the (pixel, channel) entries, stage != float64 model on "
                     f"{(idx != i64).mean():.3e}, float32 model != float64 model on {(i32 != i64).mean():.3e}")
        got = dst.download((out_size[1], out_size[0], 4))
        assert np.array_equal(dst8.download((out_size[1], out_size[0], 4), np.uint8), M.quantise(got))
        del idx, i32, i64, got
        stage = R.LookingGlassStage(ctx, view, out_size, cal.stage_options(n))
        for name, a, b, nbytes in (("fp32 + 8 bit", dst, dst8, px * 20), ("fp32 alone", dst, None, px * 16), ("8 bit alone", None, dst8, px * 4)):
            def run_stage():
                stage.run(src, a, b)

            def run_copy():
                assert nbytes <= px * 20
                rc = L.trhip_copy_peer(ctx.h, copy_dst.data_ptr(), ctx.h, copy_src.data_ptr(), nbytes, None)
                assert rc == 0
            for _ in range(5):
                run_stage(); run_copy()
            ctx.sync()
            event_ms, wall = [], {"stage": [], "copy": []}
            for _ in range(args.rounds):
                for key, fn in (("stage", run_stage), ("copy", run_copy)):
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        fn()
                    ctx.sync()
                    wall[key].append((time.perf_counter() - t0) * 1e3 / args.frames)
                    if key == "stage":
                        event_ms.append(stage.timings()["total_ms"])
            s, c = float(np.median(wall["stage"])), float(np.median(wall["copy"]))
            lines.append(f"  {name:13s}: stage {s:.4f} ms per frame back to back (min {min(wall['stage']):.4f}), event timer of one frame {np.median(event_ms):.4f} ms "
                         f"(min {min(event_ms):.4f}); copy of {nbytes / 2**20:.1f} MiB {c:.4f} ms (min {min(wall['copy']):.4f}); "
                         f"ratio {s / c:.2f}; {nbytes / s / 1e6:.0f} GB/s of output written")
        stage.close()
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    write_section(args.out, text)


if __name__ == "__main__":
    main()
