#!/usr/bin/env python3
"""Decode the reference's golden EXRs (test/references/validate_*.exr) into
small committed fixtures under tests/golden/.

Runs only in the build container (needs /root/reference).  The decoder is
compiled in /tmp against the tinyexr header vendored by the reference; only the
decoded pixel data (float16, exactly the precision of the HALF EXRs) is
committed, as tests/golden/validate_<name>.npz.
"""
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
NAMES = ["distance", "world-pos", "view-pos", "world-normal", "view-normal", "albedo", "path-tracer"]
PIZ_FIXTURES = ("albedo", "view-normal", "path-tracer")


def main():
    exe = "/tmp/exr_to_raw"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-I", os.path.join(REF, "external"),
                           os.path.join(ROOT, "tools/exr_to_raw.cc"), "-o", exe, "-lpthread"])
    for n in NAMES:
        src = os.path.join(REF, "test/references", f"validate_{n}.exr")
        raw = f"/tmp/golden_{n}.raw"
        subprocess.check_call([exe, src, raw])
        d = open(raw, "rb").read()
        w, h = np.frombuffer(d[:8], dtype=np.int32)
        img = np.frombuffer(d[8:], dtype=np.float32).reshape(h, w, 3)
        img16 = img.astype(np.float16)
        assert np.array_equal(img16.astype(np.float32), img) or np.isnan(img).any(), "golden is not exactly half precision"
        np.savez_compressed(os.path.join(ROOT, "tests/golden", f"validate_{n}.npz"), rgb=img16)
        if n in PIZ_FIXTURES:     # the file itself (PIZ, half: written by Tauray through tinyexr) pins include/tauray_exr.hh's decoder
            shutil.copyfile(src, os.path.join(ROOT, "tests/golden", f"ref_piz_{n}.exr"))
        print(n, img.shape, "mean", img.reshape(-1, 3).mean(0), "min", img.min(), "max", img.max())


def exr_writer():
    """tests/golden/exr_tinyexr_verified.json: every file of tests/test_exr.py's tinyexr cases, written by this project's encoder and
    decoded by the reference's tinyexr; a digest is recorded only if tinyexr gave back the source pixels bit for bit."""
    import json
    import struct
    import tempfile
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_exr as T
    from tauray_amd import exr
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "exr_to_raw")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-I", os.path.join(REF, "external"),
                           os.path.join(ROOT, "tools/exr_to_raw.cc"), "-o", exe, "-lpthread"])
    f, raw = os.path.join(tmp, "a.exr"), os.path.join(tmp, "a.raw")
    verified = {}
    for key, img, alpha, half, comp in T.tinyexr_cases():
        data = exr.encode_exr(img, alpha=alpha, half=half, compression=comp)
        open(f, "wb").write(data)
        subprocess.check_call([exe, f, raw], stdout=subprocess.DEVNULL)
        d = open(raw, "rb").read()
        h, w = img.shape[:2]
        assert struct.unpack("<ii", d[:8]) == (w, h), key
        got = np.frombuffer(d[8:], dtype=np.float32).reshape(h, w, 3)
        assert np.array_equal(got.view(np.uint32), T._expected(img, False, half).view(np.uint32)), key
        verified[key] = T.normalised_digest(data, w, h, 4 if alpha else 3, half, comp)
    shutil.rmtree(tmp)
    json.dump(verified, open(os.path.join(ROOT, "tests/golden/exr_tinyexr_verified.json"), "w"), indent=0, sort_keys=True)
    print(len(verified), "files decoded by tinyexr to their source pixels")


if __name__ == "__main__":
    sys.exit(exr_writer() if sys.argv[1:] == ["--exr-writer"] else main())
