"""GPU: the raw-stereo overload of ExtractStereoFrameHIP with two StereoRectifierHIP (orb_slam2v2-1_amd/host/ORBmatcher.h) through
tests/cpp/rectify_driver.cc, on a raw colour pair: mvKeys / mDescriptors / mvKeysRight / mDescriptorsRight / mvuRight / mvDepth / N
and the match count are exactly what the Python binding ORBextractor.stereo_frame_rectified returns."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "rectify_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "rectify_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


@pytest.mark.parametrize("ch,rgb", [(3, 0), (4, 1)])
def test_raw_colour_pair_through_the_cpp_overload(driver, pkg, synth, tmp_path, ch, rgb):
    w, h = R.EUROC_SIZE
    nf, mbf, mb = 1200, 47.90639384423901, 0.11007784219
    gl, gr = synth.stereo_pair_blocky(w, h, 9)

    def colour(g, k):
        g = g.astype(np.int32)
        c = [g, (3 * g) // 4 + 40 + k, 255 - g // 2] + ([np.full_like(g, 90)] if ch == 4 else [])
        return np.stack(c, -1).astype(np.uint8)
    left, right = colour(gl, 0), colour(gr, 5)
    cams = []
    for cam in (R.EUROC_L, R.EUROC_R):
        cams += [np.ravel(cam[k]) for k in ("K", "D", "R", "P")]
    np.concatenate(cams).astype(np.float64).tofile(tmp_path / "cams.f64")
    left.tofile(tmp_path / "l.raw"); right.tofile(tmp_path / "r.raw")
    rl = pkg.StereoRectifier(R.EUROC_L["K"], R.EUROC_L["D"], R.EUROC_L["R"], R.EUROC_L["P"], w, h)
    rr = pkg.StereoRectifier(R.EUROC_R["K"], R.EUROC_R["D"], R.EUROC_R["R"], R.EUROC_R["P"], w, h)
    ref = pkg.ORBextractor(nf, 1.2, 8, 20, 7).stereo_frame_rectified(rl, rr, left, right, mbf, mb, rgb=bool(rgb))
    env = dict(os.environ)
    env.setdefault("ORBX_GAUSS_ROUNDING", os.environ.get("ORBX_TEST_GAUSS_FLAVOUR", "half_up"))   # (as tests/test_host_cpp_gpu.py)
    args = [driver, tmp_path / "l.raw", tmp_path / "r.raw", w, h, ch, rgb, tmp_path / "cams.f64", 4, repr(float(np.float32(mbf))),
            repr(float(np.float32(mb))), nf, tmp_path / "o"]
    out = subprocess.run([str(a) for a in args], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    n, nm = (int(v) for v in out.stdout.split()[:2])
    base = str(tmp_path / "o")
    got = {"kl": np.fromfile(base + ".kl", pkg.KP_DTYPE), "kr": np.fromfile(base + ".kr", pkg.KP_DTYPE),
           "dl": np.fromfile(base + ".dl", np.uint8).reshape(-1, 32), "dr": np.fromfile(base + ".dr", np.uint8).reshape(-1, 32),
           "uright": np.fromfile(base + ".uright", np.float32), "depth": np.fromfile(base + ".depth", np.float32)}
    assert n == len(ref["kl"]) > 200 and nm == ref["nmatch"] > 5
    for f in got:
        assert got[f].tobytes() == ref[f].tobytes(), f
