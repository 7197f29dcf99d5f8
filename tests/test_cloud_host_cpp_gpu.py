"""GPU: PointCloudMappingHIP (orb_slam2v2-1_amd/host/PointCloudMapping.h) through tests/cpp/cloud_driver.cc on two keyframes written
to files: globalMap and the unfiltered clouds are byte for byte what the Python binding CloudMapper.keyframe_cloud returns,
concatenated."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cloud_gpu as G   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "cloud_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "cloud_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


@pytest.mark.parametrize("ch", [3, 4])
def test_two_keyframes_through_the_cpp_class(driver, pkg, tmp_path, ch):
    w, h, res = 160, 120, 0.1
    cam = G.CAM
    m = pkg.CloudMapper(res, 3, 255)
    raws, maps, counts = [], [], []
    for i in range(2):
        color, (depth, _), M = G.colour_image(w, h, ch, i), G.depth_image(w, h, "f32", i), G.pose(i + 1)
        color.tofile(tmp_path / ("kf%d.color" % i)); depth.tofile(tmp_path / ("kf%d.depth" % i)); M.tofile(tmp_path / ("kf%d.pose" % i))
        raw, out = m.keyframe_cloud(color, depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"], M)
        raws.append(raw); maps.append(out); counts.append((len(raw), len(out)))
    args = [driver, res, w, h, ch] + [repr(float(np.float32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [2, str(tmp_path / "kf"), tmp_path / "o"]
    out = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    got_counts = [tuple(int(v) for v in l.split()) for l in out.stdout.strip().splitlines()]
    assert got_counts == counts and all(c[1] > 10 for c in counts)
    assert np.fromfile(str(tmp_path / "o") + ".map", np.uint8).tobytes() == np.concatenate(maps).tobytes()
    assert np.fromfile(str(tmp_path / "o") + ".raw", np.uint8).tobytes() == np.concatenate(raws).tobytes()
