"""GPU: ORB_SLAM2::Optimizer::PoseOptimization(Frame *) (orb_slam2v2-1_amd/host/Optimizer.h) through tests/cpp/poseopt_driver.cc on a
shim Frame built from a scene file: the pose it sets, mvbOutlier and its return value are what the Python call gives."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "poseopt_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "poseopt_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def hx(x):
    return float(x).hex()


@pytest.mark.parametrize("name", ["invalid", "n2"])
def test_optimizer_class_on_a_shim_frame(pkg, driver, tmp_path, name):
    sc = S.case(name)
    obs, octave = sc["obs"], sc["octave"]
    n = len(obs)
    before = (np.arange(n) % 3 == 0).astype(np.uint8)          # mvbOutlier as the caller left it
    cam = [np.float32(c) for c in S.CAM]
    lines = [" ".join(hx(c) for c in cam), "%d %s" % (S.NLEVELS, " ".join(hx(x) for x in S.INV_SIGMA2)),
             " ".join(hx(x) for x in sc["Tcw0"].ravel()), str(n)]
    for i in range(n):
        o = obs[i]
        lines.append("%d %d %s %s %s %d %s %s %s" % (o["valid"], before[i], hx(o["u"]), hx(o["v"]), hx(o["ur"]), octave[i],
                                                     hx(o["wx"]), hx(o["wy"]), hx(o["wz"])))
    (tmp_path / "scene.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([driver, str(tmp_path / "scene.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    got = dict((ln.split()[0], ln.split()[1:]) for ln in out.stdout.strip().split("\n"))
    T, flags, ngood, info = pkg.pose_optimization(obs, S.CAM, sc["Tcw0"], outlier=before)
    assert int(got["ret"][0]) == ngood and (ngood > 50 or name == "n2")
    assert [float.fromhex(x) for x in got["pose"]] == [float(x) for x in T.ravel()]
    assert [int(x) for x in got.get("outlier", [])] == [int(x) for x in flags]
    if name == "n2":
        assert ngood == 0 and (T == sc["Tcw0"]).all() and not flags.any()
