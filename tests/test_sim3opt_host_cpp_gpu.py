"""GPU: ORB_SLAM2::Optimizer::OptimizeSim3 (orb_slam2v2-1_amd/host/Optimizer.h) through tests/cpp/sim3opt_driver.cc on shim KeyFrames and
MapPoints built from a scene file, with null matches, a keyframe-1 slot without a map point, a bad point on either side and a point
not observed in keyframe 2 among them: vpMatches1 is nulled exactly where the Python call drops, the return value and g2oS12 are the
C ABI's result bit for bit, g2oS12 is untouched on a 0 return, and the caller's next lines (src/LoopClosing.cc:343-345) compile and
compute Scw = Scm * Smw."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3opt_ref as R        # noqa: E402
import sim3opt_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "sim3opt_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "sim3opt_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def hx(x):
    return float(x).hex()


def vec(words):
    return np.array([float.fromhex(w) for w in words])


@pytest.mark.parametrize("name", ["out65", "drop_below10"])
def test_optimizer_class_on_shim_keyframes(pkg, driver, tmp_path, name):
    sc = S.case(name)
    m, pr, octave = sc["matches"], sc["prob"], sc["octave"]
    n = len(m)
    kind = np.ones(n, int)
    if name == "out65":
        kind[np.arange(n) % 11 == 3] = 0
        kind[[5, 17, 29, 40]] = [2, 3, 4, 5]
    lines = [" ".join(hx(x) for x in pr["K1"]), " ".join(hx(x) for x in pr["K2"]),
             "%d %s" % (S.NLEVELS, " ".join(hx(x) for x in S.INV_SIGMA2)), " ".join(hx(x) for x in pr["Tcw1"]),
             " ".join(hx(x) for x in pr["Tcw2"]), " ".join(hx(x) for x in pr["R"]), " ".join(hx(x) for x in pr["t"]),
             "%s %s %d" % (hx(pr["s"]), hx(pr["th2"]), pr["fix_scale"]), str(n)]
    for i in range(n):
        assert m["inv_sigma2_1"][i] == S.INV_SIGMA2[octave[i, 0]] and m["inv_sigma2_2"][i] == S.INV_SIGMA2[octave[i, 1]]
        lines.append("%d %s %s %d %s %s %s %d %s" % (kind[i], hx(m["u1"][i]), hx(m["v1"][i]), octave[i, 0], " ".join(hx(x) for x in m["w1"][i]),
                                                     hx(m["u2"][i]), hx(m["v2"][i]), octave[i, 1], " ".join(hx(x) for x in m["w2"][i])))
    (tmp_path / "scene.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([driver, str(tmp_path / "scene.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    got = dict((ln.split()[0], ln.split()[1:]) for ln in out.stdout.strip().split("\n"))
    # the class hands g2oS12 to the C ABI as float R, t, s: (float)toRotationMatrix() of Quaterniond(R), t and s as they were
    start = R.Sim3.from_Rts(pr["R"], pr["t"], pr["s"])
    assert vec(got["start"]).tobytes() == start.vec().tobytes()
    p2 = pr.copy()
    p2["R"] = R.quat_to_R(start.q).astype(np.float32).reshape(9)
    assert np.abs(p2["R"] - pr["R"]).max() < 1e-6
    rows = np.nonzero(kind == 1)[0]
    T, dropped, ni, info = pkg.optimize_sim3(m[rows], p2)
    expect_null = kind == 0
    expect_null[rows] = dropped != 0
    assert [int(x) for x in got["null"]] == [int(x) for x in expect_null]
    assert int(got["ret"][0]) == ni
    if name == "out65":
        assert info["rounds"] == 2 and ni > 30 and dropped.any() and info["correspondences"] == len(rows) == n - 6 - 4
        sim3 = R.Sim3(info["q"], info["t"], info["s"])
        assert vec(got["sim3"]).tobytes() == sim3.vec().tobytes()
        assert [float.fromhex(x) for x in got["mat"]] == [float(x) for x in T.ravel()]
    else:
        assert info["rounds"] == 1 and ni == 0 and dropped.sum() == 6
        sim3 = start
        assert vec(got["sim3"]).tobytes() == start.vec().tobytes()          # a 0 return leaves g2oS12 untouched
    # src/LoopClosing.cc:343-345 on the shim: Scw = Scm * Smw with Smw = Sim3(R2w, t2w, 1.0)
    T2 = np.asarray(pr["Tcw2"], np.float32).reshape(4, 4)
    scw = sim3 * R.Sim3.from_Rts(T2[:3, :3], T2[:3, 3], 1.0)
    assert vec(got["scw"]).tobytes() == scw.vec().tobytes()
    assert [float.fromhex(x) for x in got["mscw"]] == [float(x) for x in scw.matrix().ravel()]
