"""GPU: ORB_SLAM2::Initializer (orb_slam2v2-1_amd/host/Initializer.h) through tests/cpp/initializer_driver.cc on two shim Frames built
from a scene file: the return value, R21, t21, vP3D and vbTriangulated in keypoint-1 indexing equal the restatement fed the sets the
driver drew with rand(); a second Initialize in the same process draws other sets and agrees with its restatement too."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_ref as R        # noqa: E402
import init_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "initializer_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "initializer_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def hx(x):
    return float(x).hex()


@pytest.mark.parametrize("name", ["unmatched_keys", "rotation_100"])
def test_initializer_class_on_shim_frames(driver, tmp_path, name):
    sc = S.case(name)
    n1, n2, N, it = len(sc["keys1"]), len(sc["keys2"]), len(sc["matches"]), 48
    m12 = np.full(n1, -1, np.int64)
    m12[sc["matches"][:, 0]] = sc["matches"][:, 1]
    lines = [" ".join(hx(np.float32(k)) for k in sc["K4"]), str(it), str(n1)]
    lines += ["%s %s %d" % (hx(sc["keys1"][i, 0]), hx(sc["keys1"][i, 1]), m12[i]) for i in range(n1)]
    lines += [str(n2)] + ["%s %s" % (hx(k[0]), hx(k[1])) for k in sc["keys2"]]
    (tmp_path / "scene.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([driver, str(tmp_path / "scene.txt"), "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    calls, cur = [], None
    for ln in out.stdout.strip().split("\n"):
        key, vals = ln.split()[0], ln.split()[1:]
        if key == "ret":
            cur = {}
            calls.append(cur)
        cur[key] = vals
    assert len(calls) == 2
    sets = [np.array([int(x) for x in c["sets"]], np.int32).reshape(it, 8) for c in calls]
    assert (sets[0] != sets[1]).any()                              # rand() continues: the second call draws other sets
    for c, s in zip(calls, sets):
        assert s.min() >= 0 and s.max() < N and all(len(set(r)) == 8 for r in s.tolist())
        r = R.initialize(sc["keys1"], sc["keys2"], sc["matches"], s, sc["K4"])
        assert int(c["ret"][0]) == r["result"]
        if not r["result"]:
            assert c["untouched"] == ["1"]
            continue
        assert [float.fromhex(x) for x in c["R"]] == [float(x) for x in r["R21"].ravel()]
        assert [float.fromhex(x) for x in c["t"]] == [float(x) for x in r["t21"]]
        tri, P = np.zeros(n1, np.uint8), np.zeros((n1, 3), np.float32)      # scattered back to keypoint-1 indexing
        tri[sc["matches"][:, 0]], P[sc["matches"][:, 0]] = r["triangulated"], r["P3D"]
        assert [int(x) for x in c["tri"]] == tri.tolist() and len(c["P3D"]) == 3 * n1
        assert [float.fromhex(x) for x in c["P3D"]] == [float(x) for x in P.ravel()]
    if name == "rotation_100":
        assert [c["ret"] for c in calls] == [["0"], ["0"]]
