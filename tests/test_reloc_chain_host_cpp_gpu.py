"""GPU: the host classes Tracking::Relocalization strings together (orb_slam2v2-1_amd/host: KeyFrameDatabaseHIP, Frame / KeyFrame::ComputeBoW,
ORBmatcher::SearchByBoW, PnPsolver, Optimizer::PoseOptimization, ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th,
ORBdist)) through tests/cpp/reloc_driver.cc, a command interpreter over shim Frame / KeyFrame / MapPoint objects built from a scene
of tests/reloc_scene.py.  The driver holds no control flow of the loop: this test sends it the command sequence of the CPU chain
(tests/reloc_chain.py: Chain.script) and compares the state every command prints - candidate ids, matches per frame keypoint,
mvKeyPointIndices, pose bits, vbInliers, mvbOutlier, mvpMapPoints, nGood, nadditional - with what the device chain of the Python
backend had at that point.  Equal results at every command imply the same control flow.  What is under test is the seam code of
the classes: PoseOptimization reading mTcw and writing mvbOutlier / SetPose, SearchByProjection projecting from mTcw itself,
the solver's index table, the frame's state carried from command to command."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_scene            # noqa: E402
import reloc_chain as RC    # noqa: E402
import reloc_scene as RS    # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")
LINES = {"detect": 1, "bow": 1, "solver": 1, "iterate": 1, "adopt": 3, "optimize": 3, "drop_outliers": 1, "project": 2, "refound": 1}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "reloc_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "reloc_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def hx(x):
    return float(x).hex()


def ints(a):
    return " ".join(str(int(v)) for v in a)


def scene_file(path, sc):
    m, q = sc["map"], sc["query"]
    lines = [" ".join(hx(np.float32(c)) for c in RS.CAM), "%d %d" % (RS.W, RS.H), "%d %s" % (RS.NLEVELS, hx(RS.LOG_SF))]
    lines += ["%s %s %s" % (hx(RS.SF[l]), hx(RS.LEVEL_SIGMA2[l]), hx(RS.INV_LEVEL_SIGMA2[l])) for l in range(RS.NLEVELS)]
    lines.append(str(len(m["pos"])))
    for j in range(len(m["pos"])):
        lines.append("%s %s %s %d %s" % (" ".join(hx(v) for v in m["pos"][j]), hx(m["maxd"][j]), hx(m["mind"][j]), int(m["bad"][j]), ints(m["desc"][j])))
    lines.append(str(len(sc["kfs"])))
    for kf in sc["kfs"]:
        lines.append("%d %d %d" % (kf["id"], int(kf["bad"]), len(kf["k"])))
        for k, mp, d in zip(kf["k"], kf["mp"], kf["d"]):
            lines.append("%s %s %d %s %d %s" % (hx(k["x"]), hx(k["y"]), k["octave"], hx(k["angle"]), mp, ints(d)))
    lines.append(str(len(q["k"])))
    for k, d in zip(q["k"], q["d"]):
        lines.append("%s %s %d %s %s" % (hx(k["x"]), hx(k["y"]), k["octave"], hx(k["angle"]), ints(d)))
    path.write_text("\n".join(lines) + "\n")


def same_pose(tokens, T):
    return [float.fromhex(x) for x in tokens] == [float(x) for x in np.asarray(T, np.float32).ravel()]


def check(cmd, out, want):
    """the lines one command printed against the state the device chain had after the same step"""
    op = cmd.split()[0]
    head = out[0].split()
    if op == "detect":
        assert [int(x) for x in head[1:]] == want["ids"], cmd
    elif op == "bow":
        assert int(head[1]) == want["n"] and [int(x) for x in head[2:]] == want["mp"].tolist(), cmd
    elif op == "solver":
        assert (int(head[1]), int(head[2])) == (want["min_inliers"], want["max_iterations"]) and [int(x) for x in head[4:]] == want["index"].tolist(), cmd
        assert int(head[3]) == len(want["index"])
    elif op == "iterate":
        assert (int(head[1]), int(head[2]), int(head[3])) == (want["found"], want["no_more"], want["n"]), (cmd[:40], head, want["found"], want["no_more"], want["n"])
        if want["found"]:
            assert out[1].split()[0] == "T" and same_pose(out[1].split()[1:], want["T"]), cmd[:40]
            assert out[2].split()[0] == "inl" and [int(x) for x in out[2].split()[1:]] == want["inl"].tolist(), cmd[:40]
    elif op == "adopt":
        assert same_pose(out[1].split()[1:], want["T"]) and [int(x) for x in out[2].split()[1:]] == want["mp"].tolist(), cmd
    elif op == "optimize":
        assert int(head[1]) == want["n"], (cmd, head, want["n"])
        assert same_pose(out[1].split()[1:], want["T"]) and [int(x) for x in out[2].split()[1:]] == [int(v != 0) for v in want["out"]], cmd
    elif op == "drop_outliers":
        assert head[0] == "mp" and [int(x) for x in head[1:]] == want["mp"].tolist(), cmd
    elif op == "project":
        assert int(head[1]) == want["n"] and [int(x) for x in out[1].split()[1:]] == want["mp"].tolist(), (cmd, head, want["n"])
    elif op == "refound":
        assert int(head[1]) == want["n"], cmd


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_host_classes_chained(driver, tmp_path, name):
    sc = RS.scene(name)
    cpu = RC.cpu_chain(name)
    gpu = RC.Chain(RC.GpuBackend(sc), sc)
    gpu.run()
    commands = [c for c, _ in cpu.script]
    assert commands == [c for c, _ in gpu.script], name              # the device chain took the CPU chain's steps
    voc, scene, script = tmp_path / "voc.txt", tmp_path / "scene.txt", tmp_path / "commands.txt"
    bow_scene.write_text(sc["voc"], str(voc))
    scene_file(scene, sc)
    script.write_text("\n".join(commands) + "\n")
    run = subprocess.run([driver, str(voc), str(scene), str(script)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr + run.stdout[-2000:]
    lines = run.stdout.strip().split("\n")
    at = 0
    for cmd, want in gpu.script:
        op = cmd.split()[0]
        n = LINES[op] + (2 if op == "iterate" and lines[at].split()[1] == "1" else 0)
        check(cmd, lines[at:at + n], want)
        at += n
    assert at == len(lines), (at, len(lines))
    print("%s: %d commands, every printed state equal to the device chain's" % (name, len(commands)))
