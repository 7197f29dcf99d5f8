"""GPU: the host classes of the local map (orb_slam2v2-1_amd/host/Tracking.h: LocalMapHIP, Tracking::UpdateLocalMap,
Tracking::SearchLocalPoints) through tests/cpp/localmap_driver.cc on shim objects built from a scene blob.  The lists, the
mnTrackReferenceForFrame marks, the reference keyframe and the NULLed slots equal the restatement tests/localmap_ref.py; and
Tracking::SearchLocalPoints leaves the frame and the points as the reference's first loop + SearchLocalPointsHIP leave a copy of them."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_ref as LR        # noqa: E402
import localmap_scene as S       # noqa: E402
from test_localmap_cpu import scene_blob      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "localmap_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "localmap_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def run(driver, tmp_path, blob):
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run([driver, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = {}
    for ln in out.stdout.strip().split("\n"):
        w = ln.split()
        lines[w[0]] = [int(x) for x in w[1:]]
    return lines


def check_lists(got, sc, want):
    i = want["info"]
    assert got["info"] == [i["empty_vote"], i["n_voted"], i["ref_kf"], i["extension_end"]]
    assert got["kf"] == list(want["local_kf"]) and got["pts"] == list(want["local_pts"])
    assert got["frame"] == list(want["frame_points"])
    assert got["kfmarks"] == ([] if i["empty_vote"] else sorted(int(k) for k in want["local_kf"]))     # the early return marks no keyframe
    assert got["ptmarks"] == sorted(int(p) for p in want["local_pts"])
    assert got["ref"] == [i["ref_kf"], i["ref_kf"]]


@pytest.mark.parametrize("name", ["plain", "bad_frame_point", "all_voted_bad", "empty_vote", "length_80_runs", "children_70_last_free", "parent_bad_is_added",
                                  "parent_ends_the_loop", "feature_counts_0_1_63_64_65_1025", "m_0", "frame_point_is_valid_0", "random"])
def test_update_local_map_class(driver, tmp_path, name):
    sc = S.scene(name)
    got = run(driver, tmp_path, scene_blob(sc) + np.array([0], np.int32).tobytes())
    check_lists(got, sc, S.expected(name))


@pytest.mark.parametrize("sensor,frame_id,last_reloc", [(0, 40, 0), (2, 40, 0), (0, 40, 39)], ids=["th1", "th3_rgbd", "th5_relocalised"])
def test_search_local_points_class(pkg, oracle, synth, driver, tmp_path, sensor, frame_id, last_reloc):
    from test_localmap_gpu import frame_scene
    sc, fr = frame_scene(pkg, oracle, synth)
    g = pkg.grid_geom(fr["w"], fr["h"])
    cam = np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"], np.float32(fr["mbf"]) / np.float32(fr["fx"]), g.min_x, g.min_y, g.max_x, g.max_y, fr["log_sf"]],
                   np.float32)
    blob = scene_blob(sc) + np.array([1], np.int32).tobytes() + cam.tobytes() + np.ascontiguousarray(fr["T"], np.float32).tobytes() + \
        np.array([sensor, frame_id, last_reloc], np.int32).tobytes() + np.ascontiguousarray(fr["k"], pkg.KP_DTYPE).tobytes() + \
        np.ascontiguousarray(fr["d"], np.uint8).tobytes() + fr["uright"].tobytes()
    got = run(driver, tmp_path, blob)
    want = LR.update_local_map(sc)
    check_lists(got, sc, want)
    nA, tA, nB, tB, same = got["search"]
    assert same == 1 and (nA, tA) == (nB, tB) and nA > 100 and tA >= nA
    # a match fills a free slot, or takes one whose point has no observation (which may be the very point it held)
    changed = [i for i, (a, b) in enumerate(zip(got["frame"], got["frame2"])) if a != b]
    assert 100 < len(changed) <= nA and all(got["frame2"][i] in want["local_pts"] for i in changed)
