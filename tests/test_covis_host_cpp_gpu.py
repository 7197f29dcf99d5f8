"""GPU: the host classes of the covisibility calls (orb_slam2v2-1_amd/host/LocalMapping.h: LocalMapping::KeyFrameCulling;
Covisibility.h: UpdateConnectionsHIP, UpdateNormalAndDepthHIP) through tests/cpp/covis_driver.cc on shim objects built from the scenes
of tests/covis_scene.py.  The printed state equals the restatement tests/covis_ref.py: which keyframes are bad or to be erased and
which points are bad; every keyframe's ordered list with its weights and its weight map, the other side's included (AddConnection);
every point's normal and distances as hexadecimal floats."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_ref as R        # noqa: E402
import covis_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "covis_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "covis_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def hx(x):
    return float(x).hex()


def write_script(path, mode, table, queries, monocular=0):
    """every keyframe gets the features its observations imply (depth 10); a query keyframe gets the query's own features"""
    kf, pts, off, obs = table["kf"], table["pts"], table["obs_off"], table["obs"]
    K, P = len(kf), len(pts)
    feats = [dict() for _ in range(K)]
    owner = np.repeat(np.arange(P), np.diff(off))
    for o in range(len(obs)):
        feats[obs["kf"][o]][int(obs["idx"][o])] = (int(owner[o]), int(obs["octave"][o]), 10.0, int(obs["stereo"][o]))
    qk = [] if queries is None else [int(s) for s in queries["query_kf"]]
    for q, s in enumerate(qk):
        f = queries["feat"][queries["feat_off"][q]:queries["feat_off"][q + 1]]
        old = feats[s]
        feats[s] = {i: (int(f["point"][i]), int(f["octave"][i]), float(f["depth"][i]), old.get(i, (0, 0, 0, 0))[3]) for i in range(len(f))}
    lines = ["%s %d %d %d %d" % (mode, monocular, K, P, len(table["sf"])), " ".join(hx(x) for x in table["sf"])]
    for s in range(K):
        n = max(feats[s]) + 1 if feats[s] else 0
        lines.append("%d %d %s %s %d" % (kf["id"][s], kf["not_erase"][s], hx(kf["th_depth"][s]), " ".join(hx(x) for x in kf["Ow"][s]), n))
        for i in range(n):
            p, octv, d, st = feats[s].get(i, (-1, 0, -1.0, 0))
            lines.append("%d %d %s %d" % (p, octv, hx(d), st))
    for p in range(P):
        lines.append("%d %d %s" % (pts["bad"][p], pts["ref_kf"][p], " ".join(hx(x) for x in pts["pos"][p])))
    lines.append(str(len(obs)))
    for o in range(len(obs)):
        lines.append("%d %d %d" % (owner[o], obs["kf"][o], obs["idx"][o]))
    lines.append(str(len(qk)))
    lines.append(" ".join(str(s) for s in qk))
    path.write_text("\n".join(lines) + "\n")


def run(driver, path):
    out = subprocess.run([driver, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    return out.stdout.strip().split("\n")


@pytest.mark.parametrize("name", ["chain", "point_dies", "not_erase", "id0", "stereo_far", "stereo_far_monocular", "stereo_count", "stereo_keeps_point", "random"])
def test_keyframe_culling_class(driver, tmp_path, name):
    sc = S.CULLING_CASES[name]()
    write_script(tmp_path / "s.txt", "cull", sc["table"], sc["queries"], sc["monocular"])
    lines = run(driver, tmp_path / "s.txt")
    _, _, v, pb = S.expected_culling(sc)
    K = len(sc["table"]["kf"])
    verdict = {int(s): int(x) for s, x in zip(sc["queries"]["query_kf"], v)}
    assert lines[:K] == ["kf %d %d %d" % (s, verdict.get(s, 0) == 1, verdict.get(s, 0) == 2) for s in range(K)]
    assert lines[K:] == ["pt %d %d" % (p, b) for p, b in enumerate(pb)]


def expected_connection_state(sc):
    """UpdateConnections of the queries one after the other, with AddConnection / UpdateBestCovisibles on the other side
    (src/KeyFrame.cc:123-161), slots standing for pointers"""
    K = len(sc["table"]["kf"])
    wmap, order = [dict() for _ in range(K)], [[] for _ in range(K)]
    for s, (ids, ws, counter) in zip(sc["queries"]["query_kf"], R.update_connections(sc["table"], sc["queries"], 15)):
        if not ids:
            continue
        for k, w in zip(ids, ws):
            if wmap[k].get(int(s)) != w:
                wmap[k][int(s)] = w
                order[k] = [(kk, ww) for ww, kk in sorted(((ww, kk) for kk, ww in wmap[k].items()), reverse=True)]
        wmap[s] = dict(counter)
        order[s] = list(zip(ids, ws))
    return wmap, order


@pytest.mark.parametrize("name", ["plain", "ties", "below_threshold", "empty", "duplicate_point", "bad_points", "Q40"])
def test_update_connections_class(driver, tmp_path, name):
    sc = S.CONNECTION_CASES[name]()
    write_script(tmp_path / "s.txt", "conn", sc["table"], sc["queries"])
    lines = run(driver, tmp_path / "s.txt")
    wmap, order = expected_connection_state(sc)
    want = []
    for s in range(len(sc["table"]["kf"])):
        want.append(("ord %d " % s + " ".join("%d:%d" % kw for kw in order[s])).rstrip())
        want.append(("map %d " % s + " ".join("%d:%d" % (k, wmap[s][k]) for k in sorted(wmap[s]))).rstrip())
    assert [ln.rstrip() for ln in lines] == want
    assert any(order[s] for s in range(len(order)) if s not in set(int(x) for x in sc["queries"]["query_kf"])) or name == "empty"   # the other side was written


@pytest.mark.parametrize("name", list(S.NORMAL_CASES))
def test_update_normal_and_depth_class(driver, tmp_path, name):
    t = S.NORMAL_CASES[name]()["table"]
    write_script(tmp_path / "s.txt", "normals", t, None)
    lines = run(driver, tmp_path / "s.txt")
    ref = R.update_normal_and_depth(t)
    got = [ln.split() for ln in lines]
    assert len(got) == len(ref)
    for p, g in enumerate(got):
        assert g[0] == "n" and int(g[1]) == p
        vals = np.array([float.fromhex(x) for x in g[2:]], np.float32)
        want = np.array(list(ref["normal"][p]) + [ref["max_distance"][p], ref["min_distance"][p]], np.float32)
        assert vals.tobytes() == want.tobytes(), p
