"""GPU: the loop-closing chain of tests/test_loop_correct_gpu.py with the map points' pose correction, which that test leaves out: on
the scenes `closed` and `fixed_scale` of tests/loop_scene.py, after the device chain, correct_loop_map (orbr_correct_loop) runs on the
scene's own table - every keyframe a slot in id order, every keypoint whose table entry is a map point an observation - with the
current keyframe's neighbours that are not bad and the current keyframe as queries.

Its corrected / non_corrected entries equal what test_loop_correct_gpu.corrected_sim3 and problem derive for the same keyframes,
within that test's float-rounding allowance, one float ulp of max(1, |x|) per entry of the 4x4 [s R | t].  The two differ by float
roundings only: the chain's Scw is a product with a float pose, so its rotation block is orthonormal to float rounding and no
further, and Quaterniond(R) -> toRotationMatrix (here) returns that block only to that accuracy, where corrected_sim3 multiplies
the block itself (measured on one MI355X: 0.62 ulp on `closed`, 0.70 ulp on `fixed_scale` at the worst entry); and Tic differs by
one float ulp wherever one of its double sums lies on a float rounding boundary (numpy's product does not sum left to right).  The corrected
points then go into optimize_essential_graph as a NON-EMPTY point table with corrected_ref (src/Optimizer.cc:1025-1034), and the result
equals essential_ref.optimize on the same inputs under the 64 x S rule of that file; the points' floats within 1 ulp + 64 x S with S their own spread over the same draws."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_ref as R        # noqa: E402
import loop_chain as LC          # noqa: E402
import loop_scene as LS          # noqa: E402
from test_loop_chain_gpu import gpu_chain                                    # noqa: E402
from test_loop_correct_gpu import corrected_sim3, problem, sim3_record       # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def scene_table(pkg, sc):
    """the scene's map as the observation table: slot = position of the keyframe's id in ascending order"""
    ids = sorted(sc["kfs"])
    slot = {k: i for i, k in enumerate(ids)}
    m = sc["map"]
    kf = np.zeros(len(ids), pkg.COVIS_KEYFRAME_DTYPE)
    rows, first = [], {}
    for k in ids:
        rec = sc["kfs"][k]
        T = rec["Tcw"]
        kf["id"][slot[k]], kf["bad"][slot[k]] = k, rec["bad"]
        kf["Ow"][slot[k]] = (-(T[:3, :3].T.astype(f64) @ T[:3, 3].astype(f64))).astype(f32)
        seen = set()
        for i, p in enumerate(rec["mp"]):
            p = int(p)
            if p < 0 or p in seen:
                continue
            seen.add(p)
            rows.append((p, slot[k], i, int(rec["k"]["octave"][i]), 0))
            first.setdefault(p, slot[k])
    pts = np.zeros(len(m["pos"]), pkg.COVIS_POINT_DTYPE)
    pts["pos"], pts["bad"] = m["pos"], m["bad"]
    pts["ref_kf"] = [first.get(p, -1) for p in range(len(pts))]
    return ids, slot, pkg.covis_table(kf, pts, rows, LS.SF)


def matrix(rec):
    """a Sim3 record as the 4x4 [s R | t]"""
    M = np.eye(4)
    M[:3, :3] = rec["s"] * R.quat_to_R(np.array(rec["q"], f64)[None])[0]
    M[:3, 3] = rec["t"]
    return M


@pytest.mark.parametrize("name", ["closed", "fixed_scale"])
def test_points_corrected_and_optimised_after_the_chain(pkg, name):
    sc = LS.scene(name)
    res = LC.closed(gpu_chain(name).result)
    assert res is not None
    cid, fix = res["kf"], sc["fix_scale"]
    ids, slot, table = scene_table(pkg, sc)
    conn = sorted([k for k in sc["kfs"][cid]["conn"] if not sc["kfs"][k]["bad"]] + [cid])
    feats = []
    for k in conn:
        f = np.zeros(len(sc["kfs"][k]["mp"]), pkg.COVIS_FEATURE_DTYPE)
        f["point"], f["octave"] = sc["kfs"][k]["mp"], sc["kfs"][k]["k"]["octave"]
        feats.append(f)
    queries = pkg.covis_queries([slot[k] for k in conn], feats)
    Scw = np.zeros(1, pkg.MAPCORRECT_SIM3_DTYPE)
    Scw["q"][0], Scw["t"][0], Scw["s"][0] = sim3_record(res["Scw"], fix)
    got = pkg.correct_loop_map(table, queries, slot[cid], np.stack([sc["kfs"][k]["Tcw"] for k in conn]), Scw[0])

    # the two Sim3 maps against test_loop_correct_gpu's own derivation
    want = corrected_sim3(sc, cid, res["Scw"])
    assert sorted(want) == conn
    vertex, vt, edges, _ = problem(pkg, sc, res)
    worst = 0.0
    for q, k in enumerate(conn):
        W = np.array(want[k], f64)      # with fixed scale its rotation block has s = 1 as the solver left it
        ulp = np.spacing(np.maximum(f32(1), np.abs(W)).astype(f32)).astype(f64)
        d = np.abs(matrix(got["corrected"][q]) - W)
        worst = max(worst, float((d / ulp).max()))
        assert (d <= ulp).all(), (k, d.max())
        snc = vt[vertex[k]]["Snc"]
        for key in ("q", "t", "s"):
            assert (np.abs(np.asarray(got["non_corrected"][key][q]) - np.asarray(snc[key])) <= np.spacing(f32(1))).all(), (k, key)
    print("%s: corrected Sim3 of %d keyframes off test_loop_correct_gpu's by at most %.3e float ulp" % (name, len(conn), worst))
    moved = np.nonzero(got["corrected_ref"] >= 0)[0]
    assert len(moved) >= 40 and (got["normals"]["status"][moved] == 0).all()
    assert set(got["corrected_ref"][moved]) <= {slot[k] for k in conn}

    # the essential graph with the corrected points: ref = the vertex of mnCorrectedReference, or of the reference keyframe
    pts = []
    for p in range(len(table["pts"])):
        if table["pts"]["bad"][p]:
            continue
        r = got["corrected_ref"][p] if got["corrected_ref"][p] >= 0 else table["pts"]["ref_kf"][p]
        if r >= 0 and ids[r] in vertex:
            pts.append((got["pos"][p][0], got["pos"][p][1], got["pos"][p][2], vertex[ids[r]]))
    points = np.array(pts, pkg.EG_POINT_DTYPE)
    assert len(points) > len(moved) > 0
    T, Po, est, info = pkg.optimize_essential_graph(vt, edges, points, fix)
    ref = R.optimize(vt, edges, points, fix)
    rng = np.random.default_rng(78)
    draws = [R.optimize(vt, edges, points, fix, order=rng, perturb=rng) for _ in range(16)]
    dev = max(float(np.abs(d["est"] - ref["est"]).max()) for d in draws)
    diff = float(np.abs(est - ref["est"]).max())
    print("%s: %d points (%d corrected); S = %.3e, kernels - restatement = %.3e" % (name, len(points), len(moved), dev, diff))
    assert info["free_vertices"] == ref["info"]["free_vertices"] and info["blocks"] == ref["info"]["blocks"]
    assert diff <= 64 * dev, (diff, dev)
    ulp = np.spacing(np.maximum(f32(1), np.abs(ref["Tcw"])).astype(f32)).astype(f64)
    assert (np.abs(T.astype(f64) - ref["Tcw"].astype(f64)) <= ulp + 64 * dev).all()
    pulp = np.spacing(np.maximum(f32(1), np.abs(ref["pts"])).astype(f32)).astype(f64)
    pdev = max(float(np.abs(d["pts"].astype(f64) - ref["pts"].astype(f64)).max()) for d in draws)      # S of the points themselves: an estimate's spread times |P|
    assert (np.abs(Po.astype(f64) - ref["pts"].astype(f64)) <= pulp + 64 * pdev).all(), pdev
