"""GPU: the loop-closing chain of tests/test_loop_chain_gpu.py carried one step further, on the scenes `closed` (free scale) and
`fixed_scale` of tests/loop_scene.py: the Sim3 the chain's refine stage (row a28) produced for the keyframe that closed the loop is
propagated to that keyframe's neighbours on the host as LoopClosing::CorrectLoop does (src/LoopClosing.cc:430-470: Sic = Tiw * Twc in
float, CorrectedSiw = Sic * Scw, NonCorrectedSiw = Sim3(Riw, tiw, 1)), and the essential graph is optimised
(orbg_optimize_essential_graph): one vertex per keyframe that is not bad, the matched keyframe fixed, the current side's spanning tree
(each keyframe's parent is the one before it), the matched keyframe's tree edges to its neighbours, and the loop connections from the
current keyframe to the matched keyframe and its neighbours.

In these scenes every current-side keyframe is a neighbour of the current one, so every one carries a CorrectedSim3 and the graph
starts next to its optimum (the residual is the float rounding of Tic); what the test shows is that the chain's output is a valid
input, that the corrected current keyframe lands nearer the scene's true pose than it started (it started in the drifted frame), and
that the step equals the restatement fed the same inputs: the double estimates within 64 x S (S: the restatement's spread over 16
draws), the float poses within 1 ulp + 64 x S."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_ref as R        # noqa: E402
import loop_chain as LC          # noqa: E402
import loop_scene as LS          # noqa: E402
from test_loop_chain_gpu import gpu_chain      # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def sim3_record(M, fix_scale=False):
    """a 4x4 [s R | t] -> (q, t, s) as Sim3(R, t, s) holds it; with fixed scale s is 1 as the solver left it"""
    M = np.asarray(M, f64)
    s = 1.0 if fix_scale else float(np.sqrt((M[0, :3] * M[0, :3]).sum()))
    return R.quat_from_R((M[:3, :3] / s)[None])[0], M[:3, 3].copy(), s


def corrected_sim3(sc, cid, Scw):
    """LoopClosing::CorrectLoop :430-470, as tests/loop_chain.py's correct_loop restates it"""
    Tcw = sc["kfs"][cid]["Tcw"]
    Rwc = Tcw[:3, :3].T.copy()
    Ow = (-(Rwc.astype(f64) @ Tcw[:3, 3].astype(f64))).astype(f32)
    Twc = np.eye(4, dtype=f32)
    Twc[:3, :3], Twc[:3, 3] = Rwc, Ow
    corrected = {cid: np.asarray(Scw, f64)}
    for k in sc["kfs"][cid]["conn"]:
        if sc["kfs"][k]["bad"]:
            continue
        Tic = (sc["kfs"][k]["Tcw"].astype(f64) @ Twc.astype(f64)).astype(f32)
        Sic = np.eye(4)
        Sic[:3, :3], Sic[:3, 3] = Tic[:3, :3].astype(f64), Tic[:3, 3].astype(f64)
        corrected[k] = Sic @ corrected[cid]
    return corrected


def problem(pkg, sc, res):
    cid, mid = res["kf"], res["winner_kf"]
    corrected = corrected_sim3(sc, cid, res["Scw"])
    ids = [k for k in sorted(sc["kfs"]) if k <= cid and not sc["kfs"][k]["bad"]]
    vertex = {k: i for i, k in enumerate(ids)}
    vt = np.zeros(len(ids), pkg.EG_VERTEX_DTYPE)
    for k in ids:
        v = vt[vertex[k]]
        T = np.eye(4)
        T[:3, :] = sc["kfs"][k]["Tcw"].astype(f64)[:3, :]
        q, t, s = sim3_record(T)
        v["Snc"]["q"], v["Snc"]["t"], v["Snc"]["s"] = q, t, 1.0
        if k in corrected:
            q, t, s = sim3_record(corrected[k], sc["fix_scale"])
            v["has_nc"] = 1
        v["Scw"]["q"], v["Scw"]["t"], v["Scw"]["s"] = q, t, (s if k in corrected else 1.0)
        v["fixed"] = int(k == mid)
    near = [k for k in sc["kfs"][mid]["conn"] if k in vertex]
    edges = [(vertex[cid], vertex[j], 0) for j in sorted([mid] + near)]                   # the loop connections
    cur_side = [k for k in ids if k >= 10]
    edges += [(vertex[b], vertex[a], 1) for a, b in zip(cur_side[:-1], cur_side[1:])]     # the current side's spanning tree
    edges += [(vertex[j], vertex[mid], 1) for j in near]                                  # the matched keyframe's
    return vertex, vt, np.array(edges, pkg.EG_EDGE_DTYPE), np.zeros(0, pkg.EG_POINT_DTYPE)


@pytest.mark.parametrize("name", ["closed", "fixed_scale"])
def test_essential_graph_after_the_chain(pkg, name):
    sc = LS.scene(name)
    res = LC.closed(gpu_chain(name).result)
    assert res is not None
    cid = res["kf"]
    vertex, vt, edges, points = problem(pkg, sc, res)
    fix = sc["fix_scale"]
    T, _, est, info = pkg.optimize_essential_graph(vt, edges, points, fix)
    ref = R.optimize(vt, edges, points, fix)
    rng = np.random.default_rng(77)
    draws = [R.optimize(vt, edges, points, fix, order=rng, perturb=rng) for _ in range(16)]
    dev = max(float(np.abs(d["est"] - ref["est"]).max()) for d in draws)
    diff = float(np.abs(est - ref["est"]).max())
    print("%s: closed by %d on %d; S = %.3e, kernels - restatement = %.3e; iterations %d / %d, end %d / %d, chi2 %.3e -> %.3e" % (
        name, cid, res["winner_kf"], dev, diff, info["iterations"], ref["info"]["iterations"], info["end"], ref["info"]["end"],
        info["chi2_first"], info["chi2_last"]))
    assert info["free_vertices"] == ref["info"]["free_vertices"] and info["blocks"] == ref["info"]["blocks"]
    assert diff <= 64 * dev, (diff, dev)
    ulp = np.spacing(np.maximum(f32(1), np.abs(ref["Tcw"])).astype(f32)).astype(f64)
    assert (np.abs(T.astype(f64) - ref["Tcw"].astype(f64)) <= ulp + 64 * dev).all()
    # the corrected current keyframe against the scene's true pose [R_i | t_i] = Scw_true / scale, by its camera centre and rotation
    St = sc["Scw_true"][cid]
    Rt, tt = St[:3, :3] / sc["scale"], St[:3, 3] / sc["scale"]
    centre = lambda Rm, t: -Rm.T @ t      # noqa: E731
    T0, T1 = sc["kfs"][cid]["Tcw"].astype(f64), T[vertex[cid]].astype(f64)
    before = np.linalg.norm(centre(T0[:3, :3], T0[:3, 3]) - centre(Rt, tt))
    after = np.linalg.norm(centre(T1[:3, :3], T1[:3, 3]) - centre(Rt, tt))
    print("%s: camera centre of keyframe %d off the truth by %.4f before, %.4f after" % (name, cid, before, after))
    assert after < before
    assert np.abs(T1[:3, :3] - Rt).max() < np.abs(T0[:3, :3] - Rt).max()
    if fix:
        assert (est[:, 7] == 1.0).all()
