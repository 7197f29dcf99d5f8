"""CPU: the restatement of PnPsolver (tests/pnp_ref.py) against ground truth - the five OpenCV calls of EPnP are this project's own
Jacobi routines, so the reference the GPU tests compare with is itself checked here: it recovers the pose of seeded scenes, its
eigen- and singular values are LAPACK's, and its bookkeeping answers as a transcription of the reference's iterate / Refine that
refines at EVERY qualifying iteration.  Then the kernels' text compiled for the host (tests/cpp/pnp_lockstep.cc) against it byte
for byte, also under AddressSanitizer and UBSan, and the C ABI's host-side parts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ref as R        # noqa: E402
import pnp_scene as S      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)


def pose_errors(T, Tt):
    """(Frobenius norm of R - R_true, |t - t_true| / |t_true|)"""
    T = np.asarray(T, np.float64)
    return float(np.linalg.norm(T[:3, :3] - Tt[:3, :3])), float(np.linalg.norm(T[:3, 3] - Tt[:3, 3]) / np.linalg.norm(Tt[:3, 3]))


def test_exact_scene_every_hypothesis_that_fits_its_set_counts_all():
    """exact_40: no noise, no outliers.  EPnP on FOUR points has a four-dimensional null space and three Gauss-Newton starts; it does
    not always reach the pose, and says so itself: a hypothesis is non-degenerate when the mean reprojection error over its own
    four points (rep_errors[N]) is below 0.1 px.  Every such hypothesis counts 40 (7 of the 12 here; one more counts 40 at
    0.68 px), and the refinement over all 40 counts 40."""
    sc, r = S.case("exact_40"), S.reference("exact_40")
    good = r["rep"] < 0.1
    assert good.sum() >= 6 and (r["counts"][good] == 40).all()
    assert r["hit_iteration"] == 0 and r["refined_inliers"] == 40 and r["inliers"].all() and r["pose"] == R.POSE_REFINED


MEASURED = {"exact_40": (3.2e-8, 2.1e-8), "hit_60": (3.5e-3, 8.2e-3)}


@pytest.mark.parametrize("name", ["exact_40", "hit_60"])
def test_restatement_recovers_the_pose(name):
    """The refined pose against the scene's true pose.  No bound can be derived for it, so it was measured (MEASURED: Frobenius norm
    of R - R_true, relative translation error; DESIGN.md section 6 has the same figures) and 10 x the measurement is asserted: a later
    change of operation order that costs digits shows.  exact_40 is at the float32 narrowing of Tcw."""
    sc, r = S.case(name), S.reference(name)
    assert r["pose"] == R.POSE_REFINED
    rot, tra = pose_errors(r["Tcw"], sc["Tcw_true"])
    print("%s: |R - R_true| = %.3g, |t - t_true| / |t_true| = %.3g" % (name, rot, tra))
    assert rot <= 10 * MEASURED[name][0] and tra <= 10 * MEASURED[name][1]


def test_hit_scene_keeps_every_clear_inlier():
    """hit_60: the returned inlier set contains every constructed inlier whose reprojection error under the TRUE pose is below half
    its threshold, and no gross outlier"""
    sc, r = S.case("hit_60"), S.reference("hit_60")
    c = sc["corrs"]
    uv = S.project(sc["Tcw_true"], c["w"].astype(np.float64))
    e2 = (uv[:, 0] - c["u"]) ** 2 + (uv[:, 1] - c["v"]) ** 2
    clear = ~sc["outlier"] & (e2 < 0.5 * c["sigma2"] * sc["th2"])
    assert clear.sum() >= 35 and r["inliers"][clear].all() and not r["inliers"][sc["outlier"]].any()


def test_scenes_take_the_paths_they_are_for():
    r = S.reference("n_4")          # min_inliers == N: one iteration in the plan, iterate(5) runs 5; 4 is never > 4
    assert (S.case("n_4")["min_inliers"], S.case("n_4")["max_iterations"]) == (4, 1)
    assert r["iterations_run"] == 5 and r["hit_iteration"] == -1 and r["no_more"] == 1 and r["pose"] == R.POSE_BEST and r["best_inliers"] == 4
    r = S.reference("n_9")          # below min_inliers 10: nothing runs
    assert (r["iterations"], r["no_more"], r["pose"], r["iterations_run"]) == (0, 1, R.POSE_NONE, 0)
    assert [len(S.case(k)["corrs"]) for k in ("wave_63", "wave_64", "wave_65", "n_257", "n_1100")] == [63, 64, 65, 257, 1100]
    for k in ("wave_63", "wave_64", "wave_65"):
        assert S.reference(k)["hit_iteration"] > 0
    assert S.reference("n_257")["refined_inliers"] > 256 and S.reference("n_257")["best_inliers"] > 256
    r = S.reference("n_1100")       # the refinement gathers more than 1024 points
    assert r["hit_iteration"] > 0 and r["best_inliers"] > 900 and r["refined_inliers"] > 1024 - 64
    r = S.reference("exhausted_60")  # qualifying iterations, refinements that count 30 and never more: the best pose, no_more
    assert r["hit_iteration"] == -1 and r["no_more"] == 1 and r["pose"] == R.POSE_BEST and r["best_inliers"] == 30 == S.case("exhausted_60")["min_inliers"]
    assert (r["rcounts"][r["rcounts"] >= 0] == 30).all() and (r["counts"] == 30).sum() > 1 and r["best_iteration"] == int(np.argmax(r["counts"] == 30))
    r = S.reference("refine_fails_then_hits")
    assert r["counts"][1] == 20 and r["rcounts"][1] == 20 and r["counts"][3] == 40 and r["rcounts"][3] == 40 and r["hit_iteration"] == 3
    assert (r["rcounts"][[0, 2, 4, 5, 6]] == -1).all()
    sc, r, r1 = S.case("two_calls"), S.reference("two_calls"), S.reference("hit_60")
    h = r["hit_iteration"]          # a qualifying iteration that is no record returns the prior set's refinement again
    assert h > 0 and sc["min_inliers"] <= r["counts"][h] <= sc["prior_best_inliers"] and r["best_iteration"] == -1
    assert (r["rcounts"][:-1] == -1).all() and r["rcounts"][-1] == r["refined_inliers"] == r1["refined_inliers"]
    assert S.same(r["Tcw"], r1["Tcw"]) and (r["inliers"] == r1["inliers"]).all() and (r["best_flags"] == r1["best_flags"]).all()
    r = S.reference("planar")       # PCA: the smallest eigenvalue is about 0, a control point collapses, CC is singular: the
    rc = r["rcounts"][r["rcounts"] >= 0]   # pseudo-inverse leaves a column out and the refinement is poor - nothing spins, nothing is NaN
    assert len(rc) >= 1 and np.isfinite(r["rmodels"]).all() and np.isfinite(r["models"]).all()
    w = S.case("planar")["corrs"]["w"].astype(np.float64)
    assert np.linalg.eigvalsh(np.cov(w.T))[0] < 1e-12
    r, sc = S.reference("behind"), S.case("behind")
    assert r["hit_iteration"] >= 0 and not r["inliers"][[5, 6]].any()
    r = S.reference("duplicate")    # set 0 names two identical points: a model all the same, few inliers, the call ends
    assert r["counts"][0] < 4 and r["iterations_run"] == 6


@pytest.mark.parametrize("name", list(S.CASES))
def test_conditions_of_the_byte_comparison(name):
    S.assert_conditions(name)


def test_jacobi_eig12_against_lapack():
    """50 seeded symmetric positive semi-definite 12x12, 25 of them of rank 8 (MtM of four points).  Eigenvalues: measured 1.1e-15 of
    the largest, asserted 10 x.  The null space is compared as a subspace, by projector difference (measured 7.9e-15, asserted
    10 x), never vector by vector: any basis of it is an answer."""
    rng = np.random.default_rng(12)
    for k in range(50):
        G = rng.normal(size=(8 if k < 25 else 30, 12))
        A = G.T @ G
        A = (A + A.T) / 2
        d, ut = R.eig_sym(A.tolist())
        ref = np.linalg.eigvalsh(A)[::-1]
        assert np.abs(np.array(d) - np.abs(ref)).max() <= 1.1e-14 * ref.max()
        assert all(d[i] >= d[i + 1] for i in range(11))
        U = np.array(ut)
        assert np.abs(U @ U.T - np.eye(12)).max() < 1e-13
        if k < 25:
            P = U[8:].T @ U[8:]
            Q = np.linalg.eigh(A)[1][:, :4]
            assert np.abs(P - Q @ Q.T).max() <= 7.9e-14
    d, ut = R.eig_sym(np.zeros((12, 12)).tolist())         # a zero matrix rotates nothing; a NaN cannot spin
    assert not any(d) and ut == np.eye(12).tolist()
    d, _ = R.eig_sym(np.full((3, 3), np.nan).tolist())
    assert all(x != x for x in d)


def test_double_svd_solves_against_lapack():
    """50 seeded 6 x k systems, k = 4, 3, 5 in turn, as the three beta approximations: solution measured 4.2e-15 relative,
    singular values 7.3e-16 of the largest; 10 x asserted.  A rank-deficient system: the column below 2 DBL_EPSILON sum(w) is left
    out and the minimum-norm solution results.  The 3x3 decomposition: U diag(w) V^T = A, det-sign free, w descending."""
    rng = np.random.default_rng(12)
    for k in range(50):
        m = (4, 3, 5)[k % 3]
        A, b = rng.normal(size=(6, m)), rng.normal(size=6)
        x = np.array(R.svd_solve(A.tolist(), b.tolist()))
        xr = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.abs(x - xr).max() <= 4.2e-14 * np.abs(xr).max()
        _, w, _ = R.jacobi_svd_d(A.tolist())
        sv = np.linalg.svd(A, compute_uv=False)
        assert np.abs(np.sort(w)[::-1] - sv).max() <= 7.3e-15 * sv.max()
    A = rng.normal(size=(6, 4))
    A[:, 3] = A[:, 0] + A[:, 1]
    b = rng.normal(size=6)
    x = np.array(R.svd_solve(A.tolist(), b.tolist()))
    assert np.abs(x - np.linalg.pinv(A) @ b).max() < 1e-12
    for k in range(10):
        A = rng.normal(size=(3, 3))
        U, V, w = R.svd3_d(A.tolist())
        U, V = np.array(U), np.array(V)
        assert np.abs(U * np.array(w) @ V.T - A).max() < 1e-14 and w[0] >= w[1] >= w[2]
        inv = np.array(R.svd_invert3(A.tolist()))
        assert np.abs(inv @ A - np.eye(3)).max() < 1e-10
    x = [7.0] * 4                                         # qr_solve on a zero matrix: the early return leaves x as it was
    R.qr_solve([0.0] * 24, [1.0] * 6, x)
    assert x == [7.0] * 4


def test_pnp_parameters_table(pkg):
    """src/PnPsolver.cc:121-157 by hand, Relocalization's (0.99, 10, 300, 4, 0.5f, 5.991f).  n 100: int(50.0) = 50, epsilon 0.5,
    log(0.01) / log(1 - 0.125) = -4.60517 / -0.133531 = 34.49 -> 35.  n 10: int(5.0) = 5 -> 10 = n: one iteration.  n 60: 30, 35.
    n 16: 8 -> 10, epsilon 10/16 = 0.625, 0.625^3 = 0.244141, log(0.755859) = -0.279900, 16.45 -> 17.  n 0: min_inliers stays 10,
    epsilon 10 / 0 = inf and the logarithm of a negative number is NaN: kept in range as max_iterations (the reference's conversion
    is undefined); iterate answers bNoMore before it matters.  epsilon 0.3, min 20, n 60: int(18.0) = 18 -> 20, epsilon 1/3,
    log(26/27) = -0.0377403, 122.02 -> 123.  min_set 3: ORBX_ERR_ARG."""
    table = [((100, 0.99, 10, 300, 4, 0.5), (50, 35)), ((10, 0.99, 10, 300, 4, 0.5), (10, 1)), ((60, 0.99, 10, 300, 4, 0.5), (30, 35)),
             ((16, 0.99, 10, 300, 4, 0.5), (10, 17)), ((0, 0.99, 10, 300, 4, 0.5), (10, 300)), ((60, 0.99, 20, 300, 4, 0.3), (20, 123)),
             ((4, 0.99, 4, 300, 4, 0.5), (4, 1)), ((100, 0.99, 10, 20, 4, 0.5), (50, 20)), ((9, 0.99, 10, 300, 4, 0.5), (10, 300))]
    for args, want in table:
        assert R.pnp_parameters(*args) == want, args
        assert pkg.pnp_parameters(*args) == want, args
    with pytest.raises(pkg.OrbxError) as e:
        pkg.pnp_parameters(100, 0.99, 10, 300, 3, 0.5)
    assert e.value.status == pkg.ORBX_ERR_ARG
    a = __import__("ctypes").c_int(0)
    assert pkg.lib().orbp_pnp_parameters(10, 0.99, 10, 300, 4, 0.5, None, __import__("ctypes").byref(a)) == pkg.ORBX_ERR_ARG
    assert pkg.lib().orbp_pnp_parameters(-1, 0.99, 10, 300, 4, 0.5, __import__("ctypes").byref(a), __import__("ctypes").byref(a)) == pkg.ORBX_ERR_ARG


def test_records_only_replay_equals_refining_at_every_iteration():
    """k_pnp_select looks a refined count up only at records and at the prior slot; the reference refines mvbBestInliers at EVERY
    qualifying iteration.  200 random count sequences, each as two consecutive calls, with a synthetic refinement table (a refined
    count per SET, whoever asks): hit iteration, iterations run, no_more, what is returned and the carried state are the same."""
    rng = np.random.default_rng(3)
    for trial in range(200):
        mi = int(rng.integers(8, 30))
        max_its = int(rng.integers(1, 40))
        table = {}                                   # set key -> refined count; keys: (call, iteration)
        state = dict(done=0, best=0, best_key=None)
        done, prior_best, prior_key = 0, 0, None
        for callno in range(2):
            k = int(rng.integers(1, 45))
            its = max(max_its - done, k)
            lo = int(rng.integers(0, mi + 5))
            counts = rng.integers(0, lo + int(rng.integers(1, 25)), its)
            for it in range(its):                    # few refinements pass, so that sequences run on
                table[(callno, it)] = int(rng.integers(0, mi + 3)) if rng.random() < 0.8 else int(rng.integers(mi, mi + 30))
            rec = R.records(counts, mi, prior_best)
            rcounts = np.full(its + 1, -1)
            for s in rec:
                rcounts[s] = table[(callno, s)]
            if prior_best > 0:
                rcounts[its] = table[prior_key]
            o = R.replay(counts, rcounts, mi, max_its, done, prior_best)
            hit, run, no_more, ret_best = R.iterate_reference([int(c) for c in counts], lambda key: table[key if not isinstance(key, int) else (callno, key)],
                                                              mi, max_its, k, state)
            assert run <= its and (o["hit_iteration"], o["iterations_run"], o["no_more"]) == (hit, run, int(no_more)), (trial, callno)
            assert ret_best == (o["pose"] in (R.POSE_BEST, R.POSE_PRIOR_BEST)) and (hit >= 0) == (o["pose"] == R.POSE_REFINED)
            assert o["best_inliers"] == state["best"]
            if hit >= 0:
                key = state["best_key"] if not isinstance(state["best_key"], int) else (callno, state["best_key"])
                assert o["refined_inliers"] == table[key] and o["slot"] == (its if o["best_iteration"] < 0 else o["best_iteration"])
            if o["best_iteration"] >= 0:
                prior_key = (callno, o["best_iteration"])
                assert state["best_key"] == o["best_iteration"]
            if isinstance(state["best_key"], int):
                state["best_key"] = (callno, state["best_key"])
            done, prior_best = done + run, o["best_inliers"]
            assert done == state["done"]
            if no_more and hit < 0:
                break


def build_lockstep(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "csrc"), *extra, "-o", out, os.path.join(ROOT, "tests", "cpp", "pnp_lockstep.cc")])
    return out


@pytest.fixture(scope="module")
def lockstep(tmp_path_factory):
    """tests/cpp/pnp_lockstep.cc: the kernels' text compiled for the host as one thread per workgroup (no GPU, no HIP runtime)"""
    return build_lockstep(str(tmp_path_factory.mktemp("bin") / "pnp_lockstep"))


def run_lockstep(exe, tmp_path, name, env=None):
    b = S.batch(S.BATCH_3) if name == "batch_3" else S.single(name)
    (tmp_path / "in.bin").write_bytes(S.pack(b))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120, env=env)
    outs = S.unpack(b, (tmp_path / "out.bin").read_bytes())
    names = [S.BATCH_3[0], None] + list(S.BATCH_3[1:]) if name == "batch_3" else [name]
    assert len(outs) == len(names)
    for o, k in zip(outs, names):
        if k is None:
            i = o["info"]
            assert (i["n"], i["iterations"], i["hit_iteration"], i["best_iteration"], i["no_more"], i["pose"]) == (0, 0, -1, -1, 1, 0)
            assert not i["Tcw"].any() and o["counts"].size == 0 and o["flags"].size == 0
        else:
            S.assert_equals_restatement(o, S.reference(k))


@pytest.mark.parametrize("name", list(S.CASES) + ["batch_3"])
def test_kernel_text_as_host_threads_equals_the_restatement(lockstep, tmp_path, name):
    """Every output byte of every scene: counts, double models, float poses, chosen approximations, flags, refined counts, models,
    poses and flags of every slot, the info record, the returned and the kept flags (a NaN equals a NaN).  batch_3: three problems
    of different n and an empty one in one chain - each problem's bytes are those of its own run."""
    run_lockstep(lockstep, tmp_path, name)


def test_kernel_text_under_sanitizers(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined ends clean on the scenes that stress its indexing: the
    refinement past 1024 points, the prior slot, the batch with an empty problem, the degenerate set"""
    exe = build_lockstep(str(tmp_path / "pnp_lockstep_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name in ("n_1100", "two_calls", "batch_3", "duplicate", "n_4", "n_9", "planar"):
        run_lockstep(exe, tmp_path, name)


def test_library_exports_the_declared_entry_points(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbx.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(orbp_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert sorted(decl) == sorted(pkg.PNP_EXPORTS) and len(decl) == 3
    for L in (pkg.lib(), pkg.lib(developer=True)):
        for n, nargs in decl.items():
            assert hasattr(L, n) and len(getattr(L, n).argtypes) == nargs, n
    assert (pkg.PNP_CORR_DTYPE.itemsize, pkg.PNP_PROBLEM_DTYPE.itemsize, pkg.PNP_INFO_DTYPE.itemsize) == (24, 36, 164)
    assert pkg.PNP_CORR_DTYPE == R.CORR_DTYPE and pkg.PNP_PROBLEM_DTYPE == R.PROBLEM_DTYPE and pkg.PNP_INFO_DTYPE == R.INFO_DTYPE


def test_argument_errors_before_a_device(pkg):
    """every ORBX_ERR_ARG case of include/orbx.h, on a machine with or without a GPU: the checks come before the device is touched"""
    L = pkg.lib()
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    sc = S.case("hit_60")
    corrs, sets, prob = sc["corrs"], np.ascontiguousarray(sc["sets"][:8], np.int32), S.problem(sc)
    n = len(corrs)
    counts, inl, best, info = np.zeros(8, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(1, R.INFO_DTYPE)

    def f(corrs=corrs, n=n, prob=prob, sets=sets, its=8, prior=None, counts=counts, inl=inl, best=best, info=info):
        return L.orbp_pnp_ransac(p(corrs), n, p(prob), p(sets), its, p(prior), p(counts), None, None, None, None, None, p(inl), p(best), p(info), 0)
    for kw in (dict(corrs=None), dict(prob=None), dict(sets=None), dict(counts=None), dict(inl=None), dict(best=None), dict(info=None),
               dict(n=3), dict(n=-1), dict(its=-1)):
        assert f(**kw) == pkg.ORBX_ERR_ARG, kw
    bad = sets.copy(); bad[5, 1] = n
    assert f(sets=bad) == pkg.ORBX_ERR_ARG and b"out of 60" in L.orbx_last_error()
    bad = sets.copy(); bad[0, 0] = -1
    assert f(sets=bad) == pkg.ORBX_ERR_ARG
    bad = sets.copy(); bad[3, 3] = bad[3, 0]
    assert f(sets=bad) == pkg.ORBX_ERR_ARG and b"twice" in L.orbx_last_error()
    for v in (-1.0, np.nan, np.inf):
        bad = corrs.copy(); bad["sigma2"][7] = v
        assert f(corrs=bad) == pkg.ORBX_ERR_ARG and b"sigma2" in L.orbx_last_error(), v
    pr = prob.copy(); pr["prior_best_inliers"] = 3
    assert f(prob=pr) == pkg.ORBX_ERR_ARG and b"prior" in L.orbx_last_error()
    fl = np.zeros(n, np.uint8); fl[:5] = 1
    assert f(prob=pr, prior=fl) == pkg.ORBX_ERR_ARG
    pr = prob.copy(); pr["min_inliers"] = n + 1
    assert f(prob=pr) == pkg.ORBX_ERR_ARG and b"min_inliers" in L.orbx_last_error()
    b = S.batch(S.BATCH_3)
    B = len(b["problems"])
    nh, np_ = int(b["set_offsets"][-1]), int(b["offsets"][-1])
    cb, ib, bb, fb = np.zeros(nh, np.int32), np.zeros(np_, np.uint8), np.zeros(np_, np.uint8), np.zeros(B, R.INFO_DTYPE)

    def g(off=b["offsets"], soff=b["set_offsets"], B=B, sets=b["sets"]):
        return L.orbp_pnp_ransac_batch(p(b["corrs"]), p(off), B, p(b["problems"]), p(sets), p(soff), p(b["prior"]), p(cb), None, None, None, None,
                                       None, p(ib), p(bb), p(fb), 0)
    off = b["offsets"].copy(); off[2] = off[1] - 1
    assert g(off=off) == pkg.ORBX_ERR_ARG and b"decrease" in L.orbx_last_error()
    soff = b["set_offsets"].copy(); soff[3] = soff[2] - 1
    assert g(soff=soff) == pkg.ORBX_ERR_ARG
    off = b["offsets"].copy(); off[0] = -1
    assert g(off=off) == pkg.ORBX_ERR_ARG
    soff = b["set_offsets"].copy(); soff[1], soff[2] = soff[1] - 3, soff[1]    # the empty problem given three sets: n = 0 < 4
    assert g(soff=soff) == pkg.ORBX_ERR_ARG and b"4 are needed" in L.orbx_last_error()
    assert g(off=None) == pkg.ORBX_ERR_ARG and g(soff=None) == pkg.ORBX_ERR_ARG and g(B=-1) == pkg.ORBX_ERR_ARG


def test_draw_sets(pkg):
    for n in (4, 5, 65, 300):
        s = pkg.pnp_draw_sets(n, 50, np.random.default_rng(n))
        assert s.shape == (50, 4) and s.dtype == np.int32 and s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 4 for row in s.tolist())
    assert (pkg.pnp_draw_sets(4, 20, np.random.default_rng(1)).sum(axis=1) == 6).all()           # n = 4: every set a permutation
    a = pkg.pnp_draw_sets(40, 10, np.random.default_rng(7))
    rng = np.random.default_rng(7)
    assert (a == R.draw_sets(40, 10, lambda lo, hi: int(rng.integers(lo, hi + 1)))).all()        # the restatement's procedure
    with pytest.raises(ValueError):
        pkg.pnp_draw_sets(3, 1, np.random.default_rng(0))


def test_pnp_solver_needs_a_gpu(pkg):
    """no CPU fallback: without a device the calls fail with ORBX_ERR_NO_DEVICE; with one they work.  A solver with fewer
    correspondences than min_inliers answers no_more without a device either way."""
    sc = S.case("n_9")
    so = pkg.PnPsolver(sc["corrs"], sc["K"])
    so.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, no_more, inl, n = so.iterate(5)
    assert T is None and no_more and n == 0 and len(inl) == 9 and so.planned(5) == 0
    sc = S.case("n_4")
    so = pkg.PnPsolver(sc["corrs"], sc["K"])
    so.set_ransac_parameters(0.99, 4, 300, 4, 0.5, 5.991)
    assert (so.min_inliers, so.max_iterations, so.planned(5)) == (4, 1, 5)
    if pkg.device_count() == 0:
        with pytest.raises(pkg.OrbxError) as e:
            so.iterate(5, sc["sets"])
        assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
        assert pkg.lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    else:
        T, no_more, _, n = so.iterate(5, sc["sets"])
        assert T is not None and no_more and n == 4 and so.iterations == 5
