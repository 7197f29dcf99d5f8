"""GPU: k_init_normalize / k_init_ransac / k_init_select / k_init_reconstruct (orbi_*, csrc/orbx_initializer.hip) against the numpy
restatement tests/init_ref.py on every scene of tests/init_scene.py: CASES.  The conditions of the comparison are asserted first,
on the restatement's own trace.  Discrete outputs equal; the float outputs - the scores of all 2 x iterations hypotheses, H21,
F21, R21, t21, the points - BYTE-equal: the sums are ordered, nothing is contracted, and float / and sqrt are correctly rounded;
only the parallax goes through the device's math library (acosf): within 4 ulp.  Two runs byte-identical; the device form equal
to the host form, also past the LDS chunks; a second host thread after orbx_thread_release_scratch equal to the first; a thread
whose staging pair regrows in between equal to the single calls."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu


def run(pkg, sc):
    ini = pkg.Initializer(sc["keys1"], sc["K4"], sigma=sc["sigma"], iterations=sc["iterations"])
    full = ini.initialize(sc["keys2"], sc["matches"], sc["sets"], sc["min_parallax"], sc["min_triangulated"])
    return full, ini.search(sc["keys2"], sc["matches"], sc["sets"])


def info_bytes(info):
    return tuple(v.tobytes() if isinstance(v, np.ndarray) else v for _, v in sorted(info.items()))


def as_bytes(full, srch=None):
    ok, Rm, t, P, tri, info = full
    b = (ok, Rm.tobytes(), t.tobytes(), P.tobytes(), tri.tobytes(), info_bytes(info))
    if srch is not None:
        b += (srch[0].tobytes(), srch[1].tobytes(), srch[2].tobytes(), info_bytes(srch[3]))
    return b


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), np.float32(1e-30))))


def check_against_reference(name, full, srch):
    sc, r = S.assert_conditions(name)                  # the conditions first
    ok, Rm, t, P, tri, info = full
    scores, iH, iF, sinfo = srch
    s = r["search"]
    diff = np.abs(scores.astype(np.float64) - s["scores"].astype(np.float64))
    print("%s: scores differ in %d of %d, max %.3e; parallax %r (kernel) %r (restatement)" % (
        name, int((scores != s["scores"]).sum()), scores.size, float(np.nanmax(diff)), info["parallax"], float(r["parallax"])))
    # FindHomography / FindFundamental through orbi_search
    assert scores.tobytes() == s["scores"].tobytes()
    assert tuple(sinfo["best_iteration"]) == tuple(r["best"]) and tuple(sinfo["inliers"]) == r["inliers"]
    assert (iH == s["inliersH"]).all() and (iF == s["inliersF"]).all()
    assert sinfo["H21"].tobytes() == r["H21"].tobytes() and sinfo["F21"].tobytes() == r["F21"].tobytes()
    assert sinfo["ncand"] == 0 and sinfo["best_good"] == 0
    # the whole call
    for k in ("SH", "SF", "RH"):
        assert np.float32(info[k]).tobytes() == np.float32(r[k]).tobytes() == np.float32(sinfo[k]).tobytes(), k
    assert info["model"] == r["model"] == sinfo["model"] and tuple(info["best_iteration"]) == tuple(r["best"]) and tuple(info["inliers"]) == r["inliers"]
    assert info["H21"].tobytes() == r["H21"].tobytes() and info["F21"].tobytes() == r["F21"].tobytes()
    assert int(ok) == r["result"] and info["ncand"] == r["ncand"] and list(info["ngood"]) == r["ngood"]
    assert (info["best_good"], info["second_good"]) == (r["best_good"], r["second_good"])
    assert Rm.tobytes() == r["R21"].tobytes() and t.tobytes() == r["t21"].tobytes() and P.tobytes() == r["P3D"].tobytes()
    assert (tri == r["triangulated"]).all()
    assert ulps(info["parallax"], r["parallax"]) <= 4
    assert all(ulps(a, b) <= 4 for a, b in zip(info["cand_parallax"], r["cand_parallax"]))
    exp = S.CASES[name][1]
    assert exp[0] in (None, int(ok)) and exp[1] in (None, info["model"])


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_against_restatement(pkg, name):
    sc = S.case(name)
    full, srch = run(pkg, sc)
    check_against_reference(name, full, srch)
    again = run(pkg, sc)
    assert as_bytes(full, srch) == as_bytes(*again)                 # determinism: identical bytes in all outputs


def test_two_generators_give_two_self_consistent_answers(pkg):
    """200 iterations on the 257-match scene with sets from PCG64 and from MT19937: each equals its restatement
    (test_kernels_against_restatement), and the two have different winners"""
    a, b = run(pkg, S.case("wg_257")), run(pkg, S.case("wg_257_mt"))
    assert (S.case("wg_257")["keys1"] == S.case("wg_257_mt")["keys1"]).all() and (S.case("wg_257")["sets"] != S.case("wg_257_mt")["sets"]).any()
    assert a[0][5]["best_iteration"].tolist() != b[0][5]["best_iteration"].tolist()
    for name, (full, srch) in (("wg_257", a), ("wg_257_mt", b)):
        r = S.reference(name)
        assert tuple(full[5]["best_iteration"]) == tuple(r["best"]) and full[0] == bool(r["result"]) == True       # noqa: E712
        assert full[5]["inliers"][1] == int(srch[2].sum()) and full[4].sum() <= full[5]["best_good"]


def test_min_8_search_returns_models_and_inliers(pkg):
    sc = S.case("min_8")
    full, (scores, iH, iF, info) = run(pkg, sc)
    assert not full[0] and full[5]["best_good"] <= 50 and not full[1].any() and not full[3].any() and not full[4].any()
    assert info["best_iteration"][1] >= 0 and iF.all() and np.abs(info["F21"]).max() > 0


def test_degenerate_scene_terminates_with_clean_outputs(pkg):
    full, srch = run(pkg, S.case("degenerate"))
    ok, Rm, t, P, tri, info = full
    assert not ok and not Rm.any() and not t.any() and not P.any() and not tri.any() and np.isfinite(srch[0]).all()


def test_device_form_and_second_thread_equal_host_form(pkg):
    """keypoint records uploaded to the device (mvKeysUn of two device-resident frames): orbi_initialize_device equals the host form
    bit for bit - also from a second host thread, before and after it released its scratch"""
    import torch
    sc = S.case("general_150")
    host = pkg.Initializer(sc["keys1"], sc["K4"], iterations=sc["iterations"]).initialize(sc["keys2"], sc["matches"], sc["sets"])
    recs = []
    for k in (sc["keys1"], sc["keys2"]):
        kp = np.zeros(len(k), pkg.KP_DTYPE)
        kp["x"], kp["y"], kp["size"], kp["angle"], kp["octave"], kp["class_id"] = k[:, 0], k[:, 1], 31.0, 45.0, 1, -1
        recs.append(torch.from_numpy(kp.view(np.uint8).copy()).cuda())
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    args = (recs[0].data_ptr(), len(sc["keys1"]), recs[1].data_ptr(), len(sc["keys2"]), sc["matches"], sc["sets"], sc["K4"])
    dev = pkg.initialize_device(*args, stream=stream)
    assert as_bytes(dev) == as_bytes(host) and host[0]
    got = {}

    def second_thread():
        try:
            got["a"] = as_bytes(pkg.initialize_device(*args, stream=stream))
            assert pkg.matcher_lib().orbx_thread_release_scratch() == 0
            got["b"] = as_bytes(pkg.initialize_device(*args))
            got["c"] = as_bytes(pkg.Initializer(sc["keys1"], sc["K4"], iterations=sc["iterations"]).initialize(sc["keys2"], sc["matches"], sc["sets"]))
            assert pkg.matcher_lib().orbx_thread_release_scratch() == 0
        except Exception as e:      # noqa: BLE001
            got["error"] = e

    th = threading.Thread(target=second_thread)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    assert got["a"] == got["b"] == got["c"] == as_bytes(host)


def test_scratch_regrows_inside_one_thread(pkg):
    """a fresh host thread: wave_65 reserves the staging pair at its 1 MiB floor, regrow_513 - whose 2 x 1100 x 513 flag bytes alone
    exceed that floor - makes it regrow, wave_65 runs in the regrown pair; every output equals the same call from this thread
    (and regrow_513's equals its restatement: test_kernels_against_restatement)"""
    big, small = S.case("regrow_513"), S.case("wave_65")
    assert 2 * big["iterations"] * len(big["matches"]) > 1 << 20 > 64 * 2 * small["iterations"] * len(small["matches"])
    got = {}

    def worker():
        try:
            got["first"] = as_bytes(*run(pkg, small))
            got["big"] = as_bytes(*run(pkg, big))
            got["again"] = as_bytes(*run(pkg, small))
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001
            got["error"] = e

    th = threading.Thread(target=worker)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    assert got["big"] == as_bytes(*run(pkg, big))
    assert got["first"] == got["again"] == as_bytes(*run(pkg, small))
    assert got["rc"] == pkg.ORBX_OK == 0


def test_device_form_past_the_chunks(pkg):
    """chunk_1025 with keypoint records (stride 7) in HBM: three passes of k_init_ransac, two of k_init_normalize per frame, and the
    strided loop of k_init_reconstruct read their keys through the record stride; equal to the host form bit for bit"""
    import torch
    sc = S.case("chunk_1025")
    host = pkg.Initializer(sc["keys1"], sc["K4"], iterations=sc["iterations"]).initialize(sc["keys2"], sc["matches"], sc["sets"])
    recs = []
    for k in (sc["keys1"], sc["keys2"]):
        kp = np.zeros(len(k), pkg.KP_DTYPE)
        kp["x"], kp["y"], kp["size"], kp["angle"], kp["octave"], kp["class_id"] = k[:, 0], k[:, 1], 31.0, 45.0, 1, -1
        recs.append(torch.from_numpy(kp.view(np.uint8).copy()).cuda())
    assert pkg.KP_DTYPE.itemsize == 7 * 4 and len(sc["matches"]) == len(sc["keys1"]) == len(sc["keys2"]) == 1025
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    dev = pkg.initialize_device(recs[0].data_ptr(), len(sc["keys1"]), recs[1].data_ptr(), len(sc["keys2"]), sc["matches"], sc["sets"],
                                sc["K4"], stream=stream)
    assert as_bytes(dev) == as_bytes(host) and host[0]
    assert host[0] == bool(S.reference("chunk_1025")["result"]) and tuple(host[5]["best_iteration"]) == tuple(S.reference("chunk_1025")["best"])


def test_default_sets_are_drawn_when_none_are_given(pkg):
    sc = S.case("wave_65")
    ini = pkg.Initializer(sc["keys1"], sc["K4"], iterations=32)
    sets = pkg.draw_sets(65, 32, np.random.default_rng(0))
    assert as_bytes(ini.initialize(sc["keys2"], sc["matches"])) == as_bytes(ini.initialize(sc["keys2"], sc["matches"], sets))
