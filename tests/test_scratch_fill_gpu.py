"""No result depends on what fresh scratch memory held.

Every scratch block of the library - plan buffers, staging, frame records, the matchers' arena and its pinned mirror, the staging pairs,
the BoW scratch, the keyframe database, the cloud / octree / rgbd / rectify / stereo scratch - is written before it is read within a call,
or is one of the few buffers initialised at allocation (DESIGN.md section 4a lists who writes and who reads each).  The allocator hides a
violation: the first blocks of a process are zero pages, a recycled block holds what its last owner left.  Here every case runs three
times on FRESH scratch (a new handle, orbx_thread_release_scratch() for the thread's): with the developer build's fill
(orbx_debug_set_alloc_fill) off, with every new block filled with the word 1, and with 3.  Small words on purpose: one misread as a
count, an index or a level gives a wrong answer, not an access out of range.

Per case: the fill-off bytes equal the oracle or restatement the module's own test compares with (through that test's helper); the bytes
at fill 1 and at fill 3 equal the fill-off bytes over every output word; and orbx_debug_alloc_fill_stats shows at least the blocks
DESIGN.md section 4a lists for the call, i.e. the fill reached the code under test.

Two sizes differ from the sizes first asked for this file, because neither the reference nor the extractor accepts them: 160x120 has
room for 4 pyramid levels at scale 1.2, not 8 (level 4 would be 77x58, the reference needs 62x62: plan_size refuses, and so does the
oracle), so 160x120 runs with 4 levels and the smallest 4:3 size that takes 8 levels, 300x225, runs the 8-level case."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc          # noqa: E402
import tracking_chain as tc       # noqa: E402

pytestmark = pytest.mark.gpu
WORDS = (1, 3)
# blocks of a new extractor handle's first call: the corner-sparse word + the 19 plan buffers (plan_buffers; + 3 with shared sweeps)
PLAN_BLOCKS = 1 + 19
STAGING_BLOCKS = 1 + 3 + 3          # ensure_staging: d_in, d_kps / d_desc / d_counts and their pinned mirrors
STEREO_BLOCKS = 4                   # stereo_scratch_reserve: st_sad, st_rc, st_items, st_binStart
VIEW_BLOCKS = 2 + 2 + 1 + 1         # fv_d[2], fv_h[2], fv_stage (pageable images), fv_flag
ARENA_BLOCKS = 3                    # arena_begin: base, pinned mirror, completion word
PAIR_BLOCKS = 2                     # StagePair::reserve: device block + pinned mirror


class Fill:
    """Switches the fill for one test (the `fill` fixture) and runs a case three times on fresh scratch."""

    def __init__(self, pkg):
        self.pkg, self.L = pkg, pkg.matcher_lib()
        assert self.L._orbx_developer and pkg.lib(True) is self.L

    def fresh(self):
        gc.collect()                                       # handles of the previous run that nobody closed
        assert self.L.orbx_thread_release_scratch() == 0
        s = self.pkg.debug_thread_scratch()
        assert (s["arena_cap"], s["stage_cap"], s["bow_cap"], s["arena_word"]) == (0, 0, 0, 0), s

    def three(self, run, min_blocks, check=None, what=""):
        """run() -> {name: bytes / int / tuple}: creates its handles, makes its calls, closes the handles.  check(raw result of the
        fill-off run) pins the baseline to the oracle / restatement when run() does not do that itself."""
        outs, stats = [], []
        for word in (None,) + WORDS:
            self.fresh()
            self.pkg.debug_set_alloc_fill(word is not None, word or 0)
            try:
                raw = run()
                stats.append(self.pkg.debug_alloc_fill_stats())
            finally:
                self.pkg.debug_set_alloc_fill(0)
            if word is None and check is not None:
                check(raw)
            outs.append(raw["bytes"] if isinstance(raw, dict) and "bytes" in raw else raw)
        base = outs[0]
        assert stats[0] == (0, 0), stats                   # off is off
        for word, out, st in zip(WORDS, outs[1:], stats[1:]):
            assert sorted(out) == sorted(base), (what, word)
            for key in sorted(base):
                assert out[key] == base[key], "%s: %s differs with fresh scratch filled with %d" % (what, key, word)
            print("%s fill %d: %d blocks, %d bytes filled" % (what, word, st[0], st[1]))
            assert st[0] >= min_blocks and st[1] >= 4 * min_blocks, (what, word, st, min_blocks)
        return base


@pytest.fixture
def fill(pkg, hooks):
    """Switches the fill on for one test (Fill.three does), and off again; afterwards the thread's scratch is released and the handles are
    dropped.  The `hooks` fixture sends extractors and matchers to the developer build; the vocabulary, the keyframe database, the BoW
    matchers, the rectifier and the cloud mapper always load pkg.lib(), so for the test's duration that name answers with the developer
    build too (what ORBX_LIB does for the threads worker's process): the fill exists there only."""
    f = Fill(pkg)
    pkg.lib()
    kept, pkg._lib = pkg._lib, pkg.lib(True)
    try:
        yield f
    finally:
        pkg.debug_set_alloc_fill(0)
        gc.collect()
        f.L.orbx_thread_release_scratch()
        pkg._lib = kept


def _b(a):
    return np.ascontiguousarray(a).tobytes()


# ---------------------------------------------------------------------------------------------------------------- extraction
EXTRACT_SIZES = {"160x120_4lv": (160, 120, 300, 4, 31), "300x225_8lv": (300, 225, 300, 8, 32), "900x700_10lv": (900, 700, 500, 10, 87)}
_oracle_extract = {}


def oracle_extract(oracle, synth, w, h, nf, nl, seed):
    key = (w, h, nf, nl, seed)
    if key not in _oracle_extract:
        k, d = oracle.Extractor(nf, 1.2, nl, 20, 7).extract(synth.frame(w, h, seed))
        assert len(k) >= 4
        _oracle_extract[key] = (k.tobytes(), d.tobytes())
    return _oracle_extract[key]


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("size", sorted(EXTRACT_SIZES))
def test_extract_batch(pkg, oracle, synth, fill, size, B):
    """orbx_extract_batch on a new handle: B = 1 and 2 take the small-batch forms (level chains, the quad-tree fed by the FAST stage's
    histogram, whose buffers are the zero-initialised ones), B = 5 the batched forms (the cell lists swept in place: d_slots is read
    past each cell's last written entry, d_octPart / d_octBest past the level's).  Keypoints, descriptors and counts of every image."""
    w, h, nf, nl, seed = EXTRACT_SIZES[size]
    imgs = np.stack([synth.frame(w, h, seed + i) for i in range(B)])
    want = [oracle_extract(oracle, synth, w, h, nf, nl, seed + i) for i in range(B)]

    def run():
        ex = pkg.ORBextractor(nf, 1.2, nl, 20, 7)
        got = ex.extract_batch(imgs)
        p = ex.debug_last_plan()
        assert p["histOct"] == (B <= 4 and not p["strips"]), p       # up to ORBX_HIST_IMAGES images: the quad-tree loads the FAST stage's histogram
        ex.close()
        out = {"n": tuple(len(k) for k, _ in got)}
        for b, (k, d) in enumerate(got):
            out["k%d" % b], out["d%d" % b] = k.tobytes(), d.tobytes()
        return out

    def check(out):
        for b in range(B):
            assert (out["k%d" % b], out["d%d" % b]) == want[b], (size, B, b)
    fill.three(run, PLAN_BLOCKS + STAGING_BLOCKS, check, "extract_batch %s B=%d" % (size, B))


def test_extract_size_change_on_a_live_handle(pkg, oracle, synth, fill):
    """ensure_plan frees and reallocates every plan buffer when the size changes: 160x120, 333x257 and 160x120 again on one handle."""
    sizes = [(160, 120, 41), (333, 257, 42), (160, 120, 43)]
    want = [oracle_extract(oracle, synth, w, h, 300, 4, s) for w, h, s in sizes]

    def run():
        ex = pkg.ORBextractor(300, 1.2, 4, 20, 7)
        out = {}
        for i, (w, h, s) in enumerate(sizes):
            k, d = ex(synth.frame(w, h, s))
            out["k%d" % i], out["d%d" % i] = k.tobytes(), d.tobytes()
        ex.close()
        return out

    def check(out):
        for i in range(3):
            assert (out["k%d" % i], out["d%d" % i]) == want[i], i
    fill.three(run, 3 * (PLAN_BLOCKS - 1) + 1, check, "size change")


STEREO_SIZES = {"300x225": (300, 225, 300, 5), "900x700": (900, 700, 500, 6)}
_oracle_stereo = {}


def oracle_stereo(oracle, synth, w, h, nf, k):
    """What tracking_chain.OracleBackend.frame computes (the reference of the stereo frame tests), for the 10-level size too."""
    if (w, h, nf, k) not in _oracle_stereo:
        nl = 10 if w == 900 else 8
        left, right = synth.stereo_pair_blocky(w, h, k)
        el, er = oracle.Extractor(nf, 1.2, nl, 20, 7), oracle.Extractor(nf, 1.2, nl, 20, 7)
        kl, dl = el.extract(left)
        kr, dr = er.extract(right)
        mbf = 47.9
        mb = float(np.float32(mbf) / np.float32(435.2))
        n, ur, dp = oracle.stereo_match(kl, dl, kr, dr, [el.pyramid_level(i) for i in range(nl)], [er.pyramid_level(i) for i in range(nl)],
                                        el.scale_factors, el.inv_scale_factors, mbf, mb)
        assert n >= 4 and len(kl) >= 4 and len(kr) >= 4, (n, len(kl), len(kr))
        _oracle_stereo[(w, h, nf, k)] = (left, right, nl, mbf, mb,
                                         {"kl": kl.tobytes(), "dl": dl.tobytes(), "kr": kr.tobytes(), "dr": dr.tobytes(), "uright": _b(ur), "depth": _b(dp),
                                          "nmatch": int(n)})
    return _oracle_stereo[(w, h, nf, k)]


def _hbm(ptr, nbytes):
    """nbytes of device memory at ptr, after the call has synchronised."""
    import torch    # noqa: F401  (the HIP runtime the process already uses answers to this name once torch is loaded)
    out = np.zeros(max(nbytes, 1), np.uint8)
    hip = C.CDLL("libamdhip64.so")
    if nbytes:
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(2)) == 0
    return out[:nbytes].tobytes()


@pytest.mark.parametrize("form", ["stereo_frame", "stereo_frame_view"])
@pytest.mark.parametrize("size", sorted(STEREO_SIZES))
def test_stereo_frame(pkg, oracle, synth, fill, size, form):
    """orbx_stereo_frame and orbx_stereo_frame_view (pageable images: staged through fv_stage) on a new handle, two calls each so that both
    frame records of the view form are used: keypoints, descriptors, mvuRight, mvDepth and the counts; for the view form the pinned
    record as the caller sees it AND the record in HBM, downloaded after a synchronisation."""
    w, h, nf, k = STEREO_SIZES[size]
    left, right, nl, mbf, mb, want = oracle_stereo(oracle, synth, w, h, nf, k)
    keys = ("kl", "dl", "kr", "dr", "uright", "depth")

    def run():
        ex = pkg.ORBextractor(nf, 1.2, nl, 20, 7)
        out = {}
        for call in range(2):
            f = getattr(ex, form)(left, right, mbf, mb)
            for key in keys:
                out["%s%d" % (key, call)] = _b(f[key])
            out["nmatch%d" % call] = int(f["nmatch"])
            if form == "stereo_frame_view":
                v, a, b = f["view"], len(f["kl"]), len(f["kr"])
                for key, ptr, n in (("kl", v.d_kl, 28 * a), ("dl", v.d_dl, 32 * a), ("kr", v.d_kr, 28 * b), ("dr", v.d_dr, 32 * b),
                                    ("uright", v.d_uright, 4 * a), ("depth", v.d_depth, 4 * a)):
                    out["hbm_%s%d" % (key, call)] = _hbm(ptr, n)
        ex.close()
        return out

    def check(out):
        for call in range(2):
            for key in keys:
                assert out["%s%d" % (key, call)] == want[key], (form, call, key)
                if form == "stereo_frame_view":
                    assert out["hbm_%s%d" % (key, call)] == want[key], (form, call, "HBM " + key)
            assert out["nmatch%d" % call] == want["nmatch"]
    blocks = PLAN_BLOCKS + STEREO_BLOCKS + (VIEW_BLOCKS if form == "stereo_frame_view" else STAGING_BLOCKS + 2)
    fill.three(run, blocks, check, "%s %s" % (form, size))


# ------------------------------------------------------------------------------------------------------------ the latency chain
CHAIN = (320, 240, 400, 4)


def test_latency_chain(pkg, oracle, synth, fill):
    """tracking_chain.Chain on GpuViewBackend for 4 frames (orbx_stereo_frame_view, orbm_search_by_projection_frame_device,
    orbm_search_local_points_device: the tracking role of tests/test_match_threads_gpu.py) with the thread's scratch released first,
    so that the arena, its mirror and the completion word are re-created filled; the log equals the oracle chain's.
    320x240 with 400 features: checked on the CPU, the oracle chain's tracked frames have proj_n = 81, 102, 95 and local_n = 1, 3, 6;
    with 300 features local_n of frame 1 is 0, and the next smaller 4:3 sizes (288x216, 256x192) have no room for 8 levels."""
    w, h, nf, nframes = CHAIN
    frames, _ = synth.stereo_sequence(w, h, nframes, k=11, step=0.04)
    poses = tc.poses(nframes, 0.04)
    ref = tc.Chain(tc.OracleBackend(w, h, nf), w, h, nf)
    for t in range(nframes):
        ref.step(frames[t][0], frames[t][1], poses[t])
    assert all(s["proj_n"] >= 20 and s["local_n"] > 0 for s in ref.log[1:]), [(s["proj_n"], s["local_n"]) for s in ref.log[1:]]

    def run():
        be = tc.GpuViewBackend(w, h, nf)
        c = tc.Chain(be, w, h, nf)
        paths = []
        for t in range(nframes):
            c.step(frames[t][0], frames[t][1], poses[t])
            paths.append(pkg.debug_match_path()[0])
        assert set(paths[1:]) <= {pkg.RES_PAR_Q2, pkg.RES_PAR_Q4}, paths      # the completion word was used
        out = {"%s%d" % (key, t): s.get(key) for t, s in enumerate(c.log) for key in tc.COMPARED}
        log = [dict(s) for s in c.log]
        del c
        be.exl.close(); be.exr.close()
        return {"bytes": out, "log": log}

    def check(raw):
        assert tc.first_difference(ref.log, raw["log"]) is None, tc.first_difference(ref.log, raw["log"])
    fill.three(run, PLAN_BLOCKS + VIEW_BLOCKS + STEREO_BLOCKS + ARENA_BLOCKS, check, "latency chain")


# ------------------------------------------------------------------------------------------- guided searches, BoW: tests/match_cases.py
@pytest.fixture(scope="module")
def cases(pkg, oracle, synth):
    """The calls tests/match_threads_worker.py replays, with their oracle results (computed once, never modified), + SearchLocalPoints
    with 3000 world points (k_resolve_par with 4 queries per thread)."""
    frame = mc.limits_frame(oracle, synth)
    lm, _ = mc.local_mapping_cases(pkg, oracle, synth)
    lc, _ = mc.loop_closing_cases(pkg, oracle, synth, frame)
    by = {c.name: c for c in lm + lc}
    by["search_local_points_3000"] = mc.local_points_case(pkg, oracle, synth, 3000, "search_local_points_3000")
    return by


def _case_run(pkg, case, shared_voc=False):
    def run():
        shared = {}
        if shared_voc:
            voc = mc.vocabulary()
            shared["voc"] = pkg.Vocabulary(10, 3, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
        got = case.run(pkg, shared)
        path = pkg.debug_match_path()[:2] if case.guided else None
        bad = []
        import match_threads_worker as worker
        worker.check_results("0", 0, case.name, got, case.want, bad)          # the comparison the threaded test makes
        return {"bytes": {k: (_b(v) if isinstance(v, np.ndarray) else int(v)) for k, v in got.items()}, "bad": bad, "path": path}
    return run


def _oracle_equal(raw):
    assert raw["bad"] == [], raw["bad"]


# (case, thread option, resolver the call must report)
GUIDED = [("search_by_projection", None, "RES_PAR_Q2"), ("search_local_points_3000", None, "RES_PAR_Q4"), ("match_windows", None, "RES_PAR_Q2"),
          ("search_by_projection", "fast_wave", "RES_WAVE"), ("match_windows", "fast_wave", "RES_WAVE"),
          ("search_local_points_3000", "fast_wave", "RES_WAVE"),
          ("search_by_projection", "exact", "RES_EXACT"), ("match_windows", "exact", "RES_EXACT"), ("search_local_points_3000", "exact", "RES_EXACT"),
          ("search_for_initialization", None, "RES_WAVE"), ("search_for_initialization_513", None, "RES_EXACT"),
          ("search_for_initialization", "exact", "RES_EXACT")]
OPTIONS = {"fast_wave": (3, 1), "exact": (2, 1)}


@pytest.mark.parametrize("name,option,resolver", GUIDED, ids=["%s-%s" % (n, o or "default") for n, o, _ in GUIDED])
def test_guided_search(pkg, fill, cases, name, option, resolver):
    """Every resolver path of the guided searches at the sizes of tests/match_cases.py: k_resolve_par with 2 and with 4 queries per
    thread, the single-wave resolvers, the exact kernels by option, and SearchForInitialization in both forms (k_resolve_init; the
    exact kernel behind a window of 513 candidates).  The path is asserted through orbm_debug_match_path."""
    case = cases[name]
    run0 = _case_run(pkg, case)

    def run():
        if option:
            assert fill.L.orbm_set_thread_option(*OPTIONS[option]) == 0
        try:
            raw = run0()
        finally:
            if option:
                fill.L.orbm_set_thread_option(OPTIONS[option][0], 0)
        assert raw["path"][0] == getattr(pkg, resolver), (name, option, raw["path"])
        if option == "exact":
            assert raw["path"][1] == pkg.FB_OPTION
        return raw
    # the exact kernels of the host-array entry points work in the staging pair; the fast path in the arena (a fall-back has used both)
    blocks = PAIR_BLOCKS if option == "exact" else ARENA_BLOCKS + (PAIR_BLOCKS if resolver == "RES_EXACT" else 0)
    fill.three(run, blocks, _oracle_equal, "%s (%s)" % (name, option or "default"))


@pytest.mark.parametrize("name", ["orbv_transform", "search_by_bow_kf_frame", "search_by_bow_kf_kf", "search_for_triangulation", "best_in_windows"])
def test_bow_and_windows(pkg, fill, cases, name):
    """orbv_transform on a new vocabulary handle, SearchByBoW (both variants) and SearchForTriangulation at the crowded nodes - all in
    the thread's BoW scratch - and orbm_best_in_windows (arena)."""
    blocks = {"orbv_transform": 3 + 1, "best_in_windows": ARENA_BLOCKS - 1}.get(name, 1)
    fill.three(_case_run(pkg, cases[name], shared_voc=name == "orbv_transform"), blocks, _oracle_equal, name)


def test_stereo_batch_matcher(pkg, oracle, synth, fill):
    """orbm_stereo_batch_device behind orbx_extract_batch_device (tracking_chain.GpuDeviceBackend.frame: one handle, image slots 0 / 1)
    against the oracle's stereo frame; the matcher's scratch (SAD values, right records, row bins, bin entries) is the handle's."""
    w, h, nf, k = STEREO_SIZES["300x225"]
    left, right, nl, mbf, mb, want = oracle_stereo(oracle, synth, w, h, nf, k)

    def run():
        be = tc.GpuDeviceBackend(w, h, nf)
        f = be.frame(left, right, mbf, mb)
        path = pkg.debug_stereo_path()
        out = {"kl": _b(f["k"]), "dl": _b(f["d"]), "uright": _b(f["uright"]), "depth": _b(f["depth"]), "useLds": path[0]}
        be.exl.close(); be.exr.close()
        return out

    def check(out):
        for key in ("kl", "dl", "uright", "depth"):
            assert out[key] == want[key], key
        assert out["useLds"] == 1
    fill.three(run, PLAN_BLOCKS + STEREO_BLOCKS, check, "stereo batch")


# ------------------------------------------------------------------------------------------- one small scene per remaining module
def test_keyframe_database(pkg, fill):
    """add, erase, re-add, a loop query and relocalisation queries (the scene of test_reloc_erase_and_readd): every hit list equals the
    restatement's inside Pair, in all three runs; across the runs the hits' bytes and the candidate lists are compared."""
    import test_kfdb_gpu as K
    S = K.S

    def run():
        rng = np.random.default_rng(29)
        p = K.Pair(pkg, 2000, initial_entries=64)          # (a small pool: the adds make it regrow)
        wa, wb = list(range(0, 40, 2)), list(range(1000, 1040, 2))
        qa, qb = S.bow(rng, wa), S.bow(rng, wb)
        v1 = S.bow(rng, wa[:18] + [1000] + list(range(500, 520)))
        p.add(1, v1)
        p.add(2, S.bow(rng, [1000] + wb[1:] + list(range(700, 730))))
        p.add(3, S.bow(rng, [1000] + wb[2:] + list(range(800, 810))))
        p.cov(2, [1, 3]); p.cov(1, [2]); p.cov(3, [1])
        out = {}
        p.reloc(qa); p.reloc(qb)
        p.erase(1)
        p.reloc(qb)
        p.add(1, v1)
        p.cov(1, [2])
        for i, (q, kind) in enumerate(((qa, "reloc"), (qb, "reloc"), (qb, "loop"))):
            if kind == "reloc":
                p.reloc(q)
                cand, hits = p.db.detect_relocalization_candidates(*S.arrays(q), hits=True)
            else:
                p.loop(q, [3], 0.0)
                cand, hits = p.db.detect_loop_candidates(*S.arrays(q), [3], 0.0, hits=True)
            out["cand%d" % i], out["hits%d" % i] = tuple(int(c) for c in cand), _b(hits)
        out["scores"] = _b(p.score(qb, [2, 3, 1]))
        del p
        return out
    fill.three(run, 3 + 4 + 1 + 1, None, "keyframe database")      # pool (2) + pinned buffer, 4 slot arrays, id -> slot, query scratch


def test_pose_optimization(pkg, fill):
    import test_poseopt_gpu as T
    name = "mixed300"
    sc, mark, ref, dev = T.reference(name)

    def run():
        res = pkg.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=mark)
        return {"bytes": dict(enumerate(T.as_bytes(res))), "res": res}
    fill.three(run, PAIR_BLOCKS, lambda raw: T.check_against_reference(name, raw["res"]), "pose optimisation")


def test_initializer(pkg, fill):
    import test_initializer_gpu as T
    sc = T.S.case("wave_65")

    def run():
        full, srch = T.run(pkg, sc)
        return {"bytes": dict(enumerate(T.as_bytes(full, srch))), "res": (full, srch)}
    fill.three(run, PAIR_BLOCKS, lambda raw: T.check_against_reference("wave_65", *raw["res"]), "Initializer")


def test_sim3(pkg, fill):
    import test_sim3_gpu as T
    sc = T.S.case("wave_65")
    keys = ("counts", "models", "flags", "hit_inliers", "n", "iterations", "hit_iteration", "best_iteration", "best_inliers", "s", "R", "t", "T12")

    def run():
        o = pkg.sim3_ransac_batch(sc["pairs"], [0, len(sc["pairs"])], T.S.problem(sc), sc["sets"], [0, len(sc["sets"])])[0]
        return {"bytes": {k: _b(np.asarray(o[k])) for k in keys}, "res": o}

    def check(raw):                       # that file's comparison with the restatement, on this result
        kept = T._runs.get("wave_65")
        T._runs["wave_65"] = raw["res"]
        try:
            T.test_kernels_equal_the_restatement(pkg, "wave_65")
        finally:
            if kept is None:
                del T._runs["wave_65"]
            else:
                T._runs["wave_65"] = kept
    fill.three(run, PAIR_BLOCKS, check, "Sim3")


def test_pnp(pkg, fill):
    import test_pnp_gpu as T
    sc = T.S.case("wave_65")

    def run():
        o = T.call(pkg, sc)
        return {"bytes": {k: _b(np.asarray(o[k])) for k in T.KEYS}, "res": o}
    fill.three(run, PAIR_BLOCKS, lambda raw: T.S.assert_equals_restatement(T.as_lockstep(raw["res"]), T.S.reference("wave_65"), full=False), "PnP")


def test_rgbd_frame(pkg, oracle, synth, fill):
    """orbx_rgbd_frame 321x241 (odd size), TUM1 distortion, 16-bit depth, on a new handle."""
    import test_rgbd_gpu as T
    w, h, kind, cam = 321, 241, "u16", T.R.TUM1
    k = w + h + len(kind) + len("tum1")
    channels, rgb = (3, True) if k % 3 == 0 else (4, False) if k % 3 == 1 else (3, False)
    color = T.colorize(synth.frame(w, h, k), channels, k)
    depth, factor = T.depth_image(w, h, kind, k)
    ok, od = oracle.Extractor(T.NF, 1.2, 8, 20, 7).extract(T.R.gray_from_color(color, rgb))

    def run():
        ex = pkg.ORBextractor(T.NF, 1.2, 8, 20, 7)
        r = ex.rgbd_frame(color, depth, pkg.RGBDCamera(**cam), factor, rgb=rgb)
        ex.close()
        return {"bytes": {f: _b(r[f]) for f in r}, "res": r}

    def check(raw):
        r = raw["res"]
        T.assert_kp_equal(r["kp"], ok)
        np.testing.assert_array_equal(r["desc"], od)
        T.assert_assoc_bits(r["kun"], r["uright"], r["depth"], r["kp"], depth, factor, cam)
    fill.three(run, PLAN_BLOCKS + 3, check, "rgbd frame")


def test_rectified_stereo_frame(pkg, oracle, synth, fill):
    """orbx_stereo_frame_rectified on the EuRoC maps, colour input: new rectifiers (maps, tiles) and a new handle (raw-pair scratch)."""
    import test_rectify_gpu as T
    w, h = T.R.EUROC_SIZE
    left, right = T.colour_pair(*synth.stereo_pair_blocky(w, h, 7))
    holder = {}

    def run():
        (rl, ml), (rr, mr) = T.make(pkg, "euroc_752x480"), T.make(pkg, "euroc_right")
        holder["maps"] = (ml, mr)
        ex = pkg.ORBextractor(T.NF, 1.2, 8, 20, 7)
        got = ex.stereo_frame_rectified(rl, rr, left, right, T.MBF, T.MB, rgb=False)
        out = {f: _b(got[f]) for f in ("kl", "dl", "kr", "dr", "uright", "depth")}
        out["nmatch"] = int(got["nmatch"])
        ex.close(); rl.close(); rr.close()
        return {"bytes": out, "res": got}

    def check(raw):
        got, (ml, mr) = raw["res"], holder["maps"]
        gl, gr = T.R.rectify_gray(left, *ml, rgb=False), T.R.rectify_gray(right, *mr, rgb=False)
        okl, odl = oracle.Extractor(T.NF, 1.2, 8, 20, 7).extract(gl)
        okr, odr = oracle.Extractor(T.NF, 1.2, 8, 20, 7).extract(gr)
        T.assert_kp_equal(got["kl"], okl, "left ")
        T.assert_kp_equal(got["kr"], okr, "right ")
        assert (got["dl"] == odl).all() and (got["dr"] == odr).all() and got["nmatch"] > 5
    fill.three(run, PLAN_BLOCKS + STEREO_BLOCKS + 2 * 5, check, "rectified stereo frame")      # a rectifier: two maps, the fixed-point form, tiles, tap boxes


def test_cloud(pkg, fill):
    """generate at 61x47 (three frames, three poses, holes of every kind) and the voxel filter of 1025 points at leaf 0.25 (two radix
    passes; the sort's buffers hold 1025 pairs of a capacity of 2048), each on a new mapper."""
    import torch
    import test_cloud_gpu as T
    w, h, B, step = 61, 47, 3, 2
    modes = ("holes", "none", "all")
    colors = [T.colour_image(w, h, 4, b) for b in range(B)]
    dd = [T.depth_image(w, h, "u16", b, modes[b]) for b in range(B)]
    depths, factor = [d for d, _ in dd], dd[0][1]
    poses = [T.pose(b) for b in range(B)]
    cloud = T.random_cloud(1025)

    def run():
        m = pkg.CloudMapper(0.1, step, 202)
        got, n = T.gpu_generate(pkg, torch, m, colors, depths, factor, poses, m.capacity(w, h))
        m.close()
        m2 = pkg.CloudMapper(0.25, 3, 255)
        vox, vn = T.gpu_voxel(pkg, torch, m2, [cloud])
        m2.close()
        out = {"gen%d" % b: g.tobytes() for b, g in enumerate(got)}
        out.update(n=tuple(int(x) for x in n), vox=vox[0].tobytes(), vn=int(vn[0]))
        return {"bytes": out, "res": (got, vox, vn)}

    def check(raw):
        got, vox, vn = raw["res"]
        for b in range(B):
            T.assert_same(got[b], T.R.generate(colors[b], depths[b], T.CAM["fx"], T.CAM["fy"], T.CAM["cx"], T.CAM["cy"], poses[b], factor, step, 202), "frame %d" % b)
        ref, rn = T.ref_voxel(1025, 0, 0.25)
        assert vn[0] == rn > 300
        T.assert_same(vox[0], ref)
    fill.three(run, 1 + 3, check, "cloud")


def test_octomap(pkg, fill):
    """random_sparse_3001 and the three-segment batch (a full, an empty and a short segment) on a new mapper: data bytes (.bt), leaf
    rows and the info record."""
    import torch
    import test_octomap_gpu as T
    pts = T.random_points(3001, 11)
    cap = 1100
    a, c = T.random_points(cap + 5, 50), T.random_points(37, 51, 2.0, (3, 3, 3))
    ref1 = T.R.octomap(pts, T.R.AXIS_SWAP, 0.1)
    ref2 = T.R.octomap(np.concatenate([a[:cap], c]), T.R.AXIS_SWAP, 0.1)

    def run():
        m = pkg.CloudMapper(0.1, 3, 255)
        out = {}
        for i, (segs, ref, kw) in enumerate((([pts], ref1, {}), ([a, np.zeros((0, 3), np.float32), c], ref2, dict(counts=[cap + 5, 0, 37], cap=cap)))):
            data, leaves, info = T.gpu_octree(pkg, torch, m, segs, None, 0.1, ref["data_bytes"] + 32, ref["leaves"] + 4, **kw)
            out["bt%d" % i], out["leaves%d" % i], out["info%d" % i] = data, leaves.tobytes(), tuple(sorted(info.items()))
        m.close()
        return out

    def check(out):
        for i, ref in enumerate((ref1, ref2)):
            info = dict(out["info%d" % i])
            for f in T.INFO_FIELDS:
                assert info[f] == ref[f], (i, f)
            assert info["overflow"] == 0 and out["bt%d" % i] == ref["data"] and out["leaves%d" % i] == ref["leaf_rows"].astype(np.int64).tobytes()
    fill.three(run, 4, check, "octomap")
