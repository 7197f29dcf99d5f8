"""Stream order under injected stalls (DESIGN.md section 4b lists every event / stream wait and the case here that fails without it).

Every other GPU test compares results after the device is idle, with inputs complete before the call: a forgotten hipStreamWaitEvent
changes nothing there, the unordered work finishes microseconds later and the test reads milliseconds later.  Here ONE stream is held
back by tens of milliseconds (orbx_debug_stall_stream, tests/stream_stall.py) in front of the work, the results are consumed on the
caller's stream with no host wait in between, and only that stream is synchronised before the comparison - with what the suite already
compares that entry point with (the CPU oracle, a numpy restatement, or the host form the suite pins the device form to).  Until the
stalled work runs, every buffer it writes holds a different but VALID content (another image, another frame's records), so a stale
read gives a wrong answer, never an access out of range.

A case means something only if (a) the stall lasts (calibrate), (b) the stalled stream and the stream that must wait do not share a
hardware queue (independent; up to four arrangements are tried, then the case FAILS naming the pair) and (c) the stall was still pending
when the host had issued everything (or, for calls that return results to the host, the call lasted at least the measured stall).
The negative control shows what a missing wait looks like in this harness: a consumer on a second stream that does not wait sees the
stale outputs.

Measured on the MI355X (the run that completed this file; `-s` prints the same lines): calibrate: a nominal 30 ms stall 30.004 ms, a
nominal 50 ms stall 50.004 ms (three brackets each, 30.004 - 30.008 and 50.004 - 50.005).  Host-returning calls behind a stall, from the
stall's launch to the call's return: orbx_rgbd_frame 30.1 ms; orbx_stereo_frame_view, orbm_search_local_points and its _device form
50.1 ms each, polling and ORBX_OPT_STREAM_SYNC / ORBM_OPT_STREAM_SYNC = 1 alike.  Effective pairs (arrangement 0 = the first one tried):

  case                                                   stalled / must wait (or runs free)                  outcome
  chunks 2, 3 [sides]                                    side0 (+ side1) / caller's stream                   effective, arrangement 0
  chunks 2, 3 [caller]                                   caller's stream / side0 (+ side1)                   effective, arrangement 0
  early quad-tree, split call [side1]                    side1 / caller's stream                             effective, arrangement 0
  early quad-tree, split call [caller]                   caller's stream / side1                             effective, arrangement 0
  rgbd_frame depth upload                                side1 / the handle's stream                         effective, arrangement 0
  prefetch on a stalled side stream, 2 and 3 buffers     side0 / caller's stream                             effective, arrangement 0
  prefetch beside a stalled main stream, 2 and 3         caller's stream / side0                             effective, arrangement 0
  matcher behind evFastDone                              caller's stream / side0                             effective, arrangement 0
  stereo_frame_view, search_local_points (host arrays)   the stream the call itself works on                 no pair: one stream
  search_local_points_device                             caller's stream / default stream                    effective, arrangement 0 or 1
  extract + stereo, gray + extract + rgbd                caller's stream / default, main, side0, side1       effective, arrangement 0 or 1
  rectify, cloud + voxel + octree, hamming + pack,       caller's stream / default stream                    effective, arrangement 0 or 1
  search_by_projection_frame + pose, initialize
  negative control                                       caller's stream / the stream that does not wait     effective, arrangement 0; the clone saw
                                                                                                             the previous call's outputs
  FrontEnd pipelined, _late, _late_fast_alone            every ordered pair of main, side                    effective, arrangement 0
  FrontEnd pipelined_late_two_side                       every ordered pair of main, side, side2             effective, arrangement 0
  FrontEnd host streaming                                every ordered pair of main, side, hs.up, hs.down    effective, arrangement 0

No pair was inseparable, no case is marked.  Which arrangement is the first effective one depends on how many streams the process has
created before (the runtime deals them to its hardware queues round-robin), so it differs between a run of this file alone and a run
of the whole suite; the cases print theirs.  34 cases, 9 s.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_stall as SS          # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "orb_slam2v2-1_amd"
W, H, NF, NL = 320, 240, 300, 8
BW, BH, BNF = 752, 480, 900       # the smallest size at which the tests of ORBX_OPT_EARLY_OCTREE / _SPLIT_CALL reach those arrangements
MBF, FX = 386.1448, 718.856
MB = float(np.float32(MBF) / np.float32(FX))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def ref():
    import oracle
    oracle.build()
    return importlib.import_module("oracle.reference_frames")


@pytest.fixture(scope="module")
def stall_ms(pkg):
    """The measured length of a nominal 30 / 50 ms stall (once per session; asserted to be at least half the nominal length)."""
    SS.use(pkg)
    return SS.calibrate()


_mono = {}


def mono_sets(ref, w, h, nf, B, nsets, seed0):
    """nsets batches of B synthetic images with the oracle's keypoints and descriptors; computed once, never modified."""
    key = (w, h, nf, B, nsets, seed0)
    if key not in _mono:
        _mono[key] = [ref.run_pool(ref.mono_frame, [(w, h, nf, seed0 + 50 * s + i) for i in range(B)]) for s in range(nsets)]
    return _mono[key]


_stereo = {}


def stereo_sets(ref, w, h, nf, B, nsets, seed0):
    key = (w, h, nf, B, nsets, seed0)
    if key not in _stereo:
        _stereo[key] = [ref.run_pool(ref.stereo_frame, [(w, h, nf, seed0 + 50 * s + i, MBF, MB) for i in range(B)]) for s in range(nsets)]
    return _stereo[key]


class Out:
    """Device outputs of an extraction call on B images (+ clones of them, taken on a stream)."""

    def __init__(self, torch, B, cap):
        self.torch, self.B, self.cap = torch, B, cap
        self.kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
        self.desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(B, dtype=torch.int32, device="cuda")

    def args(self):
        return self.kps.data_ptr(), self.desc.data_ptr(), self.cnt.data_ptr()

    def clone_on(self, stream):
        with self.torch.cuda.stream(stream):
            return self.kps.clone(), self.desc.clone(), self.cnt.clone()


def images_mismatch(pkg, snap, want, exact=True):
    """snap = (kps, desc, cnt) tensors; want = [(keypoints, descriptors)] of the oracle -> None or a short description.  exact: all 28
    bytes of every keypoint record (tests/test_extract_gpu.py: test_device_batch_on_a_torch_side_stream); else the comparison of
    oracle.reference_frames.image_mismatch (angle within 1e-4), which the tests of the split call and of pipeline.FrontEnd use."""
    import oracle.reference_frames as rf
    kps, desc, cnt = (t.cpu().numpy() for t in snap)
    B, cap = kps.shape[:2]
    k8 = kps.view(np.uint8).reshape(B, cap, 28)
    for b, (ok, od) in enumerate(want):
        n = int(cnt[b])
        if n != len(ok):
            return "image %d: count %d != %d" % (b, n, len(ok))
        if exact:
            if k8[b, :n].tobytes() != ok.tobytes():
                return "image %d: keypoints differ" % b
            if desc[b, :n].tobytes() != od.tobytes():
                return "image %d: descriptors differ" % b
        else:
            m = rf.image_mismatch(np.frombuffer(k8[b, :n].tobytes(), pkg.KP_DTYPE), desc[b, :n], ok, od)
            if m:
                return "image %d: %s" % (b, m)
    return None


def caller_stream(torch, what, others=()):
    """An effective non-default stream for the caller's side: work on the default stream and on `others` (raw streams the library owns)
    does not queue behind it, so library work that went to one of them instead of the caller's stream would run during the stall."""
    def arrange(attempt):
        s = SS.fresh_caller_stream()
        return s, [(s.cuda_stream, 0, ("caller's stream", "default stream"))] + [(s.cuda_stream, o, ("caller's stream", n)) for n, o in others]
    return SS.effective(arrange, what)


def test_hooks_refuse_bad_arguments_and_name_the_streams(pkg, hooks, torch, synth, stall_ms):
    L = pkg.lib(True)
    for us in (0, -1, 50001):
        assert L.orbx_debug_stall_stream(None, us, 0) == pkg.ORBX_ERR_ARG
    assert L.orbx_debug_streams(None, None, 5) == pkg.ORBX_ERR_ARG
    import ctypes as C
    out = (C.c_void_p * 5)()
    assert L.orbx_debug_streams(None, out, 4) == pkg.ORBX_ERR_ARG and L.orbx_debug_streams(None, out, 6) == pkg.ORBX_ERR_ARG
    s = pkg.debug_streams(None)
    assert s["main"] == s["side0"] == s["side1"] == 0
    ex = pkg.ORBextractor(NF, 1.2, NL, 20, 7)
    s = pkg.debug_streams(ex)
    assert s["main"] and s["side0"] == ex.side_stream() and len({s["main"], s["side0"], s["side1"]}) == 3
    assert stall_ms[SS.STALL_MS] >= 15 and stall_ms[SS.POLL_STALL_MS] >= 25
    ex.close()


# ------------------------------------------------------------------------------------------------------------------ internal joins
def _join_case(pkg, torch, ref, what, opts, stalled, B, big, plan_check, exact=True):
    """extract_batch_device under `opts` with the streams `stalled` held back (names of orbx_debug_streams, or "caller"): set 0 first
    (outputs and every scratch then hold set 0's results), the stall, the images of set 1 copied in on the caller's stream, the call,
    the outputs cloned on the caller's stream, that stream alone synchronised.  A handle stream held back shows a join the caller's
    stream lacks; the caller's stream held back shows a handle stream that starts without waiting for it."""
    w, h, nf = (BW, BH, BNF) if big else (W, H, NF)
    sets = mono_sets(ref, w, h, nf, B, 2, 4100 if big else 4000)
    want = [[(e["k"], e["d"]) for e in s] for s in sets]
    runs_free = ["side0", "side1"][:opts[8] - 1] if 8 in opts else ["side1"]      # the handle streams the arrangement runs on

    def arrange(attempt):
        ex = pkg.ORBextractor(nf, 1.2, NL, 20, 7)
        for k, v in opts.items():
            ex.set_option(k, v)
        caller = SS.fresh_caller_stream()
        st = dict(pkg.debug_streams(ex), caller=caller.cuda_stream)
        pairs = []
        for n in stalled:
            pairs += [(st["caller"], st[m], ("caller's stream", m)) for m in runs_free] if n == "caller" else [(st[n], st["caller"], (n, "caller's stream"))]
        return (ex, caller, st), pairs
    ex, caller, st = SS.effective(arrange, what)
    ex(sets[0][0]["img"])
    cap = ex.max_keypoints()
    d = [torch.from_numpy(np.stack([e["img"] for e in s])).cuda() for s in sets]
    d_in = d[0].clone()
    out = Out(torch, B, cap)
    torch.cuda.synchronize()
    cs = caller.cuda_stream
    ex.extract_batch_device(d_in.data_ptr(), B, w, h, w, w * h, *out.args(), cap, cs)
    caller.synchronize()
    assert images_mismatch(pkg, (out.kps, out.desc, out.cnt), want[0], exact) is None
    stalls = [SS.stall(st[n], SS.STALL_MS) for n in stalled]
    with torch.cuda.stream(caller):
        d_in.copy_(d[1], non_blocking=True)
    ex.extract_batch_device(d_in.data_ptr(), B, w, h, w, w * h, *out.args(), cap, cs)
    snap = out.clone_on(caller)
    pending = [s.pending() for s in stalls]
    caller.synchronize()
    bad = images_mismatch(pkg, snap, want[1], exact)
    for s in stalls:
        s.wait()
    assert all(pending), "%s: a stall was over before the call had been issued: %s" % (what, pending)
    assert bad is None, "%s with %s held back: %s" % (what, stalled, bad)
    plan_check(ex, ex.debug_last_plan())
    ex.close()


@pytest.mark.parametrize("held", ["sides", "caller"])
@pytest.mark.parametrize("chunks", [2, 3])
def test_chunks_join_the_callers_stream(pkg, hooks, torch, ref, stall_ms, chunks, held):
    """ORBX_OPT_CHUNKS: chunk 1 runs on side[0], chunk 2 on side[1].  evJoin orders the caller's stream behind them (the side streams
    held back); evPyr orders each chunk behind the one in front, and so behind the images the caller's stream still produces (the
    caller's stream held back, the images arriving behind the stall)."""
    B = 4

    def plan(ex, p):
        ex.fast_kernels(B)
        assert ex.fast_images_per_launch == B // chunks and not p["histOct"], (chunks, ex.fast_images_per_launch, p)   # lastChunks = chunks
    _join_case(pkg, torch, ref, "chunks=%d, %s held back" % (chunks, held), {8: chunks}, ["side0", "side1"][:chunks - 1] if held == "sides" else ["caller"],
               B, False, plan)


@pytest.mark.parametrize("held", ["side1", "caller"])
def test_early_octree_joins_the_callers_stream(pkg, hooks, torch, ref, stall_ms, held):
    """ORBX_OPT_EARLY_OCTREE = 2: the quad-tree of levels 0 and 1 on side[1] behind evGather (the caller's stream held back: without the
    wait it sweeps the previous call's cell lists), the caller's stream behind evOctA (side[1] held back)."""
    def plan(ex, p):
        assert p["octForm"] == pkg.OCT_EARLY and p["earlyLv"] == 2 and p["aSplit"] == 0 and p["strips"], p
    _join_case(pkg, torch, ref, "early quad-tree, %s held back" % held, {19: 2, 6: 3}, [held], 8, True, plan)


@pytest.mark.parametrize("held", ["side1", "caller"])
def test_split_call_joins_the_callers_stream(pkg, hooks, torch, ref, stall_ms, held):
    """ORBX_OPT_SPLIT_CALL = 3: the quad-tree of levels [0, 3) on side[1] behind evGather, their descriptors behind evOctA."""
    def plan(ex, p):
        assert p["octForm"] == pkg.OCT_SPLIT and p["aSplit"] == 3 and p["earlyLv"] == 0, p
    _join_case(pkg, torch, ref, "split call, %s held back" % held, {15: 3}, [held], 8, True, plan, exact=False)


def test_rgbd_frame_waits_for_its_depth_upload(pkg, hooks, torch, synth, oracle, stall_ms):
    """orbx_rgbd_frame uploads the depth image on side[1] behind evDepth: two calls with two depth images, the upload stream held back
    before the second - its association must be the second image's."""
    import test_rgbd_gpu as TR
    import rgbd_ref
    cam = rgbd_ref.TUM1
    color = TR.colorize(synth.frame(W, H, 77), 3, 77)
    (d1, factor), (d2, _) = TR.depth_image(W, H, "u16", 1), TR.depth_image(W, H, "u16", 2)
    d2 = np.ascontiguousarray(d2[::-1])           # (nothing like the first)
    ok, od = oracle.Extractor(NF, 1.2, NL, 20, 7).extract(rgbd_ref.gray_from_color(color, True))

    def arrange(attempt):
        ex = pkg.ORBextractor(NF, 1.2, NL, 20, 7)
        st = pkg.debug_streams(ex)
        return (ex, st), [(st["side1"], st["main"], ("side1", "main"))]
    ex, st = SS.effective(arrange, "rgbd_frame depth upload")
    r1 = ex.rgbd_frame(color, d1, pkg.RGBDCamera(**cam), factor)
    TR.assert_assoc_bits(r1["kun"], r1["uright"], r1["depth"], r1["kp"], d1, factor, cam, "first depth ")
    s = SS.stall(st["side1"], SS.STALL_MS)
    r2 = ex.rgbd_frame(color, d2, pkg.RGBDCamera(**cam), factor)
    ms = s.since()
    print("rgbd_frame behind a %.1f ms stall of its upload stream: %.1f ms" % (stall_ms[SS.STALL_MS], ms))
    assert ms >= stall_ms[SS.STALL_MS], (ms, stall_ms)
    s.wait()
    TR.assert_kp_equal(r2["kp"], ok)
    np.testing.assert_array_equal(r2["desc"], od)
    assert r1["depth"].tobytes() != r2["depth"].tobytes()
    TR.assert_assoc_bits(r2["kun"], r2["uright"], r2["depth"], r2["kp"], d2, factor, cam, "second depth ")
    ex.close()


def _prefetch_handle(pkg, torch, what, buffers, stalled_is_side):
    def arrange(attempt):
        ex = pkg.ORBextractor(NF, 1.2, NL, 20, 7)
        caller = SS.fresh_caller_stream()
        st = pkg.debug_streams(ex)
        pair = (st["side0"], caller.cuda_stream, ("side0", "caller's stream")) if stalled_is_side else \
               (caller.cuda_stream, st["side0"], ("caller's stream", "side0"))
        return (ex, caller, st), [pair]
    ex, caller, st = SS.effective(arrange, what)
    ex.set_pyramid_buffers(buffers)
    return ex, caller, st


@pytest.mark.parametrize("buffers", [2, 3])
def test_extraction_waits_for_the_pyramid_built_ahead(pkg, hooks, torch, ref, stall_ms, buffers):
    """The side stream is held back before prefetch_batch_device: the extraction that takes that pyramid waits for evPrefetch.  Without
    the wait its FAST stage reads the buffer's previous pyramid - another batch's."""
    B = 3
    sets = mono_sets(ref, W, H, NF, B, 3, 4200)
    want = [[(e["k"], e["d"]) for e in s] for s in sets]
    ex, caller, st = _prefetch_handle(pkg, torch, "prefetch on a stalled side stream, %d buffers" % buffers, buffers, True)
    ex(sets[0][0]["img"])
    cap = ex.max_keypoints()
    d = [torch.from_numpy(np.stack([e["img"] for e in s])).cuda() for s in sets]
    out = Out(torch, B, cap)
    torch.cuda.synchronize()
    cs = caller.cuda_stream
    for i in range(4):                       # every buffer of the rotation has held a pyramid, every first-time allocation is done
        ex.prefetch_batch_device(d[i % 3].data_ptr(), B, W, H, W, W * H)
        ex.extract_batch_device(d[i % 3].data_ptr(), B, W, H, W, W * H, *out.args(), cap, cs)
    caller.synchronize()
    assert images_mismatch(pkg, (out.kps, out.desc, out.cnt), want[0]) is None
    s = SS.stall(st["side0"], SS.STALL_MS)
    ex.prefetch_batch_device(d[1].data_ptr(), B, W, H, W, W * H)
    ex.extract_batch_device(d[1].data_ptr(), B, W, H, W, W * H, *out.args(), cap, cs)
    snap = out.clone_on(caller)
    pending = s.pending()
    caller.synchronize()
    bad = images_mismatch(pkg, snap, want[1])
    s.wait()
    assert pending, "the stall was over before the calls had been issued"
    assert bad is None, bad
    ex.close()


@pytest.mark.parametrize("buffers", [2, 3])
def test_pyramids_built_ahead_of_a_stalled_main_stream(pkg, hooks, torch, ref, stall_ms, buffers):
    """The caller's stream is held back before extraction i (its pyramid was built ahead); prefetch and extraction of i+1, i+2, i+3
    follow at once.  The pyramid of a later batch goes into the buffer extraction i still has to read as soon as the rotation comes
    round (two buffers: i+2, three: i+3): it must wait for evFastDone of the extraction issued in front of it."""
    B = 3
    sets = mono_sets(ref, W, H, NF, B, 3, 4200)
    want = [[(e["k"], e["d"]) for e in s] for s in sets]
    ex, caller, st = _prefetch_handle(pkg, torch, "prefetch beside a stalled main stream, %d buffers" % buffers, buffers, False)
    ex(sets[0][0]["img"])
    cap = ex.max_keypoints()
    d = [torch.from_numpy(np.stack([e["img"] for e in s])).cuda() for s in sets]
    outs = [Out(torch, B, cap) for _ in range(4)]
    torch.cuda.synchronize()
    cs = caller.cuda_stream

    def pre(i):
        ex.prefetch_batch_device(d[i % 3].data_ptr(), B, W, H, W, W * H)

    def ext(i, o):
        ex.extract_batch_device(d[i % 3].data_ptr(), B, W, H, W, W * H, *o.args(), cap, cs)
    for i in range(4):
        pre(i)
        ext(i, outs[i])                      # (every output holds a valid result of ANOTHER batch than the one it gets below)
    pre(5)
    caller.synchronize()
    ex_side = torch.cuda.ExternalStream(st["side0"])
    ex_side.synchronize()
    s = SS.stall(cs, SS.STALL_MS)
    for n, i in enumerate(range(5, 9)):
        ext(i, outs[n])
        if i < 8:
            pre(i + 1)
    snaps = [o.clone_on(caller) for o in outs]
    pending = s.pending()
    caller.synchronize()
    bad = [images_mismatch(pkg, snaps[n], want[i % 3]) for n, i in enumerate(range(5, 9))]
    ex_side.synchronize()
    assert pending, "the stall was over before the calls had been issued"
    assert bad == [None] * 4, bad
    ex.close()


def test_matcher_behind_the_fast_stage_of_a_stalled_extraction(pkg, hooks, torch, ref, stall_ms):
    """pipeline.FrontEnd's side-stream job: the main stream is held back before extraction 1, stream_wait_fast_stage orders the side
    stream behind its FAST stage, and the stereo matcher of extraction 0 (on the previous pyramid) follows there.  Consumed on the
    side stream."""
    B = 2
    sets = stereo_sets(ref, W, H, NF, B, 2, 4300)
    ex, caller, st = _prefetch_handle(pkg, torch, "matcher behind evFastDone", 2, False)
    side = torch.cuda.ExternalStream(st["side0"])
    imgs = [np.concatenate([np.stack([e["left"] for e in s]), np.stack([e["right"] for e in s])]) for s in sets]
    ex(imgs[0][0])
    cap = ex.max_keypoints()
    d = [torch.from_numpy(x).cuda() for x in imgs]
    outs = [Out(torch, 2 * B, cap) for _ in range(2)]
    ur = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    dp = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cs = caller.cuda_stream

    def match(o, stream, prev):
        pkg.stereo_batch_device(ex, ex, B, 0, B, o.kps.data_ptr(), o.desc.data_ptr(), o.cnt.data_ptr(), o.kps[B:].data_ptr(),
                                o.desc[B:].data_ptr(), o.cnt[B:].data_ptr(), cap, MBF, MB, ur.data_ptr(), dp.data_ptr(), nm.data_ptr(), stream, prev=prev)
    ex.prefetch_batch_device(d[1].data_ptr(), 2 * B, W, H, W, W * H)          # (the handle has built ahead: extractions record evFastDone)
    ex.extract_batch_device(d[1].data_ptr(), 2 * B, W, H, W, W * H, *outs[1].args(), cap, cs)
    match(outs[1], cs, False)                                                  # ur / dp / nm hold the OTHER batch's results
    ex.extract_batch_device(d[0].data_ptr(), 2 * B, W, H, W, W * H, *outs[0].args(), cap, cs)
    ex.prefetch_batch_device(d[1].data_ptr(), 2 * B, W, H, W, W * H)
    caller.synchronize()
    side.synchronize()
    s = SS.stall(cs, SS.STALL_MS)
    ex.extract_batch_device(d[1].data_ptr(), 2 * B, W, H, W, W * H, *outs[1].args(), cap, cs)
    ex.stream_wait_fast_stage(st["side0"])
    match(outs[0], st["side0"], True)
    with torch.cuda.stream(side):
        snap = (ur.clone(), dp.clone(), nm.clone(), outs[0].cnt.clone())
    pending = s.pending()
    side.synchronize()
    g_ur, g_dp, g_nm, g_cnt = (t.cpu().numpy() for t in snap)
    bad = [ref.stereo_mismatch((g_ur[b, :g_cnt[b]], g_dp[b, :g_cnt[b]], int(g_nm[b])), sets[0][b]) for b in range(B)]
    caller.synchronize()
    assert pending, "the stall was over before the calls had been issued"
    assert bad == [None] * B, bad
    assert sum(e["nmatch"] for e in sets[0]) > 0 and [e["nmatch"] for e in sets[0]] != [e["nmatch"] for e in sets[1]]
    want1 = [(e["kl"], e["dl"]) for e in sets[1]] + [(e["kr"], e["dr"]) for e in sets[1]]
    assert images_mismatch(pkg, (outs[1].kps, outs[1].desc, outs[1].cnt), want1) is None
    ex.close()


# ------------------------------------------------------------------------------------------------------- fall-backs of the polls
@pytest.mark.parametrize("sync", [0, 1])
def test_stereo_frame_view_behind_a_stalled_handle_stream(pkg, hooks, torch, synth, stall_ms, sync):
    """orbx_stereo_frame_view polls the completion word for a few ms, then waits for the stream (ORBX_OPT_STREAM_SYNC = 1: at once).
    h->stream is held back for 50 ms: the record returned must be this frame's, not the one the pinned record held two calls ago."""
    frames, _ = synth.stereo_sequence(W, H, 3, k=23, step=0.04)
    ex, ex2 = pkg.ORBextractor(NF, 1.2, NL, 20, 7), pkg.ORBextractor(NF, 1.2, NL, 20, 7)
    ex.set_option(27, sync)
    st = pkg.debug_streams(ex)
    want = [ex2.stereo_frame(l, r, MBF, MB) for l, r in frames]
    keys = ("kl", "dl", "kr", "dr", "uright", "depth")
    assert any(want[0][k].tobytes() != want[2][k].tobytes() for k in keys)
    for t in (0, 1):
        f = ex.stereo_frame_view(*frames[t], MBF, MB)
        assert all(f[k].tobytes() == want[t][k].tobytes() for k in keys) and f["nmatch"] == want[t]["nmatch"]
    s = SS.stall(st["main"], SS.POLL_STALL_MS)
    f = ex.stereo_frame_view(*frames[2], MBF, MB)
    ms = s.since()
    print("stereo_frame_view (stream sync %d) behind a %.1f ms stall: %.1f ms" % (sync, stall_ms[SS.POLL_STALL_MS], ms))
    s.wait()
    for k in keys:
        assert f[k].tobytes() == want[2][k].tobytes(), k
    assert f["nmatch"] == want[2]["nmatch"]
    assert ms >= stall_ms[SS.POLL_STALL_MS], (ms, stall_ms)
    ex.close(); ex2.close()


_local = {}


def local_points_scene(pkg, oracle, synth):
    """Tracking::SearchLocalPoints on a 1241x376 frame with 1500 world points (tests/match_cases.py: local_points_case; k_resolve_par)."""
    if not _local:
        import match_cases as mc
        c = mc.local_points_case(pkg, oracle, synth, 1500, "search_local_points_1500")
        ks_, w, h, rng, k, d, sf, cam, log_sf, T, pts3, wp, pd, obs = mc.local_map(pkg, oracle, synth, 7, m=1500)
        n = len(k)
        uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 40, n), -1).astype(np.float32)
        frame_mp = np.full(n, -1, np.int32)
        held = rng.choice(n, 150, replace=False)
        frame_mp[held[:75]] = rng.choice(len(wp), 75, replace=False)
        frame_mp[held[75:]] = -2
        ext_obs = rng.integers(0, 3, n).astype(np.int32)
        pcam = pkg.Camera(mc.ks.FX, mc.ks.FY, mc.ks.CX, mc.ks.CY, mc.ks.MBF, np.float32(mc.ks.MBF) / np.float32(mc.ks.FX))
        _local.update(k=k, d=d, uright=uright, geom=pkg.grid_geom(w, h), sf=sf, wp=wp, pd=pd, T=T, cam=pcam,
                      thr=pkg.predict_scale_thresholds(log_sf, 8), frame_mp=frame_mp, ext_obs=ext_obs, want=c.want)
    return _local


def _local_result(res):
    return {"nmatches": res[0], "frame_mp": res[1], "projections": np.frombuffer(res[2].tobytes(), np.uint8)}


def _same(got, want):
    return all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in want)


@pytest.mark.parametrize("sync", [0, 1])
def test_guided_search_behind_a_stalled_arena_stream(pkg, hooks, torch, oracle, synth, stall_ms, sync):
    """orbm_search_local_points, host arrays, the fast path: arena_wait polls the completion word, then waits for the thread's arena
    stream (ORBM_OPT_STREAM_SYNC = 1: at once).  The arena's pinned mirror holds the previous call's results until the kernels run."""
    sc = local_points_scene(pkg, oracle, synth)
    L = pkg.matcher_lib()
    L.orbm_set_thread_option(4, sync)
    try:
        def call(frame_mp):
            return _local_result(pkg.search_local_points(sc["k"], sc["d"], sc["uright"], sc["geom"], sc["sf"], sc["wp"], sc["pd"], sc["T"], sc["cam"], 0.5,
                                                         sc["thr"], frame_mp, sc["ext_obs"], 1.0, 0.8))
        other = call(np.full(len(sc["k"]), -1, np.int32))       # another valid call: its results are what the mirror holds
        assert pkg.debug_match_path()[:2] == (pkg.RES_PAR_Q2, pkg.FB_NONE), pkg.debug_match_path()
        assert not _same(other, sc["want"])
        arena = pkg.debug_streams(None)["arena"]
        assert arena
        s = SS.stall(arena, SS.POLL_STALL_MS)
        got = call(sc["frame_mp"])
        ms = s.since()
        print("search_local_points (stream sync %d) behind a %.1f ms stall of the arena stream: %.1f ms" % (sync, stall_ms[SS.POLL_STALL_MS], ms))
        s.wait()
        assert pkg.debug_match_path()[:2] == (pkg.RES_PAR_Q2, pkg.FB_NONE), pkg.debug_match_path()
        assert _same(got, sc["want"])
        assert ms >= stall_ms[SS.POLL_STALL_MS], (ms, stall_ms)
    finally:
        L.orbm_set_thread_option(4, 0)


def _late_records(torch, real, stale):
    """Device arrays that hold `stale` now; -> (destinations, sources) for the copies that bring `real` in behind a stall."""
    dst = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in stale]
    src = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in real]
    return dst, src


def _behind_stall(torch, S, ms, dst, src, call):
    """The stall on S, the copies of the real inputs behind it, then the call (which returns results to the host)."""
    s = SS.stall(S.cuda_stream, ms)
    with torch.cuda.stream(S):
        for a, b in zip(dst, src):
            a.copy_(b, non_blocking=True)
    got = call()
    took = s.since()
    s.wait()
    return got, took


@pytest.mark.parametrize("sync", [0, 1])
def test_guided_search_device_form_behind_a_stalled_callers_stream(pkg, hooks, torch, oracle, synth, stall_ms, sync):
    """orbm_search_local_points_device on the caller's stream, held back for 50 ms with the frame's records arriving behind the stall
    (until then the arrays hold the same frame rotated by 17 keypoints): poll, then the stream wait; the frame read must be the late one."""
    sc = local_points_scene(pkg, oracle, synth)
    n = len(sc["k"])
    S = caller_stream(torch, "search_local_points_device")
    real = (sc["k"], sc["d"], sc["uright"])
    dst, src = _late_records(torch, real, [np.roll(a, 17, axis=0) for a in real])
    torch.cuda.synchronize()
    L = pkg.matcher_lib()
    L.orbm_set_thread_option(4, sync)
    try:
        def call():
            return _local_result(pkg.search_local_points_device(dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), n, sc["geom"], sc["sf"], sc["wp"],
                                                                sc["pd"], sc["T"], sc["cam"], 0.5, sc["thr"], sc["frame_mp"], sc["ext_obs"], 1.0, 0.8, 0,
                                                                S.cuda_stream))
        stale = call()
        assert not _same(stale, sc["want"])
        got, ms = _behind_stall(torch, S, SS.POLL_STALL_MS, dst, src, call)
        print("search_local_points_device (stream sync %d) behind a %.1f ms stall: %.1f ms" % (sync, stall_ms[SS.POLL_STALL_MS], ms))
        assert pkg.debug_match_path()[:2] == (pkg.RES_PAR_Q2, pkg.FB_NONE), pkg.debug_match_path()
        assert _same(got, sc["want"])
        assert ms >= stall_ms[SS.POLL_STALL_MS], (ms, stall_ms)
    finally:
        L.orbm_set_thread_option(4, 0)


# ------------------------------------------------------------------------------------------- the caller's stream as the only order
def _consume(torch, S, copies, launch, outputs):
    """launch(raw stream) once on what the destinations hold now (valid stale inputs -> valid stale outputs), then: the stall, the
    copies that bring the real inputs in, the call, the outputs cloned - all on S, no host wait; S alone is synchronised.
    -> (stale outputs, outputs) as numpy arrays."""
    launch(S.cuda_stream)
    S.synchronize()
    stale = [o.cpu().numpy().copy() for o in outputs]
    s = SS.stall(S.cuda_stream, SS.STALL_MS)
    with torch.cuda.stream(S):
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)
    launch(S.cuda_stream)
    with torch.cuda.stream(S):
        clones = [o.clone() for o in outputs]
    pending = s.pending()
    S.synchronize()
    got = [c.cpu().numpy() for c in clones]
    assert pending, "the stall was over before the call had been issued"
    assert any(a.tobytes() != b.tobytes() for a, b in zip(stale, got)), "the stale inputs give the same outputs: the case shows nothing"
    return stale, got


def test_callers_stream_extract_and_stereo(pkg, hooks, torch, ref, stall_ms):
    """orbx_extract_batch_device + orbm_stereo_batch_device: the images arrive behind the stall, the matcher reads what the extraction
    in front of it on the same stream produces."""
    B = 2
    sets = stereo_sets(ref, W, H, NF, B, 2, 4300)
    imgs = [np.concatenate([np.stack([e["left"] for e in s]), np.stack([e["right"] for e in s])]) for s in sets]
    ex = pkg.ORBextractor(NF, 1.2, NL, 20, 7)
    st = pkg.debug_streams(ex)
    S = caller_stream(torch, "extract + stereo", [(n, st[n]) for n in ("main", "side0", "side1")])
    ex(imgs[0][0])
    cap = ex.max_keypoints()
    d_in, d_real = torch.from_numpy(imgs[0]).cuda(), torch.from_numpy(imgs[1]).cuda()
    o = Out(torch, 2 * B, cap)
    ur = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    dp = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def launch(s):
        ex.extract_batch_device(d_in.data_ptr(), 2 * B, W, H, W, W * H, *o.args(), cap, s)
        pkg.stereo_batch_device(ex, ex, B, 0, B, o.kps.data_ptr(), o.desc.data_ptr(), o.cnt.data_ptr(), o.kps[B:].data_ptr(), o.desc[B:].data_ptr(),
                                o.cnt[B:].data_ptr(), cap, MBF, MB, ur.data_ptr(), dp.data_ptr(), nm.data_ptr(), s)
    _, got = _consume(torch, S, [(d_in, d_real)], launch, [o.kps, o.desc, o.cnt, ur, dp, nm])
    snap = tuple(torch.from_numpy(g) for g in got[:3])
    want = [(e["kl"], e["dl"]) for e in sets[1]] + [(e["kr"], e["dr"]) for e in sets[1]]
    assert images_mismatch(pkg, snap, want) is None, images_mismatch(pkg, snap, want)
    cnt = got[2]
    for b in range(B):
        m = ref.stereo_mismatch((got[3][b, :cnt[b]], got[4][b, :cnt[b]], int(got[5][b])), sets[1][b])
        assert m is None, (b, m)
    ex.close()


def test_negative_control_a_consumer_that_does_not_wait_sees_stale_outputs(pkg, hooks, torch, ref, stall_ms):
    """The consumer pattern above with the clone issued on a SECOND effective stream that does not wait for the caller's: it must see
    the outputs of the call before (another batch's).  If it saw the new ones, the arrangement could not detect a missing wait."""
    B = 3
    sets = mono_sets(ref, W, H, NF, B, 2, 4000)
    want = [[(e["k"], e["d"]) for e in s] for s in sets]
    ex = pkg.ORBextractor(NF, 1.2, NL, 20, 7)

    def arrange(attempt):
        s1, s2 = SS.fresh_caller_stream(), SS.fresh_caller_stream()
        return (s1, s2), [(s1.cuda_stream, s2.cuda_stream, ("caller's stream", "the stream that does not wait"))]
    S1, S2 = SS.effective(arrange, "negative control")
    ex(sets[0][0]["img"])
    cap = ex.max_keypoints()
    d_in, d_real = torch.from_numpy(np.stack([e["img"] for e in sets[0]])).cuda(), torch.from_numpy(np.stack([e["img"] for e in sets[1]])).cuda()
    o = Out(torch, B, cap)
    torch.cuda.synchronize()
    ex.extract_batch_device(d_in.data_ptr(), B, W, H, W, W * H, *o.args(), cap, S1.cuda_stream)
    S1.synchronize()
    s = SS.stall(S1.cuda_stream, SS.STALL_MS)
    with torch.cuda.stream(S1):
        d_in.copy_(d_real, non_blocking=True)
    ex.extract_batch_device(d_in.data_ptr(), B, W, H, W, W * H, *o.args(), cap, S1.cuda_stream)
    early = o.clone_on(S2)                   # no S2.wait_stream(S1): the missing wait
    right = o.clone_on(S1)
    S2.synchronize()
    pending = s.pending()
    S1.synchronize()
    assert pending, "the stall was over before the unordered clone had run"
    assert images_mismatch(pkg, right, want[1]) is None
    bad = images_mismatch(pkg, early, want[1])
    assert bad is not None, "a clone that did not wait equals the oracle: this arrangement cannot detect a missing wait"
    assert images_mismatch(pkg, early, want[0]) is None, "the stale outputs are not the previous call's"
    ex.close()


def test_callers_stream_gray_extract_rgbd(pkg, hooks, torch, synth, stall_ms):
    """orbx_gray_from_color_device -> orbx_extract_batch_device -> orbm_rgbd_batch_device on one stream: colour and depth images arrive
    behind the stall (tests/test_rgbd_gpu.py: test_batch_device_equals_frame - each frame equals rgbd_frame of that frame)."""
    import test_rgbd_gpu as TR
    import rgbd_ref
    B, cam, factor = 2, rgbd_ref.TUM1, 1.0 / 5000
    colors = [np.stack([TR.colorize(synth.frame(W, H, 60 + 10 * s + b), 4, b) for b in range(B)]) for s in range(2)]
    depths = [np.stack([TR.depth_image(W, H, "u16", 3 * s + b)[0] for b in range(B)]) for s in range(2)]
    ex = pkg.ORBextractor(NF, 1.2, NL, 20, 7)
    st = pkg.debug_streams(ex)
    S = caller_stream(torch, "gray + extract + rgbd", [(n, st[n]) for n in ("main", "side0", "side1")])
    ex(np.zeros((H, W), np.uint8) + 90)
    cap = ex.max_keypoints() + 64
    d_col, d_dep = torch.from_numpy(colors[0]).cuda(), torch.from_numpy(depths[0]).cuda()
    r_col, r_dep = torch.from_numpy(colors[1]).cuda(), torch.from_numpy(depths[1]).cuda()
    gs = W + 64
    d_gray = torch.zeros((B, H, gs), dtype=torch.uint8, device="cuda")
    o = Out(torch, B, cap)
    kun = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    ur = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    dp = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def launch(s):
        pkg.gray_from_color_device(d_col.data_ptr(), B, W, H, 4, False, W * 4, W * H * 4, d_gray.data_ptr(), gs, gs * H, s)
        ex.extract_batch_device(d_gray.data_ptr(), B, W, H, gs, gs * H, *o.args(), cap, s)
        pkg.rgbd_batch_device(o.kps.data_ptr(), o.cnt.data_ptr(), B, cap, d_dep.data_ptr(), pkg.DEPTH_U16, W, H, W * 2, W * H * 2, factor,
                              pkg.RGBDCamera(**cam), kun.data_ptr(), ur.data_ptr(), dp.data_ptr(), s)
    _, got = _consume(torch, S, [(d_col, r_col), (d_dep, r_dep)], launch, [d_gray, o.kps, o.desc, o.cnt, kun, ur, dp])
    g_gray, g_kps, g_desc, n, g_kun, g_ur, g_dp = got
    np.testing.assert_array_equal(g_gray[:, :, :W], rgbd_ref.gray_from_color(colors[1], False))
    g_kps, g_kun = g_kps.view(pkg.KP_DTYPE).reshape(B, cap), g_kun.view(pkg.KP_DTYPE).reshape(B, cap)
    ex1 = pkg.ORBextractor(NF, 1.2, NL, 20, 7)
    for b in range(B):
        r = ex1.rgbd_frame(colors[1][b], depths[1][b], pkg.RGBDCamera(**cam), factor, rgb=False)
        m = n[b]
        assert m == len(r["kp"]) > 50, b
        assert g_kps[b, :m].tobytes() == r["kp"].tobytes() and g_desc[b, :m].tobytes() == r["desc"].tobytes(), b
        assert g_kun[b, :m].tobytes() == r["kun"].tobytes(), b
        assert g_ur[b, :m].tobytes() == r["uright"].tobytes() and g_dp[b, :m].tobytes() == r["depth"].tobytes(), b
    ex.close(); ex1.close()


def test_callers_stream_rectify(pkg, torch, synth, stall_ms):
    """orbx_rectify_device: the raw images arrive behind the stall (tests/test_rectify_gpu.py: byte for byte against rectify_ref)."""
    import test_rectify_gpu as TQ
    import rectify_ref
    (r0, m0), (r1, m1) = TQ.make(pkg, "odd_333x221"), TQ.make(pkg, "odd_333x221")
    w, h = TQ.MAP_CASES["odd_333x221"][4:]
    B, B0 = 2, 1
    raw = [TQ.raw_images(synth, B, w, h, 1, k0=10 * s) for s in range(2)]
    S = caller_stream(torch, "rectify")
    d_src, d_real = torch.from_numpy(np.stack(raw[0])).cuda(), torch.from_numpy(np.stack(raw[1])).cuda()
    d_out = torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def launch(s):
        pkg.rectify_device(r0, r1, B0, d_src.data_ptr(), B, w, h, 1, 1, w, w * h, d_out.data_ptr(), w, w * h, s)
    _, (got,) = _consume(torch, S, [(d_src, d_real)], launch, [d_out])
    for b in range(B):
        mx, my = m0 if b < B0 else m1
        np.testing.assert_array_equal(got[b], rectify_ref.rectify_gray(raw[1][b], mx, my, rgb=True), err_msg="image %d" % b)


def test_callers_stream_cloud_voxel_octree(pkg, torch, stall_ms):
    """orbx_cloud_generate_device -> orbx_cloud_voxel_device -> orbx_octree_device on one stream, colour and depth arriving behind the
    stall (tests/test_cloud_gpu.py, tests/test_octomap_gpu.py: against cloud_ref and octomap_ref)."""
    import test_cloud_gpu as TC
    import cloud_ref
    import octomap_ref
    w, h, B, step = 61, 47, 2, 3
    colors = [np.stack([TC.colour_image(w, h, 3, 5 * s + b) for b in range(B)]) for s in range(2)]
    depths = [np.stack([TC.depth_image(w, h, "u16", 7 * s + b)[0] for b in range(B)]) for s in range(2)]
    depths[0] = np.ascontiguousarray(depths[0][:, ::-1])       # (the stale scene is another scene)
    factor = 1.0 / 5000
    poses = [TC.pose(b) for b in range(B)]
    m = pkg.CloudMapper(0.1, step, 255)
    cap = m.capacity(w, h)
    refs = [cloud_ref.generate(colors[1][b], depths[1][b], TC.CAM["fx"], TC.CAM["fy"], TC.CAM["cx"], TC.CAM["cy"], poses[b], factor, step, 255) for b in range(B)]
    vox = [cloud_ref.voxel(r, np.float32(0.1)) for r in refs]
    assert all(0 < len(r) <= cap for r in refs) and all(n > 0 for _, n in vox)
    oref = octomap_ref.octomap(np.concatenate([np.stack([v["x"], v["y"], v["z"]], 1) for v, _ in vox]), octomap_ref.AXIS_SWAP, 0.1)
    S = caller_stream(torch, "cloud + voxel + octree")
    d_col, d_dep = torch.from_numpy(colors[0]).cuda(), torch.from_numpy(depths[0]).cuda()
    r_col, r_dep = torch.from_numpy(colors[1]).cuda(), torch.from_numpy(depths[1]).cuda()
    pts = torch.zeros((B, cap, 16), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    vpts = torch.zeros((B, cap, 16), dtype=torch.uint8, device="cuda")
    vcnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    data_cap, leaf_cap = oref["data_bytes"] + 4096, oref["leaves"] + 4096
    d_data = torch.zeros(data_cap, dtype=torch.uint8, device="cuda")
    d_leaf = torch.zeros(leaf_cap * 8, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(56, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def launch(s):
        m.generate_device(d_dep.data_ptr(), pkg.DEPTH_U16, w * 2, w * h * 2, factor, d_col.data_ptr(), 3, w * 3, w * h * 3, B, w, h,
                          TC.CAM["fx"], TC.CAM["fy"], TC.CAM["cx"], TC.CAM["cy"], np.stack(poses), pts.data_ptr(), cap, cnt.data_ptr(), s)
        m.voxel_device(pts.data_ptr(), cnt.data_ptr(), B, cap, vpts.data_ptr(), cap, vcnt.data_ptr(), s)
        m.octree_device(vpts.data_ptr(), vcnt.data_ptr(), B, cap, None, 0.1, d_data.data_ptr(), data_cap, d_leaf.data_ptr(), leaf_cap, d_info.data_ptr(), s)
    _, got = _consume(torch, S, [(d_col, r_col), (d_dep, r_dep)], launch, [pts, cnt, vpts, vcnt, d_data, d_leaf, d_info])
    g_pts, g_cnt, g_vpts, g_vcnt, g_data, g_leaf, g_info = got
    for b in range(B):
        assert g_cnt[b] == len(refs[b]) and cloud_ref.same_points(g_pts[b, :g_cnt[b]].reshape(-1).view(pkg.CLOUD_DTYPE), refs[b]), b
        assert g_vcnt[b] == vox[b][1] and cloud_ref.same_points(g_vpts[b, :g_vcnt[b]].reshape(-1).view(pkg.CLOUD_DTYPE), vox[b][0]), b
    info = pkg.OctreeInfo.from_buffer_copy(g_info.tobytes()).as_dict()
    for f in ("points_in", "points_dropped", "cells", "leaves", "tree_size", "data_bytes"):
        assert info[f] == oref[f], (f, info)
    assert info["overflow"] == 0 and g_data[:info["data_bytes"]].tobytes() == oref["data"]
    rows = g_leaf[:info["leaves"] * 8].view(pkg.OCTREE_LEAF_DTYPE)
    assert (np.stack([rows[f].astype(np.int64) for f in ("kx", "ky", "kz", "depth")], axis=1) == oref["leaf_rows"]).all()


def test_callers_stream_hamming_and_pack_records(pkg, torch, stall_ms):
    """orbm_hamming_matrix_device (numpy popcount) and orbx_pack_records_device (batching.pack_records on CPU tensors)."""
    batching = importlib.import_module(PKG + ".batching")
    rng = np.random.default_rng(3)
    na, nb, B, cap = 130, 257, 3, 37
    a = [rng.integers(0, 256, (na, 32), dtype=np.uint8) for _ in range(2)]
    b = [rng.integers(0, 256, (nb, 32), dtype=np.uint8) for _ in range(2)]
    g = torch.Generator().manual_seed(11)
    rec = [(torch.randn((B, cap, 7), generator=g), torch.randint(0, 256, (B, cap, 32), generator=g, dtype=torch.uint8), torch.randn((B, cap), generator=g),
            torch.randn((B, cap), generator=g), torch.randint(0, cap + 1, (B,), generator=g, dtype=torch.int32)) for _ in range(2)]
    want = batching.pack_records(*rec[1])
    S = caller_stream(torch, "hamming + pack")
    da, db = torch.from_numpy(a[0]).cuda(), torch.from_numpy(b[0]).cuda()
    ra, rb = torch.from_numpy(a[1]).cuda(), torch.from_numpy(b[1]).cuda()
    dist = torch.zeros((na, nb), dtype=torch.int16, device="cuda")
    d_rec, r_rec = [t.cuda() for t in rec[0]], [t.cuda() for t in rec[1]]
    packed = torch.zeros((B, batching.record_bytes(cap)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def launch(s):
        assert pkg.lib().orbm_hamming_matrix_device(da.data_ptr(), na, db.data_ptr(), nb, dist.data_ptr(), s) == 0
        pkg.pack_records_device(d_rec[0].data_ptr(), d_rec[1].data_ptr(), d_rec[2].data_ptr(), d_rec[3].data_ptr(), d_rec[4].data_ptr(), B, cap,
                                packed.data_ptr(), s)
    _, (g_dist, g_packed) = _consume(torch, S, [(da, ra), (db, rb)] + list(zip(d_rec, r_rec)), launch, [dist, packed])
    np.testing.assert_array_equal(g_dist.astype(np.int32), np.unpackbits(a[1][:, None, :] ^ b[1][None, :, :], axis=2).sum(2))
    np.testing.assert_array_equal(g_packed, want.numpy())


def test_callers_stream_search_by_projection_frame_and_pose(pkg, hooks, torch, synth, stall_ms):
    """orbm_search_by_projection_frame_device and orbo_pose_optimization_device return to the host but read device arrays the stream is
    still producing (tests/test_poseopt_gpu.py: test_device_form_equals_host_form - the device forms equal the host forms)."""
    import pose_scene as PS
    w, h = 752, 480
    left, right = synth.stereo_pair_blocky(w, h, 7)
    ex = pkg.ORBextractor(1000, PS.SCALE, PS.NLEVELS, 20, 7)
    cam = pkg.Camera(*PS.CAM)
    f = ex.stereo_frame(left, right, PS.BF, float(np.float32(PS.BF) / np.float32(PS.FX)))
    k, d, ur, depth = f["kl"], f["dl"], f["uright"], f["depth"]
    n = len(k)
    last = np.zeros(n, pkg.LASTPT_DTYPE)
    good = depth > 0
    fx, fy, cx, cy = (np.float32(c) for c in PS.CAM[:4])
    last["has_mp"] = good
    last["wx"] = np.where(good, (k["x"] - cx) * depth / fx, 0)
    last["wy"] = np.where(good, (k["y"] - cy) * depth / fy, 0)
    last["wz"] = np.where(good, depth, 0)
    last["observations"], last["octave"], last["angle"] = 2, k["octave"], k["angle"]
    I = np.eye(4, dtype=np.float32)
    geom, sf = pkg.grid_geom(w, h), ex.GetScaleFactors()
    want_nm, want_cur = pkg.ORBmatcher(0.9, True).SearchByProjectionFrame(k, d, ur, geom, sf, cam, I, I, last, d, np.full(n, -1, np.int32), None, 7.0, False)
    assert want_nm > 100
    S = caller_stream(torch, "search_by_projection_frame_device + pose_optimization_device")
    real = (k, d, ur)
    dst, src = _late_records(torch, real, [np.roll(a, 17, axis=0) for a in real])
    d_last = torch.from_numpy(d.copy()).cuda()
    torch.cuda.synchronize()

    def search():
        return pkg.search_by_projection_frame_device(dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), n, geom, sf, cam, I, I, last,
                                                     d_last.data_ptr(), np.full(n, -1, np.int32), None, 7.0, False, True, 0, S.cuda_stream)
    stale = search()
    assert stale[0] != want_nm or not np.array_equal(stale[1], want_cur)
    (nm, cur), ms = _behind_stall(torch, S, SS.STALL_MS, dst, src, search)
    assert nm == want_nm and np.array_equal(cur, want_cur)
    assert ms >= stall_ms[SS.STALL_MS], (ms, stall_ms)
    # the pose from the device arrays, late again
    pts = np.zeros(n, pkg.POSE_WORLDPOS_DTYPE)
    m = cur >= 0
    pts["valid"] = m
    for a in ("wx", "wy", "wz"):
        pts[a][m] = last[a][cur[m]]
    is2 = np.asarray(ex.GetInverseScaleSigmaSquares(), np.float32)
    guess = (PS.pose([0.004, -0.006, 0.003], [0.05, -0.03, 0.08]) @ np.eye(4)).astype(np.float32)
    obs = np.zeros(n, pkg.POSE_OBS_DTYPE)
    obs["valid"], obs["u"], obs["v"], obs["ur"], obs["inv_sigma2"] = pts["valid"], k["x"], k["y"], ur, is2[k["octave"]]
    obs["wx"], obs["wy"], obs["wz"] = pts["wx"], pts["wy"], pts["wz"]
    mark = np.where(m, 1, 3).astype(np.uint8)
    import test_poseopt_gpu as TP
    host = TP.as_bytes(pkg.pose_optimization(obs, cam, guess, outlier=mark))
    for a, b in zip(dst, [np.roll(x, 17, axis=0) for x in real]):
        a.copy_(torch.from_numpy(np.ascontiguousarray(b).view(np.uint8).reshape(-1).copy()))
    torch.cuda.synchronize()

    def pose():
        return TP.as_bytes(pkg.pose_optimization_device(dst[0].data_ptr(), dst[2].data_ptr(), n, is2, pts, cam, guess, outlier=mark, stream=S.cuda_stream))
    assert pose() != host
    got, ms = _behind_stall(torch, S, SS.STALL_MS, dst, src, pose)
    assert got == host
    assert ms >= stall_ms[SS.STALL_MS], (ms, stall_ms)
    ex.close()


def test_callers_stream_initialize(pkg, hooks, torch, stall_ms):
    """orbi_initialize_device on keypoint records that arrive behind the stall (tests/test_initializer_gpu.py: the device form equals the
    host form bit for bit)."""
    import init_scene as IS
    import test_initializer_gpu as TI
    sc = IS.case("general_150")
    host = TI.as_bytes(pkg.Initializer(sc["keys1"], sc["K4"], iterations=sc["iterations"]).initialize(sc["keys2"], sc["matches"], sc["sets"]))
    recs = []
    for k in (sc["keys1"], sc["keys2"]):
        kp = np.zeros(len(k), pkg.KP_DTYPE)
        kp["x"], kp["y"], kp["size"], kp["angle"], kp["octave"], kp["class_id"] = k[:, 0], k[:, 1], 31.0, 45.0, 1, -1
        recs.append(kp)
    S = caller_stream(torch, "initialize_device")
    dst, src = _late_records(torch, recs, [np.roll(r, 17, axis=0) for r in recs])
    torch.cuda.synchronize()

    def call():
        return TI.as_bytes(pkg.initialize_device(dst[0].data_ptr(), len(sc["keys1"]), dst[1].data_ptr(), len(sc["keys2"]), sc["matches"], sc["sets"], sc["K4"],
                                                 stream=S.cuda_stream))
    assert call() != host
    got, ms = _behind_stall(torch, S, SS.STALL_MS, dst, src, call)
    assert got == host
    assert ms >= stall_ms[SS.STALL_MS], (ms, stall_ms)


# ---------------------------------------------------------------------------------------------------------- pipeline.FrontEnd
FE_W, FE_H, FE_NF, FE_B = 320, 240, 300, 2


def _frontend_streams(fe, torch):
    s = [("main", fe.streams[0].cuda_stream)]
    if fe._hs is not None:
        s += [("side", fe._side_raw), ("hs.up", fe._hs.up.cuda_stream), ("hs.down", fe._hs.down.cuda_stream)]
    else:
        s.append(("side", fe._side_raw))
        if fe.side2 is not None:
            s.append(("side2", fe.side2.cuda_stream))
    return s


def _frontend_mismatches(ref, fe, results, exps, steps, nsets):
    bad = []
    B = fe.B
    for i in range(steps - fe.ring.nbuf, steps):
        imgs, frames = results(i)
        for b in range(B):
            e = exps[i % nsets][b]
            for side, k, d, gi in (("left", e["kl"], e["dl"], b), ("right", e["kr"], e["dr"], B + b)):
                m = ref.image_mismatch(imgs[gi][0], imgs[gi][1], k, d)
                if m:
                    bad.append("step %d frame %d %s: %s" % (i, b, side, m))
            m = ref.stereo_mismatch(frames[b], e)
            if m:
                bad.append("step %d frame %d stereo: %s" % (i, b, m))
    return bad


@pytest.mark.parametrize("mode", ["pipelined", "pipelined_late", "pipelined_late_fast_alone", "pipelined_late_two_side"])
def test_frontend_rotating_batches_with_one_stream_held_back_per_step(torch, pkg, ref, stall_ms, mode):
    """tests/test_bench_step_gpu.py: test_bench_step_rotating_batches with, before step i, one of the streams the mode owns held back
    (i modulo their number): main, side, side2.  Seven steps, no host wait; the last three against the oracle of their batch."""
    pl = importlib.import_module(PKG + ".pipeline")
    w, h, nf, B, steps, nsets = FE_W, FE_H, FE_NF, FE_B, 7, 3
    exps = stereo_sets(ref, w, h, nf, B, nsets, 4400)

    def arrange(attempt):
        fe = pl.FrontEnd(w, h, nf, True, B, prefetch=True, lag_stereo=True, stereo_late=mode.startswith("pipelined_late"),
                         two_side=mode.endswith("two_side"), fast_alone=mode.endswith("fast_alone"), mbf=MBF, fx=FX)
        s = _frontend_streams(fe, torch)
        return (fe, s), [(x, y, (nx, ny)) for nx, x in s for ny, y in s if nx != ny]
    fe, streams = SS.effective(arrange, "FrontEnd " + mode)
    fe.upload(np.stack([e["left"] for e in exps[0]]), np.stack([e["right"] for e in exps[0]]))
    for s in range(1, nsets):
        fe.upload_more(np.stack([e["left"] for e in exps[s]]), np.stack([e["right"] for e in exps[s]]))
    for i in range(steps):                   # once without a stall: every first-time allocation (and its host wait) is behind us
        fe.step(i)
    fe.drain()
    assert not _frontend_mismatches(ref, fe, lambda i: fe.results(i % fe.ring.nbuf), exps, steps, nsets)
    pending = []
    stalls = []
    for i in range(steps, 2 * steps):        # (the stalled pass counts its steps from 0: its last step holds the main stream back)
        name, raw = streams[(i - steps) % len(streams)]
        s = SS.stall(raw, SS.STALL_MS)
        fe.step(i)
        pending.append((i, name, s.pending()))
        stalls.append(s)
    fe.drain()
    bad = _frontend_mismatches(ref, fe, lambda i: fe.results(i % fe.ring.nbuf), exps, 2 * steps, nsets)
    assert all(p for _, _, p in pending), pending
    assert not bad, "\n".join(bad[:20])


def test_frontend_host_streaming_with_one_stream_held_back_per_step(torch, pkg, ref, stall_ms):
    """tests/test_bench_step_gpu.py: _host_streaming("pipelined") with one of main, side, hs.up, hs.down held back before every step."""
    pl = importlib.import_module(PKG + ".pipeline")
    w, h, nf, B, steps, nsets = FE_W, FE_H, FE_NF, FE_B, 8, 3
    exps = stereo_sets(ref, w, h, nf, B, nsets, 4400)

    def arrange(attempt):
        fe = pl.FrontEnd(w, h, nf, True, B, prefetch=True, lag_stereo=True, stereo_late=False, mbf=MBF, fx=FX)
        fe.upload(np.stack([e["left"] for e in exps[0]]), np.stack([e["right"] for e in exps[0]]))
        fe.enable_host_streaming()
        s = _frontend_streams(fe, torch)
        return (fe, s), [(x, y, (nx, ny)) for nx, x in s for ny, y in s if nx != ny]
    fe, streams = SS.effective(arrange, "FrontEnd host streaming")
    src = [(torch.from_numpy(np.stack([e["left"] for e in ex])).pin_memory(), torch.from_numpy(np.stack([e["right"] for e in ex])).pin_memory())
           for ex in exps]
    pending = []

    def run(i0, stalled):
        fe.submit(i0, *src[i0 % nsets])
        fe.submit(i0 + 1, *src[(i0 + 1) % nsets])
        for i in range(i0, i0 + steps):
            if stalled:
                name, raw = streams[(i - i0) % len(streams)]
                s = SS.stall(raw, SS.STALL_MS)
            fe.step(i)
            if stalled:
                pending.append((i, name, s.pending()))
            if i >= i0 + 1:
                fe.fetch(i - 1)
            if i + 2 < i0 + steps:
                fe.submit(i + 2, *src[(i + 2) % nsets])
        fe.fetch(i0 + steps - 1)
        return _frontend_mismatches(ref, fe, fe.host_results, exps, i0 + steps, nsets)
    assert not run(0, False)
    torch.cuda.synchronize()
    bad = run(steps, True)                   # (the rotation of batches, image buffers and result sets carries on)
    fe.drain()
    assert all(p for _, _, p in pending), pending
    assert not bad, "\n".join(bad[:20])
