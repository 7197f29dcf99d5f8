"""The timed path IS the tested path: exactly the step bench.py times (orb_slam2v2-1_amd/pipeline.py: ONE handle,
orbx_extract_batch_device on 2B images, orbm_stereo_batch_device(h, h, B, 0, B, ...)) against the CPU oracle, every
frame of the batch byte for byte — keypoints, descriptors, counts, mvuRight, mvDepth, match counts.

BASELINE configs covered here in their BATCHED form: 2 (KITTI 1241x376 stereo, 1000 and 2000 features), 3 (EuRoC 752x480
stereo, 64-frame batch), 4's per-GPU share (64 frames of 1920x1080 / 4000 features; the sharded two-rank form with the
all-gather: tests/test_multirank_gpu.py).  Reference: src/Frame.cc:61-120,
481-655; src/ORBextractor.cc:1043-1105."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PKG = "orb_slam2v2-1_amd"


def _pipeline():
    return importlib.import_module(PKG + ".pipeline")


def _ref():
    import oracle  # noqa: F401  (builds the checker)
    oracle.build()
    return importlib.import_module("oracle.reference_frames")


def _run_stereo(w, h, nf, B, seed0, streams=1, steps=1, fx=None, mbf=None):
    pl, ref = _pipeline(), _ref()
    kw = {}
    if fx is not None:
        kw = {"fx": fx, "mbf": mbf}
    fe = pl.FrontEnd(w, h, nf, True, B, streams=streams, **kw)
    exp = ref.run_pool(ref.stereo_frame, [(w, h, nf, seed0 + i, fe.mbf, fe.mb) for i in range(B)])
    fe.upload(np.stack([e["left"] for e in exp]), np.stack([e["right"] for e in exp]))
    bad = []
    for i in range(steps):
        j = fe.step(i)
    fe.drain()
    for i in range(max(0, steps - fe.ring.nbuf), steps):       # every buffer set still holding a step's results
        imgs, frames = fe.results(i % fe.ring.nbuf)
        for b in range(B):
            e = exp[b]
            for side, k, d, gi in (("left", e["kl"], e["dl"], b), ("right", e["kr"], e["dr"], B + b)):
                m = ref.image_mismatch(imgs[gi][0], imgs[gi][1], k, d)
                if m:
                    bad.append("step %d frame %d %s: %s" % (i, b, side, m))
            m = ref.stereo_mismatch(frames[b], e)
            if m:
                bad.append("step %d frame %d stereo: %s" % (i, b, m))
    assert not bad, "\n".join(bad[:20])
    return exp


@pytest.mark.parametrize("w,h,nf,B", [(1241, 376, 1000, 64), (1241, 376, 2000, 64), (752, 480, 1000, 64)],
                         ids=["kitti_1000feat_B64", "kitti_2000feat_B64", "euroc_B64"])
def test_bench_step_stereo_batch(w, h, nf, B):
    exp = _run_stereo(w, h, nf, B, seed0=0)
    assert sum(e["nmatch"] for e in exp) > 50 * B        # the matcher really matched (not a batch of empty frames)


def test_bench_step_three_handles_three_streams_one_thread():
    """INTEGRATION.md's multi-handle mode: three handles on three streams driven from ONE host thread, 20 interleaved
    steps with no join in between.  The stereo scratch lives in the left handle, so the steps cannot disturb each other;
    every result still resident at the end (the last three steps, one per handle) equals the oracle."""
    _run_stereo(1241, 376, 1000, 16, seed0=200, streams=3, steps=20)


@pytest.mark.parametrize("mode,w,h,nf,B,steps", [(m, 752, 480, 600, 6, 7) for m in ("pipelined", "pipelined_late", "pipelined_late_fast_alone", "pipelined_late_two_side",
                                                                                  "pyramid_ahead_only", "plain")] +
                         [("pipelined_late", 1241, 376, 1000, 40, 10)])   # bench-sized kernels: the matcher of step i-1 really runs beside FAST(i+1)
def test_bench_step_rotating_batches(mode, w, h, nf, B, steps):
    """The software-pipelined step (pyramid of step i+1 and stereo matcher of step i-1 on the side stream beside the tail of step
    i) over THREE different resident batches and the handle's TWO pyramid buffers, seven steps without a host synchronisation:
    a matcher or a FAST stage that read the wrong buffer, or read it too early / too late, would see another batch's pixels.
    Every result still resident at the end (steps 4, 5, 6 = batches 1, 2, 0) must equal the oracle of ITS batch."""
    pl, ref = _pipeline(), _ref()
    nsets = 3
    # pipelined_late (the default order since round 4): the pyramid of step i+1 is issued BEFORE the matcher of step i-1 on the side
    # stream (three pyramid buffers) and FAST(i+1) does not wait for that matcher; ..._fast_alone: it does (rounds 2-4); ..._two_side: the
    # matcher on a second side stream, both started behind FAST (measured alternative; implies fast_alone)
    fe = pl.FrontEnd(w, h, nf, True, B, prefetch=(mode != "plain"), lag_stereo=mode.startswith("pipelined"), stereo_late=mode.startswith("pipelined_late"),
                     two_side=mode.endswith("two_side"), fast_alone=mode.endswith("fast_alone"))
    assert fe.lag == mode.startswith("pipelined") and fe.late == mode.startswith("pipelined_late") and fe.two_side == mode.endswith("two_side")
    assert fe.fast_alone == (mode.endswith("fast_alone") or mode.endswith("two_side"))
    exps = [ref.run_pool(ref.stereo_frame, [(w, h, nf, 700 + 50 * s + i, fe.mbf, fe.mb) for i in range(B)]) for s in range(nsets)]
    fe.upload(np.stack([e["left"] for e in exps[0]]), np.stack([e["right"] for e in exps[0]]))
    for s in range(1, nsets):
        fe.upload_more(np.stack([e["left"] for e in exps[s]]), np.stack([e["right"] for e in exps[s]]))
    for i in range(steps):
        fe.step(i)
    fe.drain()
    bad = []
    for i in range(steps - fe.ring.nbuf, steps):
        exp = exps[i % nsets]
        imgs, frames = fe.results(i % fe.ring.nbuf)
        for b in range(B):
            e = exp[b]
            for side, k, d, gi in (("left", e["kl"], e["dl"], b), ("right", e["kr"], e["dr"], B + b)):
                m = ref.image_mismatch(imgs[gi][0], imgs[gi][1], k, d)
                if m:
                    bad.append("step %d frame %d %s: %s" % (i, b, side, m))
            m = ref.stereo_mismatch(frames[b], e)
            if m:
                bad.append("step %d frame %d stereo: %s" % (i, b, m))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("mode", ["pipelined", "pipelined_late", "pyramid_ahead_only", "plain"])
def test_host_streaming_rotating_batches(mode):
    _host_streaming(mode)


def test_host_streaming_last_fetch_waits_for_the_matcher_it_flushes():
    """The last step's matcher is still owed when its results are fetched: fetch issues it on the side stream, behind everything on
    the compute stream, and the download must wait for it, not only for the step's own kernels.  The compute stream is parked behind
    other work between the last step and its fetch, so a download that left early carries the stereo results the buffer set held
    three steps before.  TWO batches rotate through the THREE buffer sets here, so those are the other batch's (with three batches
    a buffer set always meets the same batch again, and only a download torn by the running matcher would show)."""
    _host_streaming("pipelined", park_before_last_fetch=True, nsets=2)


def _host_streaming(mode, park_before_last_fetch=False, nsets=3):
    """End to end from host memory (FrontEnd.enable_host_streaming): THREE different batches in pinned host memory arrive by
    asynchronous copies on an upload stream into three image buffers while other batches compute, results leave on a download
    stream; eight steps without a host synchronisation until the last results are waited for.  Every result still in the pinned
    host arrays at the end (steps 5, 6, 7) must equal the oracle of ITS batch: an upload that overtook the pyramid still reading
    its buffer, a pyramid built ahead of its upload, or a download that left before the (lagged) matcher would show."""
    import torch
    pl, ref = _pipeline(), _ref()
    w, h, nf, B, steps = 752, 480, 600, 6, 8
    fe = pl.FrontEnd(w, h, nf, True, B, prefetch=(mode != "plain"), lag_stereo=mode.startswith("pipelined"), stereo_late=(mode == "pipelined_late"))
    exps = [ref.run_pool(ref.stereo_frame, [(w, h, nf, 1700 + 50 * s + i, fe.mbf, fe.mb) for i in range(B)]) for s in range(nsets)]
    fe.upload(np.stack([e["left"] for e in exps[0]]), np.stack([e["right"] for e in exps[0]]))
    fe.enable_host_streaming()
    src = [(torch.from_numpy(np.stack([e["left"] for e in ex])).pin_memory(), torch.from_numpy(np.stack([e["right"] for e in ex])).pin_memory())
           for ex in exps]
    x = torch.randn((4096, 4096), device="cuda")
    for _ in range(4):                     # park the compute stream: everything below is queued before the first kernel runs
        x = (x @ x) * 1e-4
    fe.submit(0, *src[0])
    fe.submit(1, *src[1])
    for i in range(steps):
        fe.step(i)
        if i >= 1:
            fe.fetch(i - 1)
        if i + 2 < steps:
            fe.submit(i + 2, *src[(i + 2) % nsets])
    if park_before_last_fetch:
        for _ in range(4):
            x = (x @ x) * 1e-4
    fe.fetch(steps - 1)
    bad = []
    for i in range(steps - fe.ring.nbuf, steps):
        exp = exps[i % nsets]
        imgs, frames = fe.host_results(i)
        for b in range(B):
            e = exp[b]
            for side, k, d, gi in (("left", e["kl"], e["dl"], b), ("right", e["kr"], e["dr"], B + b)):
                m = ref.image_mismatch(imgs[gi][0], imgs[gi][1], k, d)
                if m:
                    bad.append("step %d frame %d %s: %s" % (i, b, side, m))
            m = ref.stereo_mismatch(frames[b], e)
            if m:
                bad.append("step %d frame %d stereo: %s" % (i, b, m))
    fe.drain()
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("chunks", [2, 3, 4])
def test_batch_chunking_does_not_change_results(chunks):
    """Developer knob 8 cuts a batch into chunks whose kernels overlap on the handle's side streams (measured slower than one
    chunk, so off by default): per-image results must not depend on it, uneven chunk sizes included (26 images in 3 or 4
    chunks), and the stereo matcher behind it must see finished arrays."""
    pkg = importlib.import_module(PKG)
    pkg.set_default_option(8, chunks)
    try:
        _run_stereo(752, 480, 700, 13, seed0=400, steps=3)
    finally:
        pkg.set_default_option(8, 0)


def test_pyramid_built_ahead_is_used_only_for_the_same_batch():
    """orbx_extract_batch_device_prefetch: the step above always builds the next step's pyramid ahead (FrontEnd.prefetch).
    Here the edges: a pyramid built ahead for batch X must be ignored by a call on batch Y, used by a call on X (same
    bytes out as without it, mvImagePyramid included), and a second prefetch replaces the first."""
    import torch
    pkg = importlib.import_module(PKG)
    ref = _ref()
    w, h, nf, B = 640, 480, 600, 3
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7)
    sets = []
    for s in (0, 1, 2):
        exp = ref.run_pool(ref.mono_frame, [(w, h, nf, 900 + 10 * s + i) for i in range(B)])
        sets.append((exp, torch.from_numpy(np.stack([e["img"] for e in exp])).cuda()))
    ex(sets[0][0][0]["img"])
    cap = ex.max_keypoints()
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run(which):
        d = sets[which][1]
        ex.extract_batch_device(d.data_ptr(), B, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)
        torch.cuda.synchronize()
        k = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
        for b in range(B):
            n = int(cnt[b])
            got = np.frombuffer(k[b, :n].tobytes(), pkg.KP_DTYPE)
            m = ref.image_mismatch(got, desc[b, :n].cpu().numpy(), sets[which][0][b]["k"], sets[which][0][b]["d"])
            assert m is None, (which, b, m)
        return [ex.pyramid_level(l, 1).copy() for l in (0, 3, 7)]

    def pre(which):
        ex.prefetch_batch_device(sets[which][1].data_ptr(), B, w, h, w, w * h)

    plain = [run(0), run(1)]
    pre(0)
    for a, b_ in zip(run(0), plain[0]):          # used
        assert np.array_equal(a, b_)
    pre(0)
    for a, b_ in zip(run(1), plain[1]):          # built for batch 0, call on batch 1: ignored
        assert np.array_equal(a, b_)
    pre(0)
    pre(1)                                       # replaced
    for a, b_ in zip(run(1), plain[1]):
        assert np.array_equal(a, b_)
    for a, b_ in zip(run(0), plain[0]):          # nothing pending any more
        assert np.array_equal(a, b_)
    # Ordering by events alone: park the stream behind ~50 ms of other work so that all six calls below are issued before the
    # first one runs; three image sets against two pyramid buffers, so a pyramid written too early (before the FAST stage of
    # the call in front has finished with the buffer's previous contents) shows as another set's key points.
    outs = [(torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda"), torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda"),
             torch.zeros(B, dtype=torch.int32, device="cuda")) for _ in range(6)]
    x = torch.randn((8192, 8192), device="cuda")
    torch.cuda.synchronize()
    for _ in range(6):
        x = (x @ x) * 1e-4
    for i in range(6):
        w3 = i % 3
        pre(w3)
        d = sets[w3][1]
        ex.extract_batch_device(d.data_ptr(), B, w, h, w, w * h, outs[i][0].data_ptr(), outs[i][1].data_ptr(), outs[i][2].data_ptr(), cap, st)
    torch.cuda.synchronize()
    for i in range(6):
        k = outs[i][0].cpu().numpy().view(np.uint8).reshape(B, cap, 28)
        for b in range(B):
            n = int(outs[i][2][b])
            got = np.frombuffer(k[b, :n].tobytes(), pkg.KP_DTYPE)
            m = ref.image_mismatch(got, outs[i][1][b, :n].cpu().numpy(), sets[i % 3][0][b]["k"], sets[i % 3][0][b]["d"])
            assert m is None, (i, b, m)


def test_bench_step_mono_full_hd_batch64():
    """BASELINE config 4's per-GPU share as written (512 frames over 8 GPUs): 64 frames of 1920x1080, 4000 features per batched call,
    five pipelined steps over TWO rotating batches, every frame of the three result sets still resident against the oracle of ITS batch.
    At this size the quad-tree launch fills the GPU twice, so FrontEnd starts the pyramid built ahead together with FAST
    (ORBX_OPT_PREFETCH_GATE = 3): a pyramid that overwrote a buffer FAST still reads would show as another batch's pixels."""
    pl, ref = _pipeline(), _ref()
    w, h, nf, B, nsets, steps = 1920, 1080, 4000, 64, 2, 5
    exps = [ref.run_pool(ref.mono_frame, [(w, h, nf, 300 + 100 * s + i) for i in range(B)]) for s in range(nsets)]
    fe = pl.FrontEnd(w, h, nf, False, B)
    assert fe.ex.get_option(10) == 3
    fe.upload(np.stack([e["img"] for e in exps[0]]))
    fe.upload_more(np.stack([e["img"] for e in exps[1]]))
    for i in range(steps):
        fe.step(i)
    fe.drain()
    bad = []
    for i in range(steps - fe.ring.nbuf, steps):
        imgs, _ = fe.results(i % fe.ring.nbuf)
        exp = exps[i % nsets]
        for b in range(B):
            m = ref.image_mismatch(imgs[b][0], imgs[b][1], exp[b]["k"], exp[b]["d"])
            if m:
                bad.append("step %d frame %d: %s" % (i, b, m))
    assert not bad, "\n".join(bad[:20])
    assert min(len(e["k"]) for e in exps[0]) > 3800


@pytest.mark.parametrize("gate", [0, 1, 2, 3])
def test_prefetch_gate_does_not_change_results(gate, pkg):
    """ORBX_OPT_PREFETCH_GATE: the pyramid built ahead behind FAST (default), behind the quad-tree, behind the descriptors or together
    with FAST - seven pipelined mono steps over three rotating batches, results of the last three against the oracle of their batch."""
    pl, ref = _pipeline(), _ref()
    w, h, nf, B, nsets, steps = 752, 480, 800, 12, 3, 7
    exps = [ref.run_pool(ref.mono_frame, [(w, h, nf, 900 + 40 * s + i) for i in range(B)]) for s in range(nsets)]
    pkg.set_default_option(10, gate)
    try:
        fe = pl.FrontEnd(w, h, nf, False, B)
        assert fe.ex.get_option(10) == gate
        fe.upload(np.stack([e["img"] for e in exps[0]]))
        for s in range(1, nsets):
            fe.upload_more(np.stack([e["img"] for e in exps[s]]))
        for i in range(steps):
            fe.step(i)
        fe.drain()
    finally:
        pkg.set_default_option(10, 0)
    for i in range(steps - fe.ring.nbuf, steps):
        imgs, _ = fe.results(i % fe.ring.nbuf)
        for b in range(B):
            e = exps[i % nsets][b]
            assert ref.image_mismatch(imgs[b][0], imgs[b][1], e["k"], e["d"]) is None, (i, b)


def test_stereo_scratch_regrows_and_large_cap():
    """The per-handle stereo scratch grows with (B, cap); a cap above the LDS plan of k_stereo_median (12288) takes the
    global-memory form of the median kernel - results identical to the small-cap call on the same frame."""
    import torch
    pkg = importlib.import_module(PKG)
    ref = _ref()
    w, h, nf = 752, 480, 800
    e = ref.stereo_frame((w, h, nf, 77, 47.9, float(np.float32(47.9) / np.float32(435.2))))
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7)
    imgs = np.stack([e["left"], e["right"]])
    ex(imgs[0])
    d_imgs = torch.from_numpy(imgs).cuda()
    out = []
    for cap in (ex.max_keypoints(), 20000):
        kps = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda")
        desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        ur = torch.zeros((1, cap), dtype=torch.float32, device="cuda")
        dp = torch.zeros((1, cap), dtype=torch.float32, device="cuda")
        nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        ex.extract_batch_device(d_imgs.data_ptr(), 2, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)
        pkg.stereo_batch_device(ex, ex, 1, 0, 1, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), kps[1:].data_ptr(),
                                desc[1:].data_ptr(), cnt[1:].data_ptr(), cap, 47.9, float(np.float32(47.9) / np.float32(435.2)),
                                ur.data_ptr(), dp.data_ptr(), nm.data_ptr(), st)
        torch.cuda.synchronize()
        n = int(cnt[0])
        out.append((ur[0, :n].cpu().numpy(), dp[0, :n].cpu().numpy(), int(nm[0])))
    for got in out:
        assert ref.stereo_mismatch(got, e) is None, ref.stereo_mismatch(got, e)
