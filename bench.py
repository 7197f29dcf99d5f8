#!/usr/bin/env python3
"""bench.py — ORB extract+match throughput on MI355X (the BASELINE.json metric).

One step = one pass of the hot path over one batch of synthetic STEREO frames that are
already resident in HBM: ORB extraction of the left and right 1241x376 images (8 levels,
1000 features per image) + Frame::ComputeStereoMatches.  A "frame" is one stereo frame (two
images), the conservative reading of "frames/s ORB extract+match".  Each rank (one process per
GPU) owns its own frames (weak scaling); with N > 1 every step's results (left keypoints,
descriptors, counts, mvuRight, mvDepth) are all-gathered over RCCL/xGMI, overlapped with the
next step's compute.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement").  A plain run sets up, warms up, times the K steps and prints the
headline; --full adds the CPU baseline, the other workloads, the oracle checks and the per-stage / roofline / end-to-end /
tracking blocks.  --dump-outputs DIR writes what the last timed step computed as .npy files.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (w, h, nfeatures, stereo)
    "kitti_stereo_1241x376_1000feat": (1241, 376, 1000, True),
    "kitti_stereo_1241x376_2000feat": (1241, 376, 2000, True),
    "euroc_stereo_752x480_1000feat": (752, 480, 1000, True),
    "mono_1241x376_1000feat": (1241, 376, 1000, False),
    "mono_640x480_1000feat": (640, 480, 1000, False),
    "mono_1920x1080_4000feat": (1920, 1080, 4000, False),
    # corner-SPARSE scenes (synth.natural_pair: 2-5 % of the pixels are FAST corners at t = 7, the regime of real footage; the
    # frames SURVEY section 8(d) prescribes are corner-saturated, 33-53 %)
    "kitti_stereo_natural_1241x376_1000feat": (1241, 376, 1000, True),
}
NATURAL = {"kitti_stereo_natural_1241x376_1000feat"}
# the other north-star sizes measured (briefly) after the headline: (workload, frames per step).  1920x1080: 64 frames = one GPU's share of BASELINE
# config 4 (a 512-frame batch over 8 GPUs; rounds 1-5 measured 32 here)
OTHER_WORKLOADS = [("kitti_stereo_1241x376_2000feat", 64), ("euroc_stereo_752x480_1000feat", 64), ("mono_640x480_1000feat", 64),
                   ("mono_1920x1080_4000feat", 64), ("kitti_stereo_natural_1241x376_1000feat", 64)]
KITTI_FX, KITTI_BF = 718.856, 386.1448  # KITTI-00 calibration (fx, baseline*fx); same constants as pipeline.py


def level_pixels(w, h, nlevels=8, sf=1.2):
    """P = sum of inner level pixels (reference: src/ORBextractor.cc:1111-1112)."""
    s = np.float32(1.0)
    tot = 0
    for l in range(nlevels):
        inv = np.float32(1.0) / s
        tot += int(np.rint(np.float32(w) * inv)) * int(np.rint(np.float32(h) * inv))
        s = np.float32(s * np.float32(sf))
    return tot


def _gen_pair(args):
    w, h, k, stereo, kind = args
    synth = importlib.import_module("orb_slam2v2-1_amd.synth")
    if kind == "natural":
        return synth.natural_pair(w, h, k) if stereo else (synth.natural(w, h, k), None)
    if stereo:
        l, r = synth.stereo_pair_blocky(w, h, k)
        return l, r
    return synth.frame(w, h, k), None


def _pool_map(fn, jobs, workers):
    """fn over jobs on a SPAWN pool whose workers exit by themselves (close + join, never terminate): a forked worker inherits
    whatever the parent has loaded - under rocprofv3 the tool library with its signal handlers, and the pool's SIGTERM at teardown
    then aborted the workers (gpurun_out/r02_bench3.err)."""
    import multiprocessing as mp
    pool = mp.get_context("spawn").Pool(workers)
    try:
        out = pool.map(fn, jobs)
    finally:
        pool.close()
        pool.join()
    return out


def make_frames(w, h, n, k0, stereo, workers, kind="dense"):
    jobs = [(w, h, k0 + i, stereo, kind) for i in range(n)]
    if workers > 1 and n > 2:
        out = _pool_map(_gen_pair, jobs, min(workers, n))
    else:
        out = [_gen_pair(j) for j in jobs]
    left = np.stack([o[0] for o in out])
    right = np.stack([o[1] for o in out]) if stereo else None
    return left, right


def _cpu_frame(args):
    """CPU baseline worker: the ORACLE (restated CPU path) on one frame."""
    w, h, nf, k, stereo = args
    import oracle
    synth = importlib.import_module("orb_slam2v2-1_amd.synth")
    t0 = time.perf_counter()
    if stereo:
        l, r = synth.stereo_pair_blocky(w, h, k)
    else:
        l, r = synth.frame(w, h, k), None
    tgen = time.perf_counter() - t0
    t0 = time.perf_counter()
    exl = oracle.Extractor(nf, 1.2, 8, 20, 7)
    kl, dl = exl.extract(l)
    stages = exl.stage_seconds.copy()
    if stereo:
        exr = oracle.Extractor(nf, 1.2, 8, 20, 7)
        kr, dr = exr.extract(r)
        stages += exr.stage_seconds
        pl = [exl.pyramid_level(i) for i in range(8)]
        pr = [exr.pyramid_level(i) for i in range(8)]
        mb = np.float32(KITTI_BF) / np.float32(KITTI_FX)
        oracle.stereo_match(kl, dl, kr, dr, pl, pr, exl.scale_factors, exl.inv_scale_factors, KITTI_BF, mb)
    return time.perf_counter() - t0, tgen, stages


def _cpu_warm(i):
    """Brings a pool worker up: imports + one tiny oracle call."""
    import oracle
    oracle.Extractor(100, 1.2, 4, 20, 7).extract(np.zeros((120, 160), np.uint8))
    return i


def cpu_baseline(w, h, nf, stereo, budget_s=20.0):
    """Times the oracle on the host cores over a bounded sample of the same workload."""
    import oracle
    oracle.build()
    cores = max(1, min(os.cpu_count() or 1, 16))
    t1, _, _ = _cpu_frame((w, h, nf, 0, stereo))  # one frame, one core: sizes the sample
    nframes = int(max(cores, min(8 * cores, budget_s * cores / max(t1, 1e-3))))
    jobs = [(w, h, nf, 100 + i, stereo) for i in range(nframes)]
    t0 = time.perf_counter()
    res = _pool_map(_cpu_frame, jobs, cores)
    wall = time.perf_counter() - t0
    gen = sum(r[1] for r in res)
    work = sum(r[0] for r in res)
    # frame generation happens inside the workers too; remove its share of the wall time
    wall_work = wall * work / max(work + gen, 1e-9)
    st = np.sum([r[2] for r in res], 0)
    # (i) one thread, mono extract; (ii) two threads, stereo extract + ComputeStereoMatches, the way
    # the reference runs its two extractors (src/Frame.cc:78-81; ctypes releases the GIL during the oracle calls)
    import threading
    synth = importlib.import_module("orb_slam2v2-1_amd.synth")
    one_thread_mono = two_thread_stereo = None
    try:
        reps = 3
        img = synth.frame(w, h, 7)
        e1 = oracle.Extractor(nf, 1.2, 8, 20, 7)
        t0 = time.perf_counter()
        for _ in range(reps):
            e1.extract(img)
        one_thread_mono = reps / (time.perf_counter() - t0)
        if stereo:
            l, r = synth.stereo_pair_blocky(w, h, 7)
            exs = [oracle.Extractor(nf, 1.2, 8, 20, 7) for _ in range(2)]
            out = [None, None]

            def _work(i, im):
                out[i] = exs[i].extract(im)
            mb = np.float32(KITTI_BF) / np.float32(KITTI_FX)
            t0 = time.perf_counter()
            for _ in range(reps):
                ts = [threading.Thread(target=_work, args=(i, im)) for i, im in enumerate((l, r))]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                oracle.stereo_match(out[0][0], out[0][1], out[1][0], out[1][1], [exs[0].pyramid_level(i) for i in range(8)],
                                    [exs[1].pyramid_level(i) for i in range(8)], exs[0].scale_factors, exs[0].inv_scale_factors,
                                    KITTI_BF, mb)
            two_thread_stereo = reps / (time.perf_counter() - t0)
    except Exception:
        pass
    # every visible core, one frame per process at a time (bounded: two frames per process).  The pool is
    # brought up (spawn + imports) by an untimed first map, so the figure is the oracle's, not the interpreter's start-up.
    all_cores = None
    try:
        import multiprocessing as mp
        ncpu = max(1, min(os.cpu_count() or 1, 512))
        quota = None
        try:   # a container's CPU quota caps what any number of processes can use (the GPU boxes show 256 cores behind a quota of 16:
            # 256 processes then ran SLOWER than 16 - 63.7 against 84.1 frames/s - and the throttled host enqueued the timed steps late)
            q = open("/sys/fs/cgroup/cpu.max").read().split()
            quota = None if q[0] == "max" else float(q[0]) / float(q[1])
        except (OSError, ValueError, IndexError):
            pass
        if quota is not None:
            ncpu = max(1, min(ncpu, int(quota + 0.5)))
        if ncpu > cores:
            pool = mp.get_context("spawn").Pool(ncpu)
            try:
                pool.map(_cpu_warm, range(ncpu), chunksize=1)
                jobs2 = [(w, h, nf, 300 + i, stereo) for i in range(2 * ncpu)]
                t0 = time.perf_counter()
                res2 = pool.map(_cpu_frame, jobs2, chunksize=1)
                wall2 = time.perf_counter() - t0
            finally:
                pool.close()
                pool.join()
            work2, gen2 = sum(r[0] for r in res2), sum(r[1] for r in res2)
            all_cores = {"value": round(len(jobs2) / (wall2 * work2 / max(work2 + gen2, 1e-9)), 2), "unit": "frames/s", "processes": ncpu,
                         "frames": len(jobs2), "cgroup_cpu_quota_cores": quota,
                         "host_cores_visible": os.cpu_count(),
                         "parallel_efficiency": round(work2 / max(wall2 * ncpu, 1e-9), 3),
                         "note": "same oracle, one process per visible core, two frames each; parallel_efficiency = busy time / (wall x "
                                 "processes): well below 1 means the container's CPU quota (or memory bandwidth), not the core count, sets the rate"}
        else:
            all_cores = {"value": round(nframes / wall_work, 3), "unit": "frames/s", "processes": cores, "frames": nframes,
                         "cgroup_cpu_quota_cores": quota, "host_cores_visible": os.cpu_count(),
                         "note": "the bounded sample above already uses every core this container may use (visible cores capped by the "
                                 "cgroup CPU quota)"}
    except Exception as e:      # informational block: never takes the line with it
        all_cores = {"error": repr(e)}
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {
        "value": round(nframes / wall_work, 3), "unit": "frames/s", "cores": cores, "kind": "port",
        "sample": "%d synthetic %s frames %dx%d, %d features, CPU oracle (restated CPU path, gcc -O3 -march=native, "
                  "scalar FAST) on %d processes; single-core %.3f s/frame" % (
                      nframes, "stereo" if stereo else "mono", w, h, nf, cores, t1),
        "stage_share": {k: round(float(v / max(st.sum(), 1e-9)), 3) for k, v in
                        zip(["pyramid", "fast", "quadtree", "orientation", "blur", "descriptor"], st)},
        "cpu_model": model, "host_cores_visible": os.cpu_count(), "all_cores": all_cores,
        "all_cores_frames_per_s": None if not all_cores or "value" not in all_cores else all_cores["value"],
        "one_thread_mono_images_per_s": None if one_thread_mono is None else round(one_thread_mono, 2),
        "two_thread_stereo_frames_per_s": None if two_thread_stereo is None else round(two_thread_stereo, 2),
    }


def measure(fe, steps, warmup, ramp, world, dist, dev, torch, full=True):
    """Ramp + warm-up + K timed steps of fe (barrier + synchronize on both sides, MAX over ranks); full = True adds the FAST-stage
    events inside the timed region, the long_run pass and an untimed stage-profile pass.  Returns dict(dt, fast_ms, stage_ms, ncalls,
    match_ms, last_results); without `full` only dt and last are filled."""
    ex = fe.ex
    # clock ramp (untimed, not counted as warm-up steps): at least `ramp` steps AND at least half a second of GPU load - a box that
    # sat idle needs that long before the clocks hold (one fresh box in a dozen measured 9 % low behind a 0.13-s ramp)
    t_ramp, i = time.perf_counter(), 0
    while ramp > 0 and (i < ramp or time.perf_counter() - t_ramp < 0.5):
        fe.step(i)
        i += 1
        if i % 50 == 0:
            fe.drain()                  # keeps the clock comparison about executed, not merely enqueued, steps
    fe.drain()
    for i in range(warmup):
        fe.step(i)
    fe.drain()
    # Timed region: only the dominant kernel (the FAST stage: k_fast_strips) is bracketed by HIP events on its launch stream.  Every
    # recorded event idles the GPU for ~4.5 us, so the full stage breakdown is taken in a separate untimed pass below.
    if full:
        ex.set_profiling(3)     # the FAST stage of every 4th timed step (two events idle the GPU for ~9 us)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fe.step(warmup + i)
    fe.drain()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if not full:                                    # a plain run: the outputs of the last timed step, nothing else
        return {"dt": dt, "fast_ms": None, "stage_ms": None, "ncalls": None, "match_ms": None,
                "last": fe.results((warmup + steps - 1) % fe.ring.nbuf), "nprof": 0, "gathered": None, "long_run": None}
    fast_ms = float(ex.stage_ms()[0][1])            # FAST stage, averaged over the K timed steps
    # a short K (the driver's command: 20 steps = 13 ms) is one sample of a noisy quantity: the same loop once more over >= 100 steps,
    # reported beside `value` as `long_run` (never as `value`: the contract times exactly K steps)
    long_run = None
    if steps < 100 and world == 1:
        kk = 100
        ex.set_profiling(0)
        for i in range(kk // 5):
            fe.step(i)
        fe.drain()
        torch.cuda.synchronize()
        tl = time.perf_counter()
        for i in range(kk):
            fe.step(i)
        fe.drain()
        torch.cuda.synchronize()
        long_run = (kk, time.perf_counter() - tl)
        for i in range(warmup + steps - fe.ring.nbuf, warmup + steps):   # the buffer sets hold the last timed steps' results again
            fe.step(i)
        fe.drain()
    last = fe.results((warmup + steps - 1) % fe.ring.nbuf)   # outputs of the LAST TIMED step (host copies), checked later
    gath = None
    if fe.ring.gather:                              # ... and what the all-gather of that step delivered (every rank's records)
        jl = (warmup + steps - 1) % fe.ring.nbuf
        gath = (jl, warmup + steps - 1, fe.ring.gathered_steps[jl], {k: v.clone() for k, v in fe.ring.gathered(jl).items()})
    nprof = max(1, min(steps, 10))                  # untimed pass: events at every stage boundary
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(nprof)]
    ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(nprof)]
    pf, fe.prefetch = fe.prefetch, False            # stage events need the stages one after the other: no pyramid built ahead here
    fe.step(warmup + steps)                         # (this call still takes the pyramid the last timed step started)
    fe.drain()
    ex.set_profiling(1)
    for i in range(nprof):
        fe.step(warmup + steps + i, ev0[i], ev1[i])
    fe.drain()
    stage_ms, ncalls = ex.stage_ms()
    ex.set_profiling(0)
    fe.prefetch = pf
    match_ms = float(np.mean([a.elapsed_time(b) for a, b in zip(ev0, ev1)])) if fe.stereo else 0.0
    return {"dt": dt, "fast_ms": fast_ms, "stage_ms": stage_ms, "ncalls": ncalls, "match_ms": match_ms, "last": last,
            "nprof": nprof, "gathered": gath, "long_run": long_run}


def measure_gather_leg(fe, torch, n=200):
    """Cost of the communication leg of ONE step, alone on the GPU (--force-gather): the pack kernel (B frame records of fixed capacity)
    and the all-gather of them, issued exactly as the pipelined step issues them (pack on the side stream, collective from the
    front end's collective stream, async work handle waited for when the buffer set comes round again), n times back to back."""
    r = fe.ring
    fe.drain()
    side = fe.side if fe.side is not None else torch.cuda.current_stream(fe.dev)
    def leg(k):
        for i in range(k):
            j = r.acquire(i)
            if fe.lag:
                fe._publish_side(j, None, side)
            else:
                r.publish(j, None)
        r.drain()
        torch.cuda.synchronize(fe.dev)
    leg(20)
    t0 = time.perf_counter()
    leg(n)
    dt = (time.perf_counter() - t0) / n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        for i in range(n):
            r.pack_set(i % r.nbuf)
        e1.record(side)
    torch.cuda.synchronize(fe.dev)
    rb = r.pack[0].shape[1]
    return {"ms_per_step_alone": round(dt * 1e3, 4), "pack_kernel_ms": round(e0.elapsed_time(e1) / n, 4), "record_bytes_per_frame": int(rb),
            "bytes_per_step_per_rank": int(rb * r.gB), "ranks": r.world,
            "note": "pack + all_gather_into_tensor(async_op=True) + work.wait(), %d times back to back with nothing else on the GPU: the upper "
                    "bound of what the leg adds to a step (in the timed steps it runs beside the next step's kernels); a ONE-rank communicator "
                    "moves the records inside one GPU - no xGMI traffic, no scaling figure" % n}


def measure_end_to_end(fe, left, right, steps, warmup, torch):
    """The same step fed from PINNED HOST memory and delivering to pinned host memory (FrontEnd.enable_host_streaming): uploads of
    batch i + 2 and downloads of batch i - 1 on their own streams beside the kernels of batches i, i + 1.  Times K steps from the
    first upload to the arrival of the last result on the host.  Returns (seconds, host copies of the last step's results)."""
    fe.drain()
    fe.enable_host_streaming()
    pl = torch.from_numpy(np.ascontiguousarray(left)).pin_memory()
    pr = torch.from_numpy(np.ascontiguousarray(right)).pin_memory() if right is not None else None

    def run(K):
        fe.submit(0, pl, pr)
        if K > 1:
            fe.submit(1, pl, pr)
        for i in range(K):
            fe.step(i)
            if i >= 1:
                fe.fetch(i - 1)
            if i >= 3:
                fe.wait(i - 3)      # the consumer takes each result as it lands: the host stays three steps ahead of the results
            if i + 2 < K:           # (with everything enqueued unboundedly far ahead the same loop measured 1.36-2.0 ms per step)
                fe.submit(i + 2, pl, pr)
        fe.fetch(K - 1)
        fe.wait(K - 1)
    # link ramp (untimed): the first ~100 steps of host streaming run 15-20 % slower than the following ones whatever ran before on
    # the GPU (tools/e2e_variants.py: 1.33-1.36 ms per step in the first 100-step run, 1.14-1.16 in the next two) - the copy path
    # needs its own warm-up, as the clocks do
    run(max(warmup, 3))
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < 0.3:
        run(50)
    fe.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    last = fe.host_results(steps - 1)
    fe.drain()
    return dt, last


def tracking_front_end(nframes=16):
    """BASELINE config 5's SHAPE without its dataset, optimiser and back-end (KITTI-00 and a vocabulary are not in the image): the
    front-end of Tracking::Track in localisation mode chained over a synthetic 1241x376 stereo sequence, 2000 features per camera -
    Frame(stereo), SearchByProjection(cur, last), SearchLocalPoints, key frames - with the state carried from frame to frame
    (tests/tracking_chain.py).  Latency per frame of the device-resident chain, and the whole chain compared snapshot by snapshot with
    the same chain on the CPU oracle (checker leg).  Replicas only: frame t needs frame t-1."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    tc = importlib.import_module("tracking_chain")
    synth = importlib.import_module("orb_slam2v2-1_amd.synth")
    w, h, nf, step = 1241, 376, 2000, 0.04
    frames, _ = synth.stereo_sequence(w, h, nframes, k=11, step=step)
    Ts = tc.poses(nframes, step)
    dev = tc.Chain(tc.GpuViewBackend(w, h, nf), w, h, nf)       # the latency path: orbx_stereo_frame_view + device-resident matchers
    src = [(torch.from_numpy(l).pin_memory(), torch.from_numpy(r).pin_memory()) for l, r in frames]
    for t in range(nframes):
        dev.step(src[t][0], src[t][1], Ts[t])
    orc = tc.Chain(tc.OracleBackend(w, h, nf), w, h, nf)
    for t in range(nframes):
        orc.step(frames[t][0], frames[t][1], Ts[t])
    diff = tc.first_difference(orc.log, dev.log)
    log = dev.log[4:]
    med = lambda key: 1e3 * float(np.median([s[key] for s in log]))
    tot = med("t_frame") + med("t_proj") + med("t_local")
    return {"value": round(1e3 / tot, 1), "unit": "frames/s (one frame at a time)", "ms_per_frame": round(tot, 4),
            "ms_frame_extract_stereo": round(med("t_frame"), 4), "ms_search_by_projection": round(med("t_proj"), 4),
            "ms_search_local_points": round(med("t_local"), 4), "frames": nframes,
            "projection_matches_median": int(np.median([s["proj_n"] for s in log])),
            "verified": diff is None, "verified_note": ("every snapshot of %d chained frames (keypoints, descriptors, mvuRight, mvDepth, projection holders, "
                                                        "frustum records, local-map holders, map) == the same chain on the CPU oracle" % nframes)
            if diff is None else "chains diverge at frame %d, field %s" % diff,
            "entry_points": "orbx_stereo_frame_view (images in pinned host memory, record written to pinned host memory by the last kernel; no copy "
                            "command) + orbm_search_by_projection_frame_device + orbm_search_local_points_device",
            "note": "config 5's shape on a synthetic sequence: no KITTI-00, no vocabulary, no optimiser (poses are the true ones); not ATE"}


def verify_against_oracle(fe, last, seeds, frames, kind="dense"):
    """Checker leg (outside every timed region): frames `frames` of the last timed step against the CPU oracle: keypoint
    coordinates, sizes, responses, octaves, counts and descriptors bit for bit, angles within 1e-4 (north_star's float tolerance;
    bit-identical in practice); mvuRight / mvDepth / match count for stereo bit for bit."""
    import oracle
    oracle.build()
    ref = importlib.import_module("oracle.reference_frames")
    imgs, st = last
    bad = []
    for b in frames:
        if fe.stereo:
            e = ref.stereo_frame((fe.w, fe.h, fe.nf, seeds[b], fe.mbf, fe.mb, kind))
            for side, k, d, gi in (("left", e["kl"], e["dl"], b), ("right", e["kr"], e["dr"], fe.B + b)):
                m = ref.image_mismatch(imgs[gi][0], imgs[gi][1], k, d)
                if m:
                    bad.append("frame %d %s: %s" % (b, side, m))
            m = ref.stereo_mismatch(st[b], e)
            if m:
                bad.append("frame %d stereo: %s" % (b, m))
        else:
            e = ref.mono_frame((fe.w, fe.h, fe.nf, seeds[b], kind))
            m = ref.image_mismatch(imgs[b][0], imgs[b][1], e["k"], e["d"])
            if m:
                bad.append("frame %d: %s" % (b, m))
    return bad


def verify_gathered(fe, gath, ranks, frames_of_rank, kind="dense"):
    """N > 1 checker leg (rank 0, outside every timed region): the ALL-GATHERED records of the last timed step - every
    rank's frames as they arrived over the collective - against the CPU oracle of that rank's seeds.  frames_of_rank(B) picks the
    frames of each rank's block that are checked.  Returns (list of mismatches, frames checked)."""
    import oracle
    oracle.build()
    ref = importlib.import_module("oracle.reference_frames")
    pkg = importlib.import_module("orb_slam2v2-1_amd")
    bad = []
    j, step, held, rec = gath          # captured by measure() right behind the timed region (later passes refill the buffer sets)
    if held != step:
        return ["buffer set %d holds the gathered records of step %s, expected step %d" % (j, held, step)], 0
    g = {k: v.cpu().numpy() for k, v in rec.items()}
    gB, cap, nchk = fe.ring.gB, fe.cap, 0
    jobs, where = [], []
    for r in ranks:
        for b in frames_of_rank(r["frames_per_step"]):
            seed = r["first_seed"] + b
            jobs.append((fe.w, fe.h, fe.nf, seed, fe.mbf, fe.mb, kind) if fe.stereo else (fe.w, fe.h, fe.nf, seed, kind))
            where.append((r["rank"], b))
    exp = ref.run_pool(ref.stereo_frame if fe.stereo else ref.mono_frame, jobs)
    for (rk, b), e in zip(where, exp):
        row = rk * gB + b
        n = int(g["counts"][row])
        if n < 0 or n > cap:
            bad.append("rank %d frame %d: count %d" % (rk, b, n))
            continue
        k = np.frombuffer(g["kps"][row, :n].tobytes(), pkg.KP_DTYPE)
        d = g["desc"][row, :n]
        m = ref.image_mismatch(k, d, e["kl"] if fe.stereo else e["k"], e["dl"] if fe.stereo else e["d"])
        if m:
            bad.append("rank %d frame %d: %s" % (rk, b, m))
        if fe.stereo:
            ur, dp = g["uright"][row, :n], g["depth"][row, :n]
            if ur.tobytes() != e["uright"].tobytes() or dp.tobytes() != e["depth"].tobytes():
                bad.append("rank %d frame %d: gathered mvuRight / mvDepth differ" % (rk, b))
        nchk += 1
    return bad, nchk


def roofline_block(fe, m, workload, B, value, world, traffic_lookup=True):
    """roofline of the dominant kernel + whole-step figures, from the SURVEY section 8(d) byte formula."""
    w, h, stereo, nimg = fe.w, fe.h, fe.stereo, fe.nimg
    P = level_pixels(w, h)
    counts = np.array([len(k) for k, _ in m["last"][0]])
    navg = float(counts.mean())
    bytes_img = 3 * P + 60 * navg
    ncand_img = int(fe.ex.level_counts(0)[0].sum())   # FAST candidates of image 0
    bytes_frame = (2 * bytes_img + 64 * navg) if stereo else bytes_img
    stage_ms = m["stage_ms"]
    # dominant single kernel of the step (HIP events on the launch stream, averaged over the
    # timed region).  Algorithmic bytes per image: FAST+NMS reads every level once = P;
    # quad-tree reads its candidates; describe reads P + writes 60 N (SURVEY section 8(d) split).
    fast_names = fe.ex.fast_kernels(nimg)     # k_fast_strips for a GPU-filling batch (+ k_fast_cells for levels with wide cells)
    kern = {
        "+".join(fast_names): (m["fast_ms"], P * fe.ex.fast_images_per_launch),
        "k_octree": (float(stage_ms[2]), 8.0 * ncand_img * nimg),   # 4 B key + 2 B node index read, 2 B written
        "k_describe": (float(stage_ms[3]), (P + 60 * navg) * nimg),
    }
    dom = max(kern, key=lambda k: kern[k][0])
    dom_ms, dom_bytes = kern[dom]
    achieved = dom_bytes / (dom_ms * 1e-3) / 1e9
    traffic, traffic_source = None, None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if traffic_lookup and os.path.exists(pmc_path):
        try:
            pm = json.load(open(pmc_path))
            inst = [k for k in pm.get("kernels", {}) if k.split("<")[0] in dom.split("+")]   # template instances: k_fast_cells<44>
            if pm.get("workload") == workload and pm.get("batch") == B and inst:
                traffic = sum(pm["kernels"][k]["hbm_bytes_per_launch"] for k in inst)
                traffic_source = "profiles/pmc_traffic.json (separate rocprofv3 --pmc run of this command, NOT measured in this run)"
        except Exception:
            traffic = None
    roof = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": 8000.0,
            "unit": "GB/s", "frac": round(achieved / 8000.0, 5), "traffic": traffic, "traffic_source": traffic_source,
            "kernel_ms": round(dom_ms, 4), "algorithmic_bytes_per_launch": int(dom_bytes),
            "images_per_launch": fe.ex.fast_images_per_launch if dom.startswith("k_fast") else nimg,
            "pipeline_GBps": round(bytes_frame * value / world / 1e9, 2),
            "pipeline_frac": round(bytes_frame * value / world / 1e9 / 8000.0, 5),
            "algorithmic_bytes_per_frame": int(bytes_frame)}
    if dom.startswith("k_fast") and fe.lag and fe.late and not fe.fast_alone:
        roof["note"] = ("kernel_ms is this kernel's duration in the timed steps, where the stereo matcher of step i-1 (side stream) runs beside it "
                        "(--fast-alone: 0.265 ms alone / frac 0.087 and a 7 % longer step); stage_ms_per_call.fast is the FAST stage alone on the GPU")
    return roof, navg


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(fe, last, path, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: what the timed path handed its caller in the LAST timed step (this rank's frames), as float32 .npy files in
    `path`: keypoints [n, 7] (x, y, size, angle, response, octave, class_id), descriptors [n, 32] (byte values), keypoint_counts
    [images] and, for stereo, mvuRight / mvDepth [n of the left images] and stereo_matches [frames].  Images run left 0..B-1, then
    right 0..B-1; keypoints of consecutive images follow each other.  frames [frames dumped] names the frames: all of them, or a
    fixed seeded sample when the whole step would exceed `limit` bytes.  Returns the file names written."""
    imgs, st = last
    B = fe.B
    per_kp = 4 * (7 + 32 + (2 if fe.stereo else 0))
    sides = 2 if fe.stereo else 1
    nkp = [sum(len(imgs[s * B + b][0]) for s in range(sides)) for b in range(B)]
    frames = list(range(B))
    if sum(nkp) * per_kp + 16 * B > limit:
        order = np.random.default_rng(0).permutation(B)
        keep, tot = [], 0
        for b in order:
            if tot + nkp[b] * per_kp + 16 > limit:
                break
            keep.append(int(b))
            tot += nkp[b] * per_kp + 16
        frames = sorted(keep)
    order = [s * B + b for s in range(sides) for b in frames]
    kps = [imgs[i][0] for i in order]
    out = {
        "frames": np.array(frames, np.float32),
        "keypoint_counts": np.array([len(k) for k in kps], np.float32),
        "keypoints": np.concatenate([np.stack([k[f].astype(np.float32) for f in ("x", "y", "size", "angle", "response", "octave", "class_id")], 1)
                                     .reshape(-1, 7) for k in kps]),
        "descriptors": np.concatenate([imgs[i][1].astype(np.float32).reshape(-1, 32) for i in order]),
    }
    if fe.stereo:
        out["mvuRight"] = np.concatenate([st[b][0].astype(np.float32) for b in frames])
        out["mvDepth"] = np.concatenate([st[b][1].astype(np.float32) for b in frames])
        out["stereo_matches"] = np.array([st[b][2] for b in frames], np.float32)
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(name + ".npy" for name in out)


def launch_ranks(n):
    """`python bench.py --gpus N` without an outer launcher: start the N ranks as CHILD processes of torch.distributed.run (one
    per GPU, rendezvous on 127.0.0.1 at a free port) with this command line, relay what they print - rank 0's single JSON line
    goes to stdout as it arrives - and return their exit code.  Nothing in this process has touched the GPU (numpy only), and it
    is never replaced by another program: the ranks are children, the parent waits.  Under an outer torch.distributed.run
    (WORLD_SIZE / RANK set) main() never comes here."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        for line in p.stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
        rc = p.wait()
    except BaseException:
        p.terminate()           # the exact child this process started (its ranks die with the launcher)
        try:
            p.wait(30)
        except subprocess.TimeoutExpired:
            p.kill()
        raise
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ramp-steps", type=int, default=200,
                    help="untimed steps BEFORE the W warm-up steps: the GPU clocks need ~0.2 s of load to settle after the "
                         "CPU-only set-up phase (3 warm-up steps measured 2.5 %% low)")
    ap.add_argument("--workload", default="kitti_stereo_1241x376_1000feat", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=64, help="frames per step per GPU (weak scaling)")
    ap.add_argument("--total-frames", type=int, default=0,
                    help="T > 0: ONE batch of T frames per step sharded over the ranks (batching.shard_range), i.e. strong "
                         "scaling; BASELINE config 4 = --workload mono_1920x1080_4000feat --total-frames 512 --gpus 8")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the CPU baseline, the other workloads, the oracle checks, the roofline / stage "
                         "breakdown (FAST-stage events in the timed steps, an untimed stage-profile pass), long_run, end_to_end and the "
                         "tracking front end; the --no-* options below leave parts of it out.  Without it a run sets up, warms up, times "
                         "the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (keypoints, descriptors, counts, mvuRight, mvDepth; float32 .npy, "
                         "at most 64 MB) into DIR")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gather", action="store_true", help="skip the result all-gather when N > 1")
    ap.add_argument("--force-gather", action="store_true",
                    help="N = 1: run the pack + all-gather leg of the N > 1 step anyway, in a ONE-rank communicator of --backend (nccl = RCCL): "
                         "communicator set-up, the collective's stream, the async work handle and the hand-off from the handle's side stream all "
                         "execute on the one GPU of a test box; the line then also carries `gather_leg` (its cost per step)")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="skip the short untimed-by-the-driver runs of the other north-star sizes (other_workloads block)")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle check of the last timed step")
    ap.add_argument("--no-tracking", action="store_true", help="skip the chained tracking front-end block (config 5's shape)")
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the host-memory-to-host-memory pass (end_to_end block)")
    ap.add_argument("--verify-all-gathered", action="store_true",
                    help="N > 1: check EVERY frame of every rank in the all-gathered records of the last timed step against the oracle "
                         "(default: the first and last frame of each rank's block)")
    ap.add_argument("--streams", type=int, default=1,
                    help="S > 1: consecutive steps alternate over S extractor handles on S streams (independent steps overlap; "
                         "the default 1 keeps every kernel alone on the GPU so that its measured duration is its own)")
    ap.add_argument("--gen-workers", type=int, default=0,
                    help="processes that generate the synthetic frames (0 = by core count).  1 = no forked workers: use it under "
                         "rocprofv3, whose tool library in a forked worker can hang when the pool is torn down")
    ap.add_argument("--no-prefetch", action="store_true",
                    help="no software pipelining across steps (pyramid of the next step / stereo matcher of the previous one on a side "
                         "stream): every step then runs its kernels strictly one after the other")
    ap.add_argument("--no-lag-stereo", action="store_true", help="keep the pyramid built ahead but match each step's frames inside the step")
    ap.add_argument("--stereo-order", default="late", choices=["late", "early"],
                    help="order of the side stream behind FAST(i): late = pyramid(i+1) then matcher(i-1) (default, three pyramid buffers), "
                         "early = matcher(i-1) then pyramid(i+1) (rounds 2-3)")
    ap.add_argument("--fast-alone", action="store_true",
                    help="FAST(i+1) waits for the matcher of step i-1 (the arrangement of rounds 2-4: FAST has the GPU to itself; 104.8 k frames/s "
                         "against 111.8 k without the wait)")
    ap.add_argument("--overlap-pass", action="store_true",
                    help="after the measurement, an extra pass of K steps alternating over 3 handles on 3 streams; its throughput "
                         "is reported beside the headline value (\"overlapped\").  Off by default so that the kernel launches of "
                         "the default command are all single-stream (rocprof averages = the reported kernel duration)")
    ap.add_argument("--handle-options", default="", help="k=v[,k=v...]: orbx_set_option(k, v) on every extractor handle of this run (ORBX_OPT_* of "
                    "include/orbx.h: alternative kernels with identical results); recorded in config.handle_options")
    ap.add_argument("--gauss-flavour", default=os.environ.get("ORBX_TEST_GAUSS_FLAVOUR", "half_up"),
                    help="orbx_flavour_t of the handles AND of the oracle that checks them: half_up (default) | sse2 | taps:k0,k1,k2,k3")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (default); gloo only to rehearse N > 1 on a box with fewer GPUs than ranks")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    full = args.full
    verify = full and not args.no_verify
    os.environ["ORBX_TEST_GAUSS_FLAVOUR"] = args.gauss_flavour      # the oracle that checks the run, spawned workers and ranks included

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(launch_ranks(args.gpus))     # plain `python bench.py --gpus N`: this process only starts the ranks (no GPU call before)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE=%d; launch with torch.distributed.run "
                  "--nproc-per-node %d" % (args.gpus, world, args.gpus), file=sys.stderr)
        sys.exit(2)

    batching = importlib.import_module("orb_slam2v2-1_amd.batching")
    w, h, nf, stereo = WORKLOADS[args.workload]
    strong = args.total_frames > 0
    if strong:
        f0, f1 = batching.shard_range(args.total_frames, rank, world)
        B, seed0 = f1 - f0, f0
        if B < 1:
            print("bench.py: --total-frames %d leaves rank %d without frames" % (args.total_frames, rank), file=sys.stderr)
            sys.exit(2)
    else:
        B, seed0 = args.batch, 1000 * rank
    # host-side work that forks worker processes happens BEFORE this process touches the GPU
    workers = args.gen_workers if args.gen_workers > 0 else max(1, min((os.cpu_count() or 1) // max(world, 1), 16))
    kind = "natural" if args.workload in NATURAL else "dense"
    left, right = make_frames(w, h, B, seed0, stereo, workers, kind)
    seeds = [seed0 + i for i in range(B)]
    others = []
    if full and world == 1 and not args.no_other_workloads and not strong and args.streams == 1:
        for name, ob in OTHER_WORKLOADS:
            if name == args.workload:
                continue
            ow, oh, onf, ost = WORKLOADS[name]
            okind = "natural" if name in NATURAL else "dense"
            if (ow, oh, ost, okind) == (w, h, stereo, kind) and ob <= B:
                ol, orr = left[:ob], (right[:ob] if stereo else None)      # same images, other feature budget
                oseeds = seeds[:ob]
            else:
                ol, orr = make_frames(ow, oh, ob, 5000, ost, workers, okind)
                oseeds = [5000 + i for i in range(ob)]
            others.append((name, ob, ol, orr, oseeds))
    cpu = None
    if full and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(w, h, nf, stereo)

    pkg = importlib.import_module("orb_slam2v2-1_amd")
    pipeline = importlib.import_module("orb_slam2v2-1_amd.pipeline")
    pkg.lib()  # fails loudly if the HIP library is missing
    handle_options = {}
    for kv in args.handle_options.split(","):   # A/B runs: per-handle options of include/orbx.h for every handle this run creates
        if "=" in kv:
            handle_options[int(kv.split("=")[0])] = int(kv.split("=")[1])
            pkg.set_default_option(int(kv.split("=")[0]), int(kv.split("=")[1]))
    pkg.default_gauss_flavour = args.gauss_flavour
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible — the HIP path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    ndev = torch.cuda.device_count()
    if args.backend == "nccl" and world > ndev:
        print("bench.py: %d ranks but %d GPU(s): RCCL needs one GPU per rank" % (world, ndev), file=sys.stderr)
        sys.exit(3)
    dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    force_gather = bool(args.force_gather and world == 1 and not args.no_gather)
    if force_gather:      # a one-rank job has no launcher that sets the rendezvous: this process is rank 0 of 1 on the loopback address
        import socket
        s_ = socket.socket()
        s_.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(s_.getsockname()[1]))
        s_.close()
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or force_gather:
        # RCCL prints a version banner to STDOUT when its communicator is created (eagerly, with device_id given); stdout carries ONE JSON
        # line, so file descriptor 1 points at stderr while the process group comes up
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if args.backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group("gloo")
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
    gather = (world > 1 or force_gather) and not args.no_gather
    # the all-gather is a fixed-shape collective: every rank contributes as many record rows as the LARGEST block holds (a batch that
    # does not divide by the rank count leaves blocks that differ by one frame; the short blocks' last row stays empty)
    gB = max(b - a for a, b in (batching.shard_range(args.total_frames, r, world) for r in range(world))) if strong else B

    S = max(1, args.streams)
    fe = pipeline.FrontEnd(w, h, nf, stereo, B, device_index=dev_index, nbuf=3, streams=S, world=world, gather=gather,
                           gather_via_host=(args.backend != "nccl"), prefetch=not args.no_prefetch, lag_stereo=not args.no_lag_stereo, gather_B=gB,
                           stereo_late=(args.stereo_order == "late"), fast_alone=args.fast_alone, force_gather=force_gather)
    fe.upload(left, right)
    m = measure(fe, args.steps, args.warmup, args.ramp_steps, world, dist, dev, torch, full=full)
    dumped = dump_outputs(fe, m["last"], args.dump_outputs) if args.dump_outputs and rank == 0 else None
    gather_leg = measure_gather_leg(fe, torch) if force_gather else None
    dt, stage_ms = m["dt"], m["stage_ms"]

    # Extra pass (--overlap-pass, 1 GPU): the same K steps alternating over THREE extractor handles on three streams.
    # Steps are independent, so the latency-bound kernels of one step (upper pyramid levels, quad-tree, stereo bins /
    # median) overlap the VALU-bound ones of another.  Reported beside `value`, not as `value`: with kernels sharing the
    # GPU a kernel's own duration cannot be measured, and the roofline above is about kernels measured alone.
    overlapped = None
    if world == 1 and S == 1 and args.overlap_pass:
        fe3 = pipeline.FrontEnd(w, h, nf, stereo, B, device_index=dev_index, nbuf=3, streams=3)
        fe3.upload(left, right)
        for i in range(30):
            fe3.step(i)
        fe3.drain()
        t3 = time.perf_counter()
        for i in range(args.steps):
            fe3.step(i)
        fe3.drain()
        dt3 = time.perf_counter() - t3
        bad3 = verify_against_oracle(fe3, fe3.results((args.steps - 1) % 3), seeds, [0, B - 1]) if verify else []
        overlapped = {"streams": 3, "value": round(B * args.steps / dt3, 2), "unit": "frames/s",
                      "ms_per_step": round(dt3 / args.steps * 1e3, 4), "steps": args.steps, "verified": (not bad3 if verify else None),
                      "note": "independent steps alternate over 3 handles on 3 streams; kernels share the GPU, so "
                              "per-kernel durations are not isolated - informational, not the headline value"}
        del fe3

    # who took part: proves on a multi-GPU record that RCCL really saw N ranks on N devices
    me = {"rank": rank, "local_rank": local_rank, "device_index": dev_index, "device": torch.cuda.get_device_name(dev_index),
          "frames_per_step": B, "first_seed": seed0}
    ranks = [me]
    world_seen = 1
    if world > 1:
        world_seen = dist.get_world_size()
        ranks = [None] * world
        dist.all_gather_object(ranks, me)

    if rank == 0:
        frames_per_step = args.total_frames if strong else world * B
        value = frames_per_step * args.steps / dt
        if full:
            roof, navg = roofline_block(fe, m, args.workload, B, value, world)
        else:
            roof, navg = None, float(np.mean([len(k) for k, _ in m["last"][0]]))
        verified, vnote = None, "skipped (--no-verify)" if full else "skipped (the oracle check runs with --full)"
        if verify:
            vf = sorted({0, B // 2, B - 1})
            bad = verify_against_oracle(fe, m["last"], seeds, vf, kind)
            verified = not bad
            vnote = ("frames %s of the last timed step == CPU oracle: keypoint x / y / size / response / octave, counts and descriptors "
                     "bit for bit, angles within 1e-4%s" % (vf, ", mvuRight / mvDepth / match counts bit for bit" if stereo else "")
                     ) if verified else "; ".join(bad[:5])
        gathered_verified, gnote = None, None
        if m["gathered"] is not None and verify:
            pick = (lambda nb: range(nb)) if args.verify_all_gathered else (lambda nb: sorted({0, nb - 1}))
            gbad, nchk = verify_gathered(fe, m["gathered"], ranks, pick, kind)
            gathered_verified = not gbad
            gnote = ("%d frames (%s of every rank's block) of the all-gathered records of the last timed step, as received on rank 0, "
                     "== CPU oracle of the owning rank's seeds" % (nchk, "all" if args.verify_all_gathered else "first and last")
                     ) if gathered_verified else "; ".join(gbad[:5])
        out = {
            "metric": "frames/s ORB extract+match @1241x376 8-lvl 1000-feat" if args.workload.startswith("kitti_stereo_1241x376_1000")
            else "frames/s ORB extract+match (%s)" % args.workload,
            "value": round(value, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "verified": verified, "verified_note": vnote, "gathered_verified": gathered_verified, "gathered_verified_note": gnote,
            "config": {"workload": args.workload, "frame": "stereo pair (2 images)" if stereo else "mono image",
                       "width": w, "height": h, "nlevels": 8, "scale_factor": 1.2, "nfeatures": nf,
                       "ini_th_fast": 20, "min_th_fast": 7, "frames_per_step_per_gpu": B, "clock_ramp_steps": args.ramp_steps,
                       "total_frames_per_step": frames_per_step,
                       "match": "Frame::ComputeStereoMatches" if stereo else "none",
                       "pipelining": (("behind the FAST stage of step i, on a side stream: pyramid of step i+1, then stereo matcher of step i-1" +
                                       (" (FAST of step i+1 waits for it)" if fe.fast_alone else " (which may run on beside the FAST stage of step i+1)")
                                       if fe.late else "behind the FAST stage of step i, on a side stream: stereo matcher of step i-1, then pyramid of step i+1") if fe.lag
                                      else "pyramid of the next step built ahead (orbx_extract_batch_device_prefetch)") if fe.prefetch else "none",
                       "parallelism": "frames sharded over %d GPU(s)%s" % (world, ", results all-gathered (%s%s)" % ("RCCL" if args.backend == "nccl" else "gloo rehearsal",
                                                                                  ", one-rank communicator (--force-gather)" if force_gather else "") if gather else ""),
                       "world_size_observed": world_seen, "ranks": ranks,
                       "avg_keypoints_per_image": round(navg, 1), "gauss_flavour": args.gauss_flavour,
                       "handle_options": handle_options},
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "files": dumped}
        if full:
            out.update({
                "roofline": roof,
                "long_run": None if m.get("long_run") is None else {
                    "steps": m["long_run"][0], "value": round(B * m["long_run"][0] / m["long_run"][1], 2), "unit": "frames/s",
                    "ms_per_step": round(m["long_run"][1] / m["long_run"][0] * 1e3, 4),
                    "note": "the same loop over 100 steps right after the timed region (K < 100 is a short sample); informational, not `value`"},
                "stage_ms_per_call": {"pyramid": round(float(stage_ms[0]), 4), "fast": round(float(stage_ms[1]), 4),
                                      "quadtree": round(float(stage_ms[2]), 4), "describe": round(float(stage_ms[3]), 4),
                                      "extract_total": round(float(stage_ms[4]), 4), "stereo_match": round(m["match_ms"], 4),
                                      "images_per_call": fe.nimg, "calls_averaged": m["ncalls"],
                                      "fast_timed_region": round(m["fast_ms"], 4),
                                      "note": "stage breakdown from an untimed pass of %d steps after the timed region, every stage alone on the GPU "
                                              "(in the timed steps %s on a side stream behind the FAST stage of step i, beside its gather / quad-tree / descriptor "
                                              "kernels - and the matcher beside the next FAST stage -, which makes those longer and the step shorter than the sum here); "
                                              "roofline.kernel_ms is the FAST stage (%s) over the %d timed steps" % (
                                                  m["nprof"], "the stereo matcher of step i-1 and the pyramid of step i+1 run" if fe.lag else
                                                  "the pyramid of step i+1 runs" if fe.prefetch else "nothing runs", roof["kernel"], args.steps)},
            })
        if full and world == 1 and S == 1 and not args.no_end_to_end:
            # beside the headline (never `value`): the step fed from host memory, PCIe both ways inside the clock
            fe2 = fe      # the same front end (its results were captured above); a second handle's streams measured 10-15 % slower here
            dte, laste = measure_end_to_end(fe2, left, right, args.steps, 10, torch)
            bade = verify_against_oracle(fe2, laste, seeds, sorted({0, B - 1}), kind) if verify else []
            up = fe2.nimg * w * h
            down = sum(t.numel() * t.element_size() for t in fe2._hs.out[0].values())
            out["end_to_end"] = {
                "value": round(B * args.steps / dte, 2), "unit": "frames/s", "ms_per_step": round(dte / args.steps * 1e3, 4), "steps": args.steps,
                "h2d_bytes_per_step": up, "d2h_bytes_per_step": down, "h2d_GBps": round(up * args.steps / dte / 1e9, 2),
                "d2h_GBps": round(down * args.steps / dte / 1e9, 2), "verified": not bade if verify else None,
                "note": "frames start in PINNED host memory and results (keypoints, descriptors, counts, mvuRight, mvDepth at full "
                        "capacity) end in pinned host memory; one hipMemcpyAsync per camera and batch on an upload stream, three image "
                        "buffers in HBM, downloads on a third stream, all overlapped with the kernels of the neighbouring batches; the host "
                        "waits for the results of step i - 3 before it submits batch i + 2; clock from the first upload to the last "
                        "result's arrival.  NOT the headline value (which starts with frames in HBM)"}
        if full and world == 1 and not args.no_tracking and args.workload.startswith("kitti_stereo_1241x376_1000"):
            try:
                out["tracking_front_end"] = tracking_front_end()
            except Exception as e:      # a broken side block must not take the headline line with it
                out["tracking_front_end"] = {"error": repr(e)}
        if others:
            # the other north-star sizes, same definition of a step, short runs (not the headline; the driver times only `value`)
            del fe
            ow_out = {}
            for name, ob, ol, orr, oseeds in others:
                oww, ohh, onf, ost = WORKLOADS[name]
                ofe = pipeline.FrontEnd(oww, ohh, onf, ost, ob, device_index=dev_index, nbuf=3)
                ofe.upload(ol, orr)
                osteps = 30
                om = measure(ofe, osteps, 5, 60, 1, dist, dev, torch)
                om_b = measure(ofe, osteps, 5, 0, 1, dist, dev, torch)     # a 20-ms region is one noisy sample: the better of two ...
                dt_mean = 0.5 * (om["dt"] + om_b["dt"])                     # ... reported as `value`, the MEAN of the two beside it
                if om_b["dt"] < om["dt"]:
                    om = om_b
                oval = ob * osteps / om["dt"]
                oroof, onavg = roofline_block(ofe, om, name, ob, oval, 1, traffic_lookup=False)
                okind = "natural" if name in NATURAL else "dense"
                obad = verify_against_oracle(ofe, om["last"], oseeds, [0, ob - 1], okind) if verify else []
                ow_out[name] = {"value": round(oval, 2), "unit": "frames/s" if ost else "images/s", "frames_per_step": ob,
                                "steps": osteps, "repeats": "value / ms_per_step: the BETTER of 2 runs of %d steps; value_mean_of_2 / ms_per_step_mean_of_2: their mean" % osteps,
                                "ms_per_step": round(om["dt"] / osteps * 1e3, 4),
                                "value_mean_of_2": round(ob * osteps / dt_mean, 2), "ms_per_step_mean_of_2": round(dt_mean / osteps * 1e3, 4),
                                "dominant_kernel": oroof["kernel"], "dominant_kernel_ms": oroof["kernel_ms"],
                                "roofline_frac": oroof["frac"], "pipeline_frac": oroof["pipeline_frac"],
                                "avg_keypoints_per_image": round(onavg, 1),
                                "stage_ms_alone": {k: round(float(v), 4) for k, v in zip(("pyramid", "fast", "quadtree", "describe"), om["stage_ms"][:4])},
                                "verified": not obad if verify else None}
                if okind == "natural":
                    # the corner-sparse workload with and without k_fast_strips' exact row pre-test (developer knob 16 = 1: off)
                    pkg.set_default_option(16, 1)
                    om2 = measure(ofe, osteps, 5, 20, 1, dist, dev, torch)
                    pkg.set_default_option(16, 0)
                    ow_out[name].update({
                        "corner_fraction_note": "2-5 % of the pixels are FAST corners at t = 7 (dense workloads: 33-53 %)",
                        "fast_ms_with_row_pretest": round(om["fast_ms"], 4), "fast_ms_without": round(om2["fast_ms"], 4),
                        "value_without_row_pretest": round(ob * osteps / om2["dt"], 2)})
                del ofe
            out["other_workloads"] = ow_out
        if gather_leg is not None:
            out["gather_leg"] = gather_leg
        if cpu is not None:
            out["cpu_baseline"] = cpu
        if overlapped is not None:
            out["overlapped"] = overlapped
        print(json.dumps(out), flush=True)
    if world > 1 or force_gather:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
