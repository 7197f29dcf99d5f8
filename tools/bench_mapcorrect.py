"""The two loop map correction entry points (orbr_correct_loop, orbr_spread_global_ba) at the sizes a loop closure meets, beside the same
loops on the CPU.

  python tools/bench_mapcorrect.py                       # every size
  python tools/bench_mapcorrect.py loop --calls 30 --warm 5
  python tools/bench_mapcorrect.py spread
  rocprofv3 --kernel-trace --stats -- python tools/bench_mapcorrect.py loop --calls 5 --warm 2      # the kernels apart

Sizes: `loop`, one CorrectLoop: 100 connected keyframes (every third of 300) over 30 000 points with about 8 observations each;
`spread`, the map after a global bundle adjustment at the two larger sizes of tools/bench_gba.py, 160 keyframes : 16 000 points and
1000 : 100 000, the last 16 keyframes, a chain, and the points that refer to them outside the optimisation (local mapping went on).

Per call: the median and the minimum of a host clock around the C entry point itself through ctypes, its structures and output arrays
made once before the loop (argument checks, graph work, packing, upload, launches, download and the one stream synchronisation);
`upload_ms` / `download_ms`: a copy of exactly the call's input / output bytes between pinned memory and the device on a stream, timed
alone the same way; `rest_ms` = median - upload - download: the launches, the host's packing and the synchronisation.  upload_share =
upload_ms / median_ms.  `host_ms`: the reference's loops on the CPU over host/frame_shim.h's objects, std::maps and cv::Mat
temporaries (tools/mapcorrect_host_loops.cc, g++ -O2, one thread, the best of 3).  The two sides are checked to agree on the sum of
the positions they leave before a number is printed.  No ratio is a goal here.  One JSON line per size."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default


CALLS, WARM = opt("--calls", 20), opt("--warm", 3)
kinds = args or ["loop", "spread"]
pkg = importlib.import_module("orb_slam2v2-1_amd")
NLEVELS = 8
SF = np.array([1.2 ** l for l in range(NLEVELS)], np.float32)
F32 = np.float32


def poses(rng, K):
    """keyframes along x at 2 m steps looking down +z, a small rotation about y each"""
    a = rng.normal(0, 0.02, K)
    T = np.zeros((K, 4, 4), F32)
    T[:, 0, 0], T[:, 0, 2], T[:, 2, 0], T[:, 2, 2], T[:, 1, 1], T[:, 3, 3] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a), 1, 1
    C_ = np.stack([2.0 * np.arange(K), rng.normal(0, 0.05, K), rng.normal(0, 0.05, K)], 1)
    T[:, :3, 3] = -np.einsum("kij,kj->ki", T[:, :3, :3].astype(np.float64), C_)
    Ow = -np.einsum("kji,kj->ki", T[:, :3, :3].astype(np.float64), T[:, :3, 3].astype(np.float64))
    return T, Ow.astype(F32)


def make_loop(seed, K, P, mean_obs, Q):
    """bench_covis.py's map with poses: a point is seen by a run of neighbouring keyframes; every third keyframe is connected"""
    rng = np.random.default_rng(seed)
    Tcw, Ow = poses(rng, K)
    kf = np.zeros(K, pkg.COVIS_KEYFRAME_DTYPE)
    kf["id"], kf["th_depth"], kf["Ow"] = np.arange(K) + 1, 40.0, Ow
    n = np.clip(rng.poisson(mean_obs - 2, P) + 2, 2, K)
    first = np.clip(rng.integers(0, K, P) - n // 2, 0, K - n)
    pt_of = np.repeat(np.arange(P), n)
    kf_of = np.repeat(first, n) + (np.arange(len(pt_of)) - np.repeat(np.cumsum(n) - n, n))
    order = np.lexsort((pt_of, kf_of))
    idx = np.empty(len(pt_of), np.int64)
    start = np.searchsorted(kf_of[order], np.arange(K))
    idx[order] = np.arange(len(pt_of)) - start[kf_of[order]]
    lvl = np.clip(np.repeat(rng.integers(0, NLEVELS - 2, P), n) + rng.integers(0, 3, len(pt_of)), 0, NLEVELS - 1)
    pts = np.zeros(P, pkg.COVIS_POINT_DTYPE)
    pts["pos"] = np.stack([2.0 * (first + n / 2.0), rng.uniform(-2, 2, P), rng.uniform(4, 20, P)], 1)
    pts["ref_kf"] = first
    table = pkg.covis_table(kf, pts, np.stack([pt_of, kf_of, idx, lvl, np.zeros_like(lvl)], 1), SF)
    qs = np.arange(K)[::K // Q][:Q]
    feats = []
    for s in qs:
        m = kf_of == s
        f = np.zeros(int(m.sum()), pkg.COVIS_FEATURE_DTYPE)
        f["point"][idx[m]], f["octave"][idx[m]] = pt_of[m], lvl[m]
        feats.append(f)
    cur = int(qs[-2])
    Scw = np.zeros(1, pkg.MAPCORRECT_SIM3_DTYPE)
    Scw["q"][0], Scw["t"][0], Scw["s"][0] = [0.01, -0.02, 0.015, 0.9996], Tcw[cur, :3, 3].astype(np.float64) + [0.3, -0.1, 0.2], 1.05
    return dict(table=table, queries=pkg.covis_queries(qs, feats), cur=cur, Tiw=np.ascontiguousarray(Tcw[qs]), Scw=Scw)


def make_spread(seed, K, P):
    """a chain of keyframes from one origin; the last 16 outside the global BA (16 levels), and so the points that refer to them"""
    rng = np.random.default_rng(seed)
    Tcw, _ = poses(rng, K)
    gba = Tcw.copy()
    gba[:, :3, 3] += rng.normal(0, 0.05, (K, 3)).astype(F32)
    ingba = (np.arange(K) < K - 16).astype(np.uint8)
    off = np.minimum(np.arange(K + 1), K - 1).astype(np.int32)      # keyframe k's only child is k + 1
    child = np.arange(1, K, dtype=np.int32)
    ref = rng.integers(0, K, P).astype(np.int32)
    return dict(Tcw=Tcw, TcwGBA=gba, kf_in_gba=ingba, child_off=off, child=child, origins=np.zeros(1, np.int32),
                pos=np.stack([2.0 * ref + rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(4, 20, P)], 1).astype(F32),
                posGBA=rng.uniform(-2, 20, (P, 3)).astype(F32), pt_in_gba=ingba[ref].copy(), ref_kf=ref, bad=(rng.random(P) < 0.02).astype(np.uint8))


def timed(fn):
    ms, res = [], None
    for _ in range(WARM + CALLS):
        t0 = time.perf_counter()
        res = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[WARM:]
    return float(np.median(ms)), float(min(ms)), res


def copy_ms(nbytes, up):
    import torch
    h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()

    def go():
        with torch.cuda.stream(st):
            (d if up else h).copy_(h if up else d, non_blocking=True)
        st.synchronize()
    return timed(go)[0]


def al(n):
    return (n + 255) & ~255


def p_(a):
    return a.ctypes.data


def loop_call(sc):
    L = pkg.lib()
    t, q = sc["table"], sc["queries"]
    Q, P = len(q["query_kf"]), len(t["pts"])
    ct, cq = pkg._covis_c_table(t), pkg._covis_c_queries(q)
    out = dict(corrected=np.zeros(Q, pkg.MAPCORRECT_SIM3_DTYPE), non_corrected=np.zeros(Q, pkg.MAPCORRECT_SIM3_DTYPE), Tiw_new=np.zeros((Q, 4, 4), F32),
               Ow_new=np.zeros((Q, 3), F32), pos=np.zeros((P, 3), F32), corrected_ref=np.zeros(P, np.int32), normals=np.zeros(P, pkg.COVIS_NORMAL_DTYPE))
    co = pkg.MapCorrectLoopOut(*[p_(out[k]) for k in ("corrected", "non_corrected", "Tiw_new", "Ow_new", "pos", "corrected_ref", "normals")])
    a = (C.addressof(ct), C.addressof(cq), int(sc["cur"]), p_(sc["Tiw"]), p_(sc["Scw"]), C.addressof(co), 0)
    keep = (ct, cq, co)

    def go():
        rc = L.orbr_correct_loop(*a)
        if rc:
            raise pkg.OrbxError(rc, L.orbx_last_error().decode())
        return keep
    nin = sum(al(t[k].nbytes) for k in ("kf", "pts", "obs_off", "obs", "sf")) + sum(al(q[k].nbytes) for k in ("query_kf", "feat_off", "feat")) + al(4 * len(t["kf"])) + al(64 * Q)
    return go, out, nin, sum(al(v.nbytes) for v in out.values())


def spread_call(sc):
    L = pkg.lib()
    K, P = len(sc["kf_in_gba"]), len(sc["bad"])
    out = dict(Tcw_new=np.zeros((K, 4, 4), F32), TcwGBA=np.zeros((K, 4, 4), F32), kf_marked=np.zeros(K, np.uint8), kf_reached=np.zeros(K, np.uint8),
               pos=np.zeros((P, 3), F32), status=np.zeros(P, np.int32))
    si = pkg.MapCorrectSpreadIn(K, p_(sc["Tcw"]), p_(sc["TcwGBA"]), p_(sc["kf_in_gba"]), p_(sc["child_off"]), p_(sc["child"]), p_(sc["origins"]), len(sc["origins"]), P,
                                p_(sc["pos"]), p_(sc["posGBA"]), p_(sc["pt_in_gba"]), p_(sc["ref_kf"]), p_(sc["bad"]))
    so = pkg.MapCorrectSpreadOut(p_(out["Tcw_new"]), p_(out["TcwGBA"]), p_(out["kf_marked"]), p_(out["kf_reached"]), p_(out["pos"]), p_(out["status"]), 0)

    def go():
        rc = L.orbr_spread_global_ba(C.addressof(si), C.addressof(so), 0)
        if rc:
            raise pkg.OrbxError(rc, L.orbx_last_error().decode())
        return so
    nin = 2 * al(64 * K) + 2 * al(4 * K) + 2 * al(K) + 2 * al(12 * P) + 2 * al(P) + al(4 * P)
    return go, out, nin, al(64 * K) + al(12 * P) + al(4 * P)


def host_loops(exe, mode, blob):
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(blob)
        return json.loads(subprocess.run([exe, mode, os.path.join(tmp, "in.bin"), "3"], check=True, capture_output=True, text=True).stdout)


def report(line, t, nin, nout, host, pos):
    up, down = copy_ms(nin, True), copy_ms(nout, False)
    s = float(pos.astype(np.float64).sum())
    assert abs(s - host["pos_sum"]) <= 1e-9 * abs(host["pos_sum"]), (s, host)
    line.update(median_ms=round(t[0], 4), min_ms=round(t[1], 4), input_bytes=nin, output_bytes=nout, upload_ms=round(up, 4), download_ms=round(down, 4),
                rest_ms=round(t[0] - up - down, 4), upload_share=round(up / t[0], 3), host_ms=round(host["ms"], 4))
    print(json.dumps(line), flush=True)


with tempfile.TemporaryDirectory() as bindir:
    exe = os.path.join(bindir, "mapcorrect_host_loops")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"),
                           os.path.join(ROOT, "tools", "mapcorrect_host_loops.cc"), "-o", exe])
    if "loop" in kinds:
        sc = make_loop(7, 300, 30000, 8, 100)
        t, q = sc["table"], sc["queries"]
        go, out, nin, nout = loop_call(sc)
        tm = timed(go)
        hd = np.array([len(t["kf"]), len(t["pts"]), len(t["obs"]), len(t["sf"]), len(q["query_kf"]), len(q["feat"]), sc["cur"]], np.int32)
        blob = b"".join(np.ascontiguousarray(a).tobytes() for a in (hd, t["kf"], t["pts"], t["obs_off"], t["obs"], t["sf"], q["query_kf"], q["feat_off"], q["feat"],
                                                                    sc["Tiw"], sc["Scw"]))
        line = dict(call="correct_loop", keyframes=len(t["kf"]), connected=len(q["query_kf"]), points=len(t["pts"]), observations=len(t["obs"]), features=len(q["feat"]),
                    corrected=int((out["corrected_ref"] >= 0).sum()), calls=CALLS)
        report(line, tm, nin, nout, host_loops(exe, "loop", blob), out["pos"])
    if "spread" in kinds:
        for K, P in ((160, 16000), (1000, 100000)):
            sc = make_spread(8, K, P)
            go, out, nin, nout = spread_call(sc)
            tm = timed(go)
            hd = np.array([K, P, len(sc["child"]), 1], np.int32)
            blob = b"".join(np.ascontiguousarray(sc[k]).tobytes() for k in ("Tcw", "TcwGBA", "kf_in_gba", "child_off", "child", "origins", "pos", "posGBA", "pt_in_gba",
                                                                           "ref_kf", "bad"))
            line = dict(call="spread_global_ba", keyframes=K, points=P, levels=int(tm[2].levels), moved=int((out["status"] == 2).sum()),
                        took_gba=int((out["status"] == 1).sum()), calls=CALLS)
            report(line, tm, nin, nout, host_loops(exe, "spread", hd.tobytes() + blob), out["pos"])
