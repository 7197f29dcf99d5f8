"""The three covisibility entry points (orbc_update_connections, orbc_keyframe_culling, orbc_update_normal_and_depth, and the combined
orbc_covisibility) at two sizes, beside the same computations on the CPU.

  python tools/bench_covis.py                       # both sizes
  python tools/bench_covis.py local --calls 30 --warm 5
  python tools/bench_covis.py global
  rocprofv3 --kernel-trace --stats -- python tools/bench_covis.py local --calls 5 --warm 2      # the kernels apart

Sizes: `local`, a local window: 30 query keyframes of about 1500 features each among 60 keyframes, about 8 observations per point;
`global`, the write-back after a global bundle adjustment: 100 000 points with about 10 observations each over 1000 keyframes, with
30 queries of the same kind so that the other two entry points run on that table too.

Per entry point: the median and the minimum of a host clock around the C entry point itself, `orbc_covisibility` through ctypes with
its structures and output arrays made once before the loop (argument checks, packing, upload, launches, download and the one stream
synchronisation; nothing of the Python wrappers, whose allocations and precondition check are not the library's), and `upload_ms`: a host-to-device copy
of exactly the call's input bytes from pinned memory on a stream, timed alone the same way.  upload_share = upload_ms / median_ms: the
part of the call a device-resident table would save at most.  `host_*_ms`: the same three computations on the CPU over
host/frame_shim.h's objects and std::maps, a point's observation map copied per visit as the reference copies it
(tools/covis_host_loops.cc, g++ -O2, one thread, the same tables, the best of 3).  The two sides are checked to agree on
what they computed before a number is printed.  No ratio is a goal here: at the local size the upload and the call's fixed costs may
well dominate and the CPU may win.  One JSON line per size."""
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
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default


CALLS, WARM = opt("--calls", 20), opt("--warm", 3)
sizes = args or ["local", "global"]
pkg = importlib.import_module("orb_slam2v2-1_amd")
NLEVELS = 8
SF = np.array([1.2 ** l for l in range(NLEVELS)], np.float32)


def make(seed, K, P, mean_obs, Q):
    """Keyframes along a path; a point is seen by a run of neighbouring keyframes around a random centre (so that neighbours share
    many points), each at a random level near the point's own; 30 % of the observations stereo.  Consistent: feature idx of an
    observation names the point."""
    rng = np.random.default_rng(seed)
    kf = np.zeros(K, pkg.COVIS_KEYFRAME_DTYPE)
    kf["id"], kf["th_depth"] = np.arange(K), 40.0
    kf["Ow"] = np.stack([2.0 * np.arange(K), rng.normal(0, 0.05, K), rng.normal(0, 0.05, K)], 1)
    n = np.clip(rng.poisson(mean_obs - 2, P) + 2, 2, K)
    first = np.clip(rng.integers(0, K, P) - n // 2, 0, K - n)
    pt_of = np.repeat(np.arange(P), n)
    kf_of = np.repeat(first, n) + (np.arange(len(pt_of)) - np.repeat(np.cumsum(n) - n, n))
    order = np.lexsort((pt_of, kf_of))                       # feature index = rank of the observation inside its keyframe
    idx = np.empty(len(pt_of), np.int64)
    start = np.searchsorted(kf_of[order], np.arange(K))
    idx[order] = np.arange(len(pt_of)) - start[kf_of[order]]
    lvl = np.clip(np.repeat(rng.integers(0, NLEVELS - 2, P), n) + rng.integers(0, 3, len(pt_of)), 0, NLEVELS - 1)
    st = rng.random(len(pt_of)) < 0.3
    pts = np.zeros(P, pkg.COVIS_POINT_DTYPE)
    pts["pos"] = np.stack([2.0 * (first + n / 2.0), rng.uniform(-2, 2, P), rng.uniform(4, 20, P)], 1)
    pts["ref_kf"] = first
    table = pkg.covis_table(kf, pts, np.stack([pt_of, kf_of, idx, lvl, st], 1), SF)
    qs = np.sort(rng.permutation(K)[:Q])
    feats = []
    for s in qs:
        m = kf_of == s
        f = np.zeros(int(m.sum()), pkg.COVIS_FEATURE_DTYPE)
        f["point"][idx[m]], f["octave"][idx[m]] = pt_of[m], lvl[m]
        f["depth"] = rng.choice([8.0, 25.0, 60.0], len(f), p=[0.6, 0.3, 0.1])
        feats.append(f)
    return table, pkg.covis_queries(qs, feats)


def timed(fn):
    ms, res = [], None
    for _ in range(WARM + CALLS):
        t0 = time.perf_counter()
        res = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[WARM:]
    return float(np.median(ms)), float(min(ms)), res


def c_call(table, conn_q=None, cull_q=None, normals=False):
    """orbc_covisibility with everything it needs made once -> (a function that makes the call and nothing else, the output arrays)"""
    L = pkg.lib()
    K, P = len(table["kf"]), len(table["pts"])
    ct = pkg._covis_c_table(table)
    keep, a = [ct], [C.addressof(ct), None, None, None, None, None, 0]
    out = {}
    if conn_q is not None:
        Q = len(conn_q["query_kf"])
        out["ids"], out["weights"], out["n"], out["counters"] = np.zeros((Q, K), np.int32), np.zeros((Q, K), np.int32), np.zeros(Q, np.int32), np.zeros((Q, K), np.int32)
        cq = pkg._covis_c_queries(conn_q)
        cc = pkg.CovisConnections(15, K, out["ids"].ctypes.data, out["weights"].ctypes.data, out["n"].ctypes.data, out["counters"].ctypes.data)
        keep += [cq, cc]
        a[1], a[2] = C.addressof(cq), C.addressof(cc)
    if cull_q is not None:
        Q = len(cull_q["query_kf"])
        out["n_mps"], out["n_redundant"], out["verdict"], out["point_bad"] = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(P, np.uint8)
        kq = pkg._covis_c_queries(cull_q)
        kc = pkg.CovisCulling(0, 3, out["n_mps"].ctypes.data, out["n_redundant"].ctypes.data, out["verdict"].ctypes.data, out["point_bad"].ctypes.data)
        keep += [kq, kc]
        a[3], a[4] = C.addressof(kq), C.addressof(kc)
    if normals:
        out["normals"] = np.zeros(P, pkg.COVIS_NORMAL_DTYPE)
        a[5] = out["normals"].ctypes.data
    fn = L.orbc_covisibility

    def go():
        rc = fn(*a)
        if rc:
            raise pkg.OrbxError(rc, L.orbx_last_error().decode())
        return keep
    return go, out


def upload_ms(nbytes):
    import torch
    h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()

    def go():
        with torch.cuda.stream(st):
            d.copy_(h, non_blocking=True)
        st.synchronize()
    return timed(go)[0]


def al(n):
    return (n + 255) & ~255


def host_loops(table, q, exe):
    with tempfile.TemporaryDirectory() as tmp:
        hd = np.array([len(table["kf"]), len(table["pts"]), len(table["obs"]), len(table["sf"]), len(q["query_kf"]), len(q["feat"]), len(q["query_kf"]),
                       len(q["feat"]), 15, 0, 0, 3], np.int32)
        qb = q["query_kf"].tobytes() + q["feat_off"].tobytes() + q["feat"].tobytes()
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(hd.tobytes() + table["kf"].tobytes() + table["pts"].tobytes() + table["obs_off"].tobytes() + table["obs"].tobytes() + table["sf"].tobytes() + qb + qb)
        return json.loads(subprocess.run([exe, os.path.join(tmp, "in.bin"), "3"], check=True, capture_output=True, text=True).stdout)


with tempfile.TemporaryDirectory() as bindir:
    exe = os.path.join(bindir, "covis_host_loops")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"),
                           os.path.join(ROOT, "tools", "covis_host_loops.cc"), "-o", exe])
    for size in sizes:
        K, P, mean_obs, Q = {"local": (60, 11000, 8, 30), "global": (1000, 100000, 10, 30)}[size]
        table, q = make(7, K, P, mean_obs, Q)
        pkg.covis_check(table, q, culling=True)
        tab_bytes = sum(al(table[k].nbytes) for k in ("kf", "pts", "obs_off", "obs", "sf"))
        q_bytes = sum(al(q[k].nbytes) for k in ("query_kf", "feat_off", "feat"))
        line = dict(size=size, keyframes=K, points=P, observations=len(table["obs"]), queries=Q, features=len(q["feat"]), calls=CALLS)
        calls = dict(connections=c_call(table, conn_q=q), culling=c_call(table, cull_q=q), normals=c_call(table, normals=True),
                     combined=c_call(table, conn_q=q, cull_q=q, normals=True))
        conn, cull, nrm, both = (timed(calls[k][0]) for k in ("connections", "culling", "normals", "combined"))
        host = host_loops(table, q, exe)
        n, ws = calls["connections"][1]["n"], calls["connections"][1]["weights"]
        # the two sides computed the same thing, and the combined call what the single ones did
        assert int((np.minimum(n, K) + ws[:, 0] * (n > 0)).sum()) == host["connections_sum"], (host, int(n.sum()))
        assert int((calls["culling"][1]["verdict"] != 0).sum()) == host["culled"], host
        assert abs(float(calls["normals"][1]["normals"]["max_distance"].astype(np.float64).sum()) - host["max_distance_sum"]) <= 1e-5 * host["max_distance_sum"], host
        for part in ("connections", "culling", "normals"):
            for k, v in calls[part][1].items():
                assert v.tobytes() == calls["combined"][1][k].tobytes(), k
        for name, t, nbytes in (("connections", conn, tab_bytes + q_bytes), ("culling", cull, tab_bytes + q_bytes), ("normals", nrm, tab_bytes),
                                ("combined", both, tab_bytes + 2 * q_bytes)):
            up = upload_ms(nbytes)
            line[name] = dict(median_ms=round(t[0], 4), min_ms=round(t[1], 4), input_bytes=nbytes, upload_ms=round(up, 4), upload_share=round(up / t[0], 3))
        line["culled"] = host["culled"]
        line.update({k: round(v, 4) for k, v in host.items() if k.endswith("_ms")})
        print(json.dumps(line), flush=True)
