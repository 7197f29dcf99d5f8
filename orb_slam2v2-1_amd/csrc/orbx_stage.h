// orbx_stage.h — the per-host-thread staging pair: a device scratch block, a pinned host mirror of the same
// layout and a non-blocking stream, grow-only.  An entry point lays its arrays out with StagePlan (orbx_stage_plan.h), fills the mirror, moves its
// inputs with ONE upload and its results with ONE download + ONE synchronisation of that stream: no hipMalloc per call and no
// device-wide synchronisation, so other threads' extractors and matchers keep running (the reference's Tracking / LocalMapping /
// LoopClosing threads call matchers and solvers concurrently, src/LocalMapping.cc:223, src/LoopClosing.cc:249).
// Users, each with a `static thread_local StagePair` of its own: orbx_match.hip, orbx_poseopt.hip, orbx_initializer.hip,
// orbx_sim3.hip, orbx_pnp.hip, orbx_sim3opt.hip, orbx_newpoints.hip, orbx_lba.hip, orbx_essential.hip, orbx_covis.hip, orbx_mapcorrect.hip.
#pragma once
#include "orbx_internal.h"
#include "orbx_stage_plan.h"   // stage_align, StagePlan: no HIP in them

struct StagePair {
    uint8_t *d = nullptr, *h = nullptr; size_t cap = 0; int device = -1; hipStream_t stream = nullptr;
    // a thread that holds nothing makes no HIP call
    void release() {
        if (device < 0) return;
        hipSetDevice(device);
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
        if (d) hipFree(d);
        if (h) hipHostFree(h);
        *this = StagePair();
    }
    // leaves `dev` current.  Another device: everything goes.  More than cap: d and h are freed and allocated again at
    // max(2 * need, min_cap), the stream stays
    int reserve(int dev, size_t need, size_t min_cap) {
        if (device != dev) release();
        ORBX_HIP(hipSetDevice(dev));
        if (device < 0) {
            ORBX_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            device = dev;
        }
        if (cap >= need) return ORBX_OK;
        if (d) { hipFree(d); d = nullptr; }
        if (h) { hipHostFree(h); h = nullptr; }
        cap = 0;
        const size_t c = need * 2 > min_cap ? need * 2 : min_cap;
        ORBX_HIP(scratch_malloc(&d, c));
        ORBX_HIP(scratch_host_malloc((void **)&h, c, hipHostMallocDefault));
        cap = c;
        return ORBX_OK;
    }
};
