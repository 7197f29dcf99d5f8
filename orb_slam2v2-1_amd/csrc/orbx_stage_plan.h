// orbx_stage_plan.h — the HIP-free half of orbx_stage.h: how one call lays its arrays out inside a staging block.  orbx_stage.h
// includes it; the lockstep programs (tests/cpp/lba_lockstep.cc, essential_lockstep.cc), which compile a driver for the host
// without the HIP runtime, get it through orbx_lba.hip / orbx_essential.hip alone.
#pragma once
#include <stddef.h>

static inline size_t stage_align(size_t x) { return (x + 255) & ~(size_t)255; }

// layout of one call inside a StagePair: take() hands out 256-B aligned offsets; everything taken before mark_inputs() is
// uploaded in one copy; off is then the call's need
struct StagePlan {
    size_t off = 0, in_end = 0;
    size_t take(size_t bytes) { const size_t o = off; off += stage_align(bytes); return o; }
    void mark_inputs() { in_end = off; }
};
