// orbx_mapcorrect_plan.h — the graph work of orbr_spread_global_ba, on the host and HIP-free: the checks of the child lists and origins,
// the walk of src/LoopClosing.cc:686-709 as a breadth-first pass over the CHILD LISTS (a bad keyframe keeps its mpParent but is in
// nobody's child set, src/KeyFrame.cc:480-539: parents are derived from the lists, never read), and the launch levels of the keyframes
// outside the global BA.  orbx_mapcorrect.hip runs it in its packing pass; tests/cpp/mapcorrect_lockstep.cc compiles the same text.
#pragma once
#include <stdint.h>
#include <vector>
#include "orbx.h"

struct McSpreadPlan {
    std::vector<int32_t> parent;           // [K] the keyframe whose child list holds this one, -1 for none
    std::vector<uint8_t> reached, marked;  // [K] popped by the walk; mnBAGlobalForKF == nLoopKF after it
    std::vector<int32_t> order, first;     // the reached keyframes outside the global BA by level: level l is order[first[l] .. first[l + 1]), l = 1 .. levels
    int levels = 0;
    const char *what = nullptr;            // a failed check: its words, where and the value
    long long at = 0, v = 0;
    bool fail(const char *w, long long a, long long b) { what = w; at = a; v = b; return false; }
};

// false: an argument error, described in plan.what / at / v.  Pointers and sizes have been checked by the caller
static inline bool mc_plan_spread(const orbr_spread_in_t *in, McSpreadPlan &pl) {
    const int K = in->K, P = in->P;
    if (in->child_off[0] != 0) return pl.fail("child_off does not start at 0", 0, in->child_off[0]);
    for (int k = 0; k < K; k++)
        if (in->child_off[k + 1] < in->child_off[k]) return pl.fail("child_off decreases", k + 1, in->child_off[k + 1]);
    if (in->child_off[K] > 0 && !in->child) return pl.fail("child is NULL", 0, 0);
    pl.parent.assign((size_t)K, -1);
    for (int k = 0; k < K; k++)
        for (int i = in->child_off[k]; i < in->child_off[k + 1]; i++) {
            const int c = in->child[i];
            if (c < 0 || c >= K) return pl.fail("child slot out of range", i, c);
            if (c == k) return pl.fail("a keyframe is in its own child list", i, c);
            if (pl.parent[c] >= 0) return pl.fail("a keyframe is in two child lists", i, c);
            pl.parent[c] = k;
        }
    for (int p = 0; p < P; p++)
        if (in->ref_kf[p] < -1 || in->ref_kf[p] >= K) return pl.fail("ref_kf out of range", p, in->ref_kf[p]);
    pl.reached.assign((size_t)K, 0);
    pl.marked.assign((size_t)K, 0);
    std::vector<int32_t> level((size_t)K, 0), queue;
    queue.reserve((size_t)K);
    for (int i = 0; i < in->n_origins; i++) {
        const int o = in->origins[i];
        if (o < 0 || o >= K) return pl.fail("origin out of range", i, o);
        if (pl.parent[o] >= 0) return pl.fail("an origin is in a child list", i, o);
        if (pl.reached[o]) return pl.fail("an origin is repeated", i, o);
        if (!in->kf_in_gba[o]) return pl.fail("an origin is outside the global BA", i, o);
        pl.reached[o] = 1;
        queue.push_back(o);
    }
    int nlev = 0;
    for (size_t hd = 0; hd < queue.size(); hd++) {   // every keyframe has one parent and no origin has one: each is pushed once
        const int k = queue[hd];
        for (int i = in->child_off[k]; i < in->child_off[k + 1]; i++) {
            const int c = in->child[i];
            pl.reached[c] = 1;
            level[c] = in->kf_in_gba[c] ? 0 : level[k] + 1;   // the distance to the nearest reached ancestor inside the global BA
            if (level[c] > nlev) nlev = level[c];
            queue.push_back(c);
        }
    }
    for (int k = 0; k < K; k++) pl.marked[k] = in->kf_in_gba[k] || pl.reached[k];
    // a counting sort that keeps the walk's order inside a level
    pl.first.assign((size_t)nlev + 2, 0);
    for (size_t i = 0; i < queue.size(); i++)
        if (level[queue[i]] > 0) pl.first[level[queue[i]] + 1]++;
    for (int l = 1; l <= nlev + 1; l++) pl.first[l] += pl.first[l - 1];
    pl.order.resize((size_t)pl.first[nlev + 1]);
    std::vector<int32_t> at(pl.first.begin(), pl.first.end());
    for (size_t i = 0; i < queue.size(); i++) {
        const int k = queue[i];
        if (level[k] > 0) pl.order[at[level[k]]++] = k;
    }
    pl.levels = nlev;
    return true;
}
