// orbx_kfdb.hip — the keyframe database: ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc:31-309) and
// TemplatedVocabulary::score with L1Scoring (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) on gfx950.
// No inverted file is materialised: every keyframe's BoW vector lies in one entry pool
// (word ids ascending, values), and a query intersects itself with every live keyframe.
//   k_db_intersect  one wave per keyframe, four per workgroup: the query's word ids staged in LDS, the keyframe's entries
//                   64 at a time, each lane bisects the query for its word; ballot -> common words, smallest common
//                   word; the L1 terms of the hit lanes are added to the wave's running double in ascending lane
//                   order (two 32-bit readlanes per term), which is the reference's sequential sum
//   k_db_mark       sets / clears the "connected to the query keyframe" flag of the listed slots (loop query)
//   k_db_select     one workgroup: maxCommonWords, the 0.8f threshold, scored / entered flags, the stale
//                   relocalisation scores, the covisibility accumulation (one lane per entry of lScoreAndMatch), and
//                   the records of the listed keyframes compacted in slot order by ballot prefix
// The tail (order by (smallest common word, sequence number), bestAccScore, the 0.75f rule, duplicates) runs on the
// host over those records: it only compares and selects.
#include "orbx_internal.h"
#include <math.h>
#include <algorithm>
#include <mutex>
#include <new>

#define DB_LIVE 1u
#define DB_LISTED 1u      // k_db_select's per-slot state
#define DB_SCORED 2u
#define DB_ENTERED 4u
#define DB_NCOV ORBV_DB_MAX_COVISIBLE

struct DbSlot { uint32_t off; int32_t len; uint32_t seq; int32_t kf_id; uint32_t flags; };
struct DbRec { int32_t kf_id, words; uint32_t flags; float score, acc; int32_t best_kf; uint32_t minword, seq; };

// ---- L1Scoring::score (ScoringObject.cpp:23-68): the lower_bound skips only move an iterator to the first id >= the
// other one, so the walk is a merge; the double sum runs over the common words in ascending id, one rounded operation
// at a time
static double score_l1(const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2) {
    double score = 0;
    int i = 0, j = 0;
    while (i < n1 && j < n2) {
        if (w1[i] == w2[j]) {
            const double vi = v1[i], wi = v2[j];
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            i++; j++;
        } else if (w1[i] < w2[j]) i++;
        else j++;
    }
    return -score / 2.0;
}

static int check_vector(const char *fn, const uint32_t *w, const double *v, int n, int64_t nwords) {
    if (n < 0 || (n > 0 && (!w || !v))) { orbx_set_error("%s: bad vector (n %d)", fn, n); return ORBX_ERR_ARG; }
    for (int i = 0; i < n; i++) {
        if (i > 0 && w[i] <= w[i - 1]) { orbx_set_error("%s: word ids not strictly ascending at %d", fn, i); return ORBX_ERR_ARG; }
        if (nwords >= 0 && (int64_t)w[i] >= nwords) { orbx_set_error("%s: word id %u at %d is not below %lld", fn, w[i], i, (long long)nwords); return ORBX_ERR_ARG; }
    }
    return ORBX_OK;
}

extern "C" int orbv_score_l1(const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2, double *out) {
    if (!out) { orbx_set_error("orbv_score_l1: NULL out"); return ORBX_ERR_ARG; }
    if (check_vector("orbv_score_l1", w1, v1, n1, -1) || check_vector("orbv_score_l1", w2, v2, n2, -1)) return ORBX_ERR_ARG;
    *out = score_l1(w1, v1, n1, w2, v2, n2);
    return ORBX_OK;
}

// ------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// list == NULL: wave j takes slot j (a query over the database); else slot list[j] (orbv_db_score)
__global__ __launch_bounds__(256) void k_db_intersect(const uint32_t *__restrict__ qw, const double *__restrict__ qv, int nq,
                                                      const uint32_t *__restrict__ pw, const double *__restrict__ pv,
                                                      const DbSlot *__restrict__ meta, const int32_t *__restrict__ list, int n,
                                                      int32_t *__restrict__ words, uint32_t *__restrict__ minword,
                                                      double *__restrict__ score) {
    __shared__ uint32_t sq[ORBV_DB_MAX_QUERY];
    for (int i = threadIdx.x; i < nq; i += 256) sq[i] = qw[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + wave;
    if (j >= n) return;
    const int slot = __builtin_amdgcn_readfirstlane(list ? list[j] : j);
    const DbSlot m = meta[slot];
    const int len = (m.flags & DB_LIVE) ? __builtin_amdgcn_readfirstlane(m.len) : 0;
    const uint32_t *kw = pw + m.off;
    const double *kv = pv + m.off;
    double s = 0;
    int cnt = 0;
    uint32_t first = 0xFFFFFFFFu;
    for (int base = 0; base < len; base += 64) {
        const int e = base + lane;
        bool hit = false;
        double term = 0;
        uint32_t w = 0;
        if (e < len) {
            w = kw[e];
            int lo = 0, hi = nq;                       // first query position whose id is >= w
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sq[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && sq[lo] == w) {
                hit = true;
                const double vi = qv[lo], wi = kv[e];  // v1 = the query, v2 = the keyframe   (KeyFrameDatabase.cc:133, :249)
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        unsigned long long b = __ballot(hit);
        if (b) {
            if (cnt == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)w, __builtin_amdgcn_readfirstlane(__builtin_ctzll(b)));
            cnt += __builtin_popcountll(b);
            while (b) {                                // ascending lane = ascending word id
                const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(b));
                s += readlane_f64(term, l);
                b &= b - 1;
            }
        }
    }
    if (lane == 0) { words[j] = cnt; minword[j] = first; score[j] = -s / 2.0; }
}

__global__ void k_db_mark(const int32_t *__restrict__ slots, int n, uint8_t value, uint8_t *__restrict__ conn) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) conn[slots[i]] = value;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// mode 0: DetectLoopCandidates (:76-173), mode 1: DetectRelocalizationCandidates (:199-287), both up to lAccScoreAndMatch
__global__ __launch_bounds__(256) void k_db_select(int nslots, int mode, float minScore, const DbSlot *__restrict__ meta,
                                                   const uint8_t *__restrict__ conn, const int32_t *__restrict__ cov,
                                                   const int32_t *__restrict__ id2slot, int idcap,
                                                   const int32_t *__restrict__ words, const uint32_t *__restrict__ minword,
                                                   const double *__restrict__ score, float *stale, uint8_t *state, float *sif,
                                                   DbRec *__restrict__ out, int32_t *__restrict__ head) {
    __shared__ int smax[4], scnt[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // lKFsSharingWords: live, not connected to the query keyframe, at least one common word; maxCommonWords over it
    int mx = 0;
    for (int i = tid; i < nslots; i += 256) {
        const bool listed = (meta[i].flags & DB_LIVE) && !conn[i] && words[i] > 0;
        state[i] = listed ? DB_LISTED : 0;
        if (listed && words[i] > mx) mx = words[i];
    }
    mx = wave_max_i32(mx);
    if (lane == 0) smax[wave] = mx;
    __syncthreads();
    const int maxCommon = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    const int minCommon = (int)((float)maxCommon * 0.8f);   // int minCommonWords = maxCommonWords*0.8f   (:120, :235)
    for (int i = tid; i < nslots; i += 256) {
        unsigned st = state[i];
        if (st && words[i] > minCommon) {
            const float si = (float)score[i];                // float si = mpVoc->score(...)
            st |= DB_SCORED;
            if (mode == 1 || si >= minScore) st |= DB_ENTERED;
            sif[i] = si;
            if (mode == 1) stale[i] = si;                    // pKFi->mRelocScore = si
            state[i] = (uint8_t)st;
        }
    }
    __threadfence_block();
    __syncthreads();
    int total = 0;
    for (int base = 0; base < nslots; base += 256) {
        const int i = base + tid;
        const unsigned st = i < nslots ? state[i] : 0;
        DbRec r = {};
        if (st) {
            const DbSlot m = meta[i];
            r.kf_id = m.kf_id; r.words = words[i]; r.flags = st >> 1; r.minword = minword[i]; r.seq = m.seq;
            r.score = (st & DB_SCORED) ? sif[i] : (mode == 1 ? stale[i] : 0.0f);
            r.acc = 0.0f; r.best_kf = -1;
            if (st & DB_ENTERED) {
                float best = r.score, acc = r.score;
                int bestkf = m.kf_id;
                const int32_t *c = cov + (size_t)i * (DB_NCOV + 1);
                const int nc = c[0];
                for (int k = 0; k < nc; k++) {
                    const int id = c[1 + k];
                    if (id < 0 || id >= idcap) continue;
                    const int s2 = id2slot[id];
                    if (s2 < 0) continue;                    // not in the database: its stamps never equal the query's
                    const unsigned st2 = state[s2];
                    float v;
                    if (mode == 0) {                         // mnLoopQuery == id && mnLoopWords > minCommonWords   (:159)
                        if (!(st2 & DB_SCORED)) continue;
                        v = sif[s2];
                    } else {                                 // mnRelocQuery == id   (:273): mRelocScore, fresh or stale
                        if (!(st2 & DB_LISTED)) continue;
                        v = stale[s2];
                    }
                    acc += v;
                    if (v > best) { best = v; bestkf = meta[s2].kf_id; }
                }
                r.acc = acc; r.best_kf = bestkf;
            }
        }
        const unsigned long long b = __ballot(st != 0);
        if (lane == 0) scnt[wave] = __builtin_popcountll(b);
        __syncthreads();
        int pos = total + __builtin_popcountll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) pos += scnt[w];
        if (st) out[pos] = r;
        total += scnt[0] + scnt[1] + scnt[2] + scnt[3];
        __syncthreads();
    }
    if (tid == 0) { head[0] = total; head[1] = maxCommon; head[2] = minCommon; }
}

// ------------------------------------------------------------------------------------
struct orbv_db {
    int nwords = 0, device = 0;
    std::mutex mu;
    hipStream_t stream = nullptr;
    // entry pool
    uint32_t *d_pw = nullptr; double *d_pv = nullptr; size_t poolCap = 0, poolUsed = 0, liveEntries = 0;
    // slot table (a slot per add since the last clear)
    DbSlot *d_meta = nullptr; int32_t *d_cov = nullptr; float *d_stale = nullptr; uint8_t *d_conn = nullptr; size_t slotCap = 0;
    std::vector<DbSlot> slots; int live = 0; uint32_t nextSeq = 0;
    int32_t *d_id2slot = nullptr; size_t idCap = 0; std::vector<int32_t> id2slot;
    // per-call scratch: query, slot list, per-wave results, records
    uint8_t *d_q = nullptr; size_t qCap = 0;
    uint8_t *h_pin = nullptr; size_t pinCap = 0;
    size_t devBytes = 0;
};

#define ALN(x) (((x) + 255) & ~(size_t)255)

static int db_free(orbv_db *db, void *p, size_t bytes) {
    if (p) { ORBX_HIP(hipFree(p)); db->devBytes -= bytes; }
    return ORBX_OK;
}
// device array of `elem`-byte elements: at least `need` of them, doubling, the first `keep` elements preserved, the rest
// set to byte `fill`
static int db_grow(orbv_db *db, void **p, size_t *cap, size_t need, size_t elem, size_t keep, int fill) {
    if (need <= *cap) return ORBX_OK;
    size_t nc = *cap ? *cap : 64;
    while (nc < need) nc *= 2;
    void *q = nullptr;
    ORBX_HIP(scratch_malloc(&q, nc * elem));
    db->devBytes += nc * elem;
    hipError_t e = hipSuccess;
    if (keep) e = hipMemcpyAsync(q, *p, keep * elem, hipMemcpyDeviceToDevice, db->stream);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)q + keep * elem, fill, (nc - keep) * elem, db->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) { hipFree(q); db->devBytes -= nc * elem; ORBX_HIP(e); }
    int rc = db_free(db, *p, *cap * elem);
    *p = q; *cap = nc;
    return rc;
}
static int db_pin(orbv_db *db, size_t need) {
    if (need <= db->pinCap) return ORBX_OK;
    size_t nc = db->pinCap ? db->pinCap : ((size_t)1 << 16);
    while (nc < need) nc *= 2;
    if (db->h_pin) { ORBX_HIP(hipHostFree(db->h_pin)); db->h_pin = nullptr; db->pinCap = 0; }
    ORBX_HIP(scratch_host_malloc((void **)&db->h_pin, nc, hipHostMallocDefault));
    db->pinCap = nc;
    return ORBX_OK;
}
// host -> device through the pinned buffer (at byte offset `at` of it), on the handle's stream
static int db_up(orbv_db *db, void *dst, const void *src, size_t bytes, size_t at) {
    if (!bytes) return ORBX_OK;
    memcpy(db->h_pin + at, src, bytes);
    ORBX_HIP(hipMemcpyAsync(dst, db->h_pin + at, bytes, hipMemcpyHostToDevice, db->stream));
    return ORBX_OK;
}

extern "C" void orbv_db_destroy(orbv_db_t *db) {
    if (!db) return;
    if (db->stream || db->d_pw || db->d_meta || db->d_id2slot || db->d_q || db->h_pin) {
        hipSetDevice(db->device);
        if (db->stream) { hipStreamSynchronize(db->stream); hipStreamDestroy(db->stream); }
        hipFree(db->d_pw); hipFree(db->d_pv); hipFree(db->d_meta); hipFree(db->d_cov); hipFree(db->d_stale); hipFree(db->d_conn);
        hipFree(db->d_id2slot); hipFree(db->d_q);
        if (db->h_pin) hipHostFree(db->h_pin);
    }
    delete db;
}

static int db_init(orbv_db *db, int initial_entries) {
    ORBX_HIP(hipSetDevice(db->device));
    ORBX_HIP(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    const size_t n0 = initial_entries > 0 ? (size_t)initial_entries : ((size_t)1 << 20);
    ORBX_HIP(scratch_malloc((void **)&db->d_pw, n0 * 4)); db->devBytes += n0 * 4;
    ORBX_HIP(scratch_malloc((void **)&db->d_pv, n0 * 8)); db->devBytes += n0 * 8;
    db->poolCap = n0;
    return db_pin(db, (size_t)1 << 16);
}

extern "C" int orbv_db_create(int nwords, int device, int initial_entries, orbv_db_t **out) {
    if (!out) { orbx_set_error("orbv_db_create: NULL out"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (nwords < 1 || initial_entries < 0 || device < 0) { orbx_set_error("orbv_db_create: bad arguments (nwords %d, device %d, initial_entries %d)", nwords, device, initial_entries); return ORBX_ERR_ARG; }
    orbv_db *db = new (std::nothrow) orbv_db();
    if (!db) { orbx_set_error("orbv_db_create: out of memory"); return ORBX_ERR_ARG; }
    db->nwords = nwords; db->device = device;
    const int rc = db_init(db, initial_entries);
    if (rc) { orbv_db_destroy(db); return rc; }
    *out = db;
    return ORBX_OK;
}

static int check_id(const char *fn, int kf_id) {
    if (kf_id < 0) { orbx_set_error("%s: negative keyframe id %d", fn, kf_id); return ORBX_ERR_ARG; }
    if (kf_id > ORBV_DB_MAX_KF_ID) { orbx_set_error("%s: keyframe id %d is above ORBV_DB_MAX_KF_ID", fn, kf_id); return ORBX_ERR_UNSUPPORTED; }
    return ORBX_OK;
}
static inline int slot_of(const orbv_db *db, int kf_id) {
    return kf_id >= 0 && (size_t)kf_id < db->id2slot.size() ? db->id2slot[kf_id] : -1;
}

// KeyFrameDatabase::add (:40-46)
extern "C" int orbv_db_add(orbv_db_t *db, int kf_id, const uint32_t *words, const double *values, int n) {
    if (!db) { orbx_set_error("orbv_db_add: NULL handle"); return ORBX_ERR_ARG; }
    int rc = check_id("orbv_db_add", kf_id);
    if (rc) return rc;
    if (check_vector("orbv_db_add", words, values, n, db->nwords)) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (slot_of(db, kf_id) >= 0) { orbx_set_error("orbv_db_add: keyframe %d is already in the database", kf_id); return ORBX_ERR_ARG; }
    if (db->poolUsed + (size_t)n > 0x7FFFFFFFu) { orbx_set_error("orbv_db_add: more than 2^31 - 1 pool entries"); return ORBX_ERR_UNSUPPORTED; }
    ORBX_HIP(hipSetDevice(db->device));
    const size_t slot = db->slots.size();
    if (db->poolUsed + n > db->poolCap) {
        size_t cap = db->poolCap, cap2 = db->poolCap;
        if ((rc = db_grow(db, (void **)&db->d_pw, &cap, db->poolUsed + n, 4, db->poolUsed, 0))) return rc;
        if ((rc = db_grow(db, (void **)&db->d_pv, &cap2, db->poolUsed + n, 8, db->poolUsed, 0))) return rc;
        db->poolCap = cap;
    }
    if (slot + 1 > db->slotCap) {
        size_t c1 = db->slotCap, c2 = db->slotCap, c3 = db->slotCap, c4 = db->slotCap;
        if ((rc = db_grow(db, (void **)&db->d_meta, &c1, slot + 1, sizeof(DbSlot), slot, 0))) return rc;
        if ((rc = db_grow(db, (void **)&db->d_cov, &c2, slot + 1, 4 * (DB_NCOV + 1), slot, 0))) return rc;
        if ((rc = db_grow(db, (void **)&db->d_stale, &c3, slot + 1, 4, slot, 0))) return rc;
        if ((rc = db_grow(db, (void **)&db->d_conn, &c4, slot + 1, 1, slot, 0))) return rc;
        db->slotCap = c1;
    }
    if ((size_t)kf_id >= db->idCap && (rc = db_grow(db, (void **)&db->d_id2slot, &db->idCap, (size_t)kf_id + 1, 4, db->idCap, 0xFF))) return rc;
    // the slot's covisible list and stale score are zero already: grown memory is zero-filled and a slot is used once
    const DbSlot m = {(uint32_t)db->poolUsed, n, db->nextSeq, kf_id, DB_LIVE};
    const int32_t s32 = (int32_t)slot;
    const size_t o_v = ALN((size_t)n * 4), o_m = o_v + ALN((size_t)n * 8), o_i = o_m + 256;
    if ((rc = db_pin(db, o_i + 256))) return rc;
    if ((rc = db_up(db, db->d_pw + db->poolUsed, words, (size_t)n * 4, 0))) return rc;
    if ((rc = db_up(db, db->d_pv + db->poolUsed, values, (size_t)n * 8, o_v))) return rc;
    if ((rc = db_up(db, db->d_meta + slot, &m, sizeof(m), o_m))) return rc;
    if ((rc = db_up(db, db->d_id2slot + kf_id, &s32, 4, o_i))) return rc;
    ORBX_HIP(hipStreamSynchronize(db->stream));
    db->slots.push_back(m);
    if ((size_t)kf_id >= db->id2slot.size()) db->id2slot.resize(std::max((size_t)kf_id + 1, db->id2slot.size() * 2), -1);
    db->id2slot[kf_id] = s32;
    db->poolUsed += n; db->liveEntries += n; db->live++; db->nextSeq++;
    return ORBX_OK;
}

// KeyFrameDatabase::erase (:48-67): an absent keyframe is in no list, nothing happens
extern "C" int orbv_db_erase(orbv_db_t *db, int kf_id) {
    if (!db) { orbx_set_error("orbv_db_erase: NULL handle"); return ORBX_ERR_ARG; }
    if (kf_id < 0) { orbx_set_error("orbv_db_erase: negative keyframe id %d", kf_id); return ORBX_ERR_ARG; }
    std::lock_guard<std::mutex> lock(db->mu);
    const int slot = slot_of(db, kf_id);
    if (slot < 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(db->device));
    DbSlot m = db->slots[slot];
    m.flags = 0;
    const int32_t none = -1;
    int rc;
    if ((rc = db_up(db, db->d_meta + slot, &m, sizeof(m), 0))) return rc;
    if ((rc = db_up(db, db->d_id2slot + kf_id, &none, 4, 256))) return rc;
    ORBX_HIP(hipStreamSynchronize(db->stream));
    db->slots[slot] = m;
    db->id2slot[kf_id] = -1;
    db->liveEntries -= m.len; db->live--;
    return ORBX_OK;
}

// KeyFrameDatabase::clear (:69-73)
extern "C" int orbv_db_clear(orbv_db_t *db) {
    if (!db) { orbx_set_error("orbv_db_clear: NULL handle"); return ORBX_ERR_ARG; }
    std::lock_guard<std::mutex> lock(db->mu);
    ORBX_HIP(hipSetDevice(db->device));
    if (db->slotCap) {
        ORBX_HIP(hipMemsetAsync(db->d_meta, 0, db->slotCap * sizeof(DbSlot), db->stream));
        ORBX_HIP(hipMemsetAsync(db->d_cov, 0, db->slotCap * 4 * (DB_NCOV + 1), db->stream));
        ORBX_HIP(hipMemsetAsync(db->d_stale, 0, db->slotCap * 4, db->stream));
        ORBX_HIP(hipMemsetAsync(db->d_conn, 0, db->slotCap, db->stream));
    }
    if (db->idCap) ORBX_HIP(hipMemsetAsync(db->d_id2slot, 0xFF, db->idCap * 4, db->stream));
    ORBX_HIP(hipStreamSynchronize(db->stream));
    db->slots.clear();
    std::fill(db->id2slot.begin(), db->id2slot.end(), -1);
    db->poolUsed = 0; db->liveEntries = 0; db->live = 0;
    return ORBX_OK;
}

// what GetBestCovisibilityKeyFrames(10) returns for the keyframe (:151, :265), as ids, in that order
extern "C" int orbv_db_set_covisible(orbv_db_t *db, int kf_id, const int32_t *ids, int n) {
    if (!db) { orbx_set_error("orbv_db_set_covisible: NULL handle"); return ORBX_ERR_ARG; }
    if (kf_id < 0) { orbx_set_error("orbv_db_set_covisible: negative keyframe id %d", kf_id); return ORBX_ERR_ARG; }
    if (n < 0 || n > DB_NCOV || (n > 0 && !ids)) { orbx_set_error("orbv_db_set_covisible: %d ids (0 .. %d)", n, DB_NCOV); return ORBX_ERR_ARG; }
    int32_t c[DB_NCOV + 1] = {n};
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0) { orbx_set_error("orbv_db_set_covisible: negative id at %d", i); return ORBX_ERR_ARG; }
        c[1 + i] = ids[i];
    }
    std::lock_guard<std::mutex> lock(db->mu);
    const int slot = slot_of(db, kf_id);
    if (slot < 0) { orbx_set_error("orbv_db_set_covisible: keyframe %d is not in the database", kf_id); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(db->device));
    const int rc = db_up(db, db->d_cov + (size_t)slot * (DB_NCOV + 1), c, sizeof(c), 0);
    if (rc) return rc;
    ORBX_HIP(hipStreamSynchronize(db->stream));
    return ORBX_OK;
}

extern "C" int orbv_db_info(const orbv_db_t *db, int *keyframes, int64_t *entries, int64_t *pool_entries, size_t *device_bytes) {
    if (!db) { orbx_set_error("orbv_db_info: NULL handle"); return ORBX_ERR_ARG; }
    std::lock_guard<std::mutex> lock(const_cast<orbv_db *>(db)->mu);
    if (keyframes) *keyframes = db->live;
    if (entries) *entries = (int64_t)db->liveEntries;
    if (pool_entries) *pool_entries = (int64_t)db->poolCap;
    if (device_bytes) *device_bytes = db->devBytes;
    return ORBX_OK;
}

static int check_query(const char *fn, const orbv_db *db, const uint32_t *qw, const double *qv, int nq) {
    if (!db) { orbx_set_error("%s: NULL handle", fn); return ORBX_ERR_ARG; }
    if (nq > ORBV_DB_MAX_QUERY) { orbx_set_error("%s: %d query words (ORBV_DB_MAX_QUERY is %d)", fn, nq, ORBV_DB_MAX_QUERY); return ORBX_ERR_UNSUPPORTED; }
    return check_vector(fn, qw, qv, nq, db->nwords);
}

// layout of the per-call device scratch for `n` waves: query | slot list | words | minword | score | state | sif | head | records
struct DbLayout { size_t qw, qv, list, words, minword, score, state, sif, head, rec, total; };
static DbLayout db_layout(size_t n) {
    DbLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += ALN(bytes); return o; };
    L.qw = take((size_t)ORBV_DB_MAX_QUERY * 4); L.qv = take((size_t)ORBV_DB_MAX_QUERY * 8); L.list = take(n * 4);
    L.words = take(n * 4); L.minword = take(n * 4); L.score = take(n * 8); L.state = take(n); L.sif = take(n * 4);
    L.head = take(16); L.rec = take(n * sizeof(DbRec));
    L.total = off;
    return L;
}
static int db_scratch(orbv_db *db, size_t n, DbLayout *L) {
    *L = db_layout(n);
    if (L->total > db->qCap) {
        // sized for twice the waves asked for, so that a growing database does not reallocate at every query
        const DbLayout L2 = db_layout(n * 2);
        int rc = db_free(db, db->d_q, db->qCap);
        db->d_q = nullptr; db->qCap = 0;
        if (rc) return rc;
        ORBX_HIP(scratch_malloc((void **)&db->d_q, L2.total));
        db->qCap = L2.total; db->devBytes += L2.total;
    }
    return ORBX_OK;
}

// mpVoc->score(query, keyframe) for the listed keyframes: the minScore loop of LoopClosing::DetectLoop (src/LoopClosing.cc:135-147)
extern "C" int orbv_db_score(orbv_db_t *db, const uint32_t *qw, const double *qv, int nq, const int32_t *kf_ids, int n, double *scores) {
    int rc = check_query("orbv_db_score", db, qw, qv, nq);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!kf_ids || !scores))) { orbx_set_error("orbv_db_score: bad arguments"); return ORBX_ERR_ARG; }
    if (n == 0) return ORBX_OK;
    std::lock_guard<std::mutex> lock(db->mu);
    std::vector<int32_t> list(n);
    for (int i = 0; i < n; i++) {
        list[i] = slot_of(db, kf_ids[i]);
        if (list[i] < 0) { orbx_set_error("orbv_db_score: keyframe %d (at %d) is not in the database", kf_ids[i], i); return ORBX_ERR_ARG; }
    }
    if (nq == 0) { for (int i = 0; i < n; i++) scores[i] = -0.0 / 2.0; return ORBX_OK; }   // no common word: score = -0/2.0
    ORBX_HIP(hipSetDevice(db->device));
    DbLayout L;
    if ((rc = db_scratch(db, n, &L))) return rc;
    const size_t p_qv = ALN((size_t)nq * 4), p_list = p_qv + ALN((size_t)nq * 8), p_out = p_list + ALN((size_t)n * 4);
    if ((rc = db_pin(db, p_out + (size_t)n * 8))) return rc;
    uint8_t *d = db->d_q;
    if ((rc = db_up(db, d + L.qw, qw, (size_t)nq * 4, 0)) || (rc = db_up(db, d + L.qv, qv, (size_t)nq * 8, p_qv)) ||
        (rc = db_up(db, d + L.list, list.data(), (size_t)n * 4, p_list))) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_db_intersect, dim3((n + 3) / 4), dim3(256), 0, db->stream, (const uint32_t *)(d + L.qw), (const double *)(d + L.qv), nq,
                       db->d_pw, db->d_pv, db->d_meta, (const int32_t *)(d + L.list), n, (int32_t *)(d + L.words),
                       (uint32_t *)(d + L.minword), (double *)(d + L.score));
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(db->h_pin + p_out, d + L.score, (size_t)n * 8, hipMemcpyDeviceToHost, db->stream));
    ORBX_HIP(hipStreamSynchronize(db->stream));
    memcpy(scores, db->h_pin + p_out, (size_t)n * 8);
    return ORBX_OK;
}

static int db_detect(const char *fn, orbv_db *db, int mode, const uint32_t *qw, const double *qv, int nq, const int32_t *connected,
                     int nconnected, float min_score, int32_t *cand, int cand_cap, int *ncand, orbv_db_hit_t *hits, int hit_cap,
                     int *nhits) {
    int rc = check_query(fn, db, qw, qv, nq);
    if (rc) return rc;
    if (!ncand || cand_cap < 0 || (cand_cap > 0 && !cand) || (hits && hit_cap < 0) || nconnected < 0 || (nconnected > 0 && !connected)) {
        orbx_set_error("%s: bad arguments", fn);
        return ORBX_ERR_ARG;
    }
    for (int i = 0; i < nconnected; i++)
        if (connected[i] < 0) { orbx_set_error("%s: negative connected id at %d", fn, i); return ORBX_ERR_ARG; }
    *ncand = 0;
    if (nhits) *nhits = 0;
    std::lock_guard<std::mutex> lock(db->mu);
    const int nslots = (int)db->slots.size();
    if (nq == 0 || db->live == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(db->device));
    std::vector<int32_t> conn;
    for (int i = 0; i < nconnected; i++) {
        const int s = slot_of(db, connected[i]);   // a connected keyframe that is not in the database is in no list anyway
        if (s >= 0) conn.push_back(s);
    }
    const int nconn = (int)conn.size();
    DbLayout L;
    if ((rc = db_scratch(db, std::max(nslots, nconn), &L))) return rc;
    const size_t p_qv = ALN((size_t)nq * 4), p_list = p_qv + ALN((size_t)nq * 8), p_head = p_list + ALN((size_t)nconn * 4), p_rec = p_head + 256;
    if ((rc = db_pin(db, p_rec + (size_t)nslots * sizeof(DbRec)))) return rc;
    uint8_t *d = db->d_q;
    if ((rc = db_up(db, d + L.qw, qw, (size_t)nq * 4, 0)) || (rc = db_up(db, d + L.qv, qv, (size_t)nq * 8, p_qv)) ||
        (rc = db_up(db, d + L.list, conn.data(), (size_t)nconn * 4, p_list))) return rc;
    (void)hipGetLastError();
    if (nconn) hipLaunchKernelGGL(k_db_mark, dim3((nconn + 255) / 256), dim3(256), 0, db->stream, (const int32_t *)(d + L.list), nconn, (uint8_t)1, db->d_conn);
    hipLaunchKernelGGL(k_db_intersect, dim3((nslots + 3) / 4), dim3(256), 0, db->stream, (const uint32_t *)(d + L.qw), (const double *)(d + L.qv), nq,
                       db->d_pw, db->d_pv, db->d_meta, (const int32_t *)nullptr, nslots, (int32_t *)(d + L.words),
                       (uint32_t *)(d + L.minword), (double *)(d + L.score));
    hipLaunchKernelGGL(k_db_select, dim3(1), dim3(256), 0, db->stream, nslots, mode, min_score, db->d_meta, db->d_conn, db->d_cov, db->d_id2slot,
                       (int)db->idCap, (const int32_t *)(d + L.words), (const uint32_t *)(d + L.minword), (const double *)(d + L.score),
                       db->d_stale, d + L.state, (float *)(d + L.sif), (DbRec *)(d + L.rec), (int32_t *)(d + L.head));
    if (nconn) hipLaunchKernelGGL(k_db_mark, dim3((nconn + 255) / 256), dim3(256), 0, db->stream, (const int32_t *)(d + L.list), nconn, (uint8_t)0, db->d_conn);
    ORBX_HIP(hipGetLastError());
    // head and records are adjacent in the scratch (L.rec = L.head + 256): one copy
    ORBX_HIP(hipMemcpyAsync(db->h_pin + p_head, d + L.head, 256 + (size_t)nslots * sizeof(DbRec), hipMemcpyDeviceToHost, db->stream));
    ORBX_HIP(hipStreamSynchronize(db->stream));
    const int nl = ((const int32_t *)(db->h_pin + p_head))[0];
    if (nl < 0 || nl > nslots) { orbx_set_error("%s: %d records for %d slots", fn, nl, nslots); return ORBX_ERR_HIP; }
    // lKFsSharingWords' order: ascending (smallest common word, position in that word's list = sequence of the add)
    std::vector<DbRec> rec((const DbRec *)(db->h_pin + p_rec), (const DbRec *)(db->h_pin + p_rec) + nl);
    std::sort(rec.begin(), rec.end(), [](const DbRec &a, const DbRec &b) { return a.minword != b.minword ? a.minword < b.minword : a.seq < b.seq; });
    float bestAcc = mode == 0 ? min_score : 0.0f;                  // :145, :259
    for (const DbRec &r : rec)
        if ((r.flags & 2u) && r.acc > bestAcc) bestAcc = r.acc;
    const float minScoreToRetain = 0.75f * bestAcc;                // :176, :290
    std::vector<int32_t> out;
    for (const DbRec &r : rec)
        if ((r.flags & 2u) && r.acc > minScoreToRetain && std::find(out.begin(), out.end(), r.best_kf) == out.end()) out.push_back(r.best_kf);
    *ncand = (int)out.size();
    if (nhits) *nhits = nl;
    if ((int)out.size() > cand_cap || (hits && nl > hit_cap)) {
        orbx_set_error("%s: %d candidates / %d listed keyframes do not fit the capacities %d / %d", fn, (int)out.size(), nl, cand_cap, hits ? hit_cap : 0);
        return ORBX_ERR_ARG;
    }
    for (size_t i = 0; i < out.size(); i++) cand[i] = out[i];
    if (hits)
        for (int i = 0; i < nl; i++) {
            const DbRec &r = rec[i];
            const orbv_db_hit_t h = {r.kf_id, r.words, r.flags, r.score, r.acc, r.best_kf};
            hits[i] = h;
        }
    return ORBX_OK;
}

extern "C" int orbv_db_detect_loop(orbv_db_t *db, const uint32_t *qw, const double *qv, int nq, const int32_t *connected, int nconnected,
                                   float min_score, int32_t *cand, int cand_cap, int *ncand, orbv_db_hit_t *hits, int hit_cap, int *nhits) {
    return db_detect("orbv_db_detect_loop", db, 0, qw, qv, nq, connected, nconnected, min_score, cand, cand_cap, ncand, hits, hit_cap, nhits);
}

extern "C" int orbv_db_detect_reloc(orbv_db_t *db, const uint32_t *qw, const double *qv, int nq, int32_t *cand, int cand_cap, int *ncand,
                                    orbv_db_hit_t *hits, int hit_cap, int *nhits) {
    return db_detect("orbv_db_detect_reloc", db, 1, qw, qv, nq, nullptr, 0, 0.0f, cand, cand_cap, ncand, hits, hit_cap, nhits);
}
