// KeyFrameDatabase.cc — see KeyFrameDatabase.h
#include "KeyFrameDatabase.h"
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace ORB_SLAM2 {

namespace {
void check(int rc, const char *what) {
    if (rc != ORBX_OK) throw std::runtime_error(std::string(what) + ": " + orbx_last_error());
}
// a DBoW2::BowVector is a std::map: its iteration order is ascending word id
void flatten(const DBoW2::BowVector &v, std::vector<uint32_t> &w, std::vector<double> &x) {
    w.clear(); x.clear();
    w.reserve(v.size()); x.reserve(v.size());
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { w.push_back(it->first); x.push_back(it->second); }
}
}  // namespace

void KeyFrameDatabaseHIP::create(unsigned int nwords, int initial_entries) {
    const int device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;
    check(orbv_db_create((int)nwords, device, initial_entries, &mDb), "KeyFrameDatabaseHIP");
}

KeyFrameDatabaseHIP::KeyFrameDatabaseHIP(const ORBVocabulary &voc) : mDb(NULL) { create(voc.size(), 0); }
KeyFrameDatabaseHIP::KeyFrameDatabaseHIP(unsigned int nwords, int initial_entries) : mDb(NULL) { create(nwords, initial_entries); }
KeyFrameDatabaseHIP::~KeyFrameDatabaseHIP() { if (mDb) orbv_db_destroy(mDb); }

void KeyFrameDatabaseHIP::add(int id, const DBoW2::BowVector &v) {
    std::vector<uint32_t> w; std::vector<double> x;
    flatten(v, w, x);
    check(orbv_db_add(mDb, id, w.data(), x.data(), (int)w.size()), "KeyFrameDatabaseHIP::add");
}

void KeyFrameDatabaseHIP::erase(int id) { check(orbv_db_erase(mDb, id), "KeyFrameDatabaseHIP::erase"); }
void KeyFrameDatabaseHIP::clear() { check(orbv_db_clear(mDb), "KeyFrameDatabaseHIP::clear"); }

void KeyFrameDatabaseHIP::SetCovisible(int id, const std::vector<int> &ids) {
    std::vector<int32_t> a(ids.begin(), ids.end());
    check(orbv_db_set_covisible(mDb, id, a.data(), (int)a.size()), "KeyFrameDatabaseHIP::SetCovisible");
}

int KeyFrameDatabaseHIP::size() const {
    int n = 0;
    check(orbv_db_info(mDb, &n, NULL, NULL, NULL), "KeyFrameDatabaseHIP::size");
    return n;
}

std::vector<int> KeyFrameDatabaseHIP::detect(const DBoW2::BowVector &v, const std::set<int> *connected, float minScore) {
    std::vector<uint32_t> w; std::vector<double> x;
    flatten(v, w, x);
    std::vector<int32_t> conn;
    if (connected) conn.assign(connected->begin(), connected->end());
    std::vector<int32_t> cand((size_t)size() + 1);   // a candidate is a keyframe of the database, listed once
    const char *what = connected ? "KeyFrameDatabaseHIP::DetectLoopCandidates" : "KeyFrameDatabaseHIP::DetectRelocalizationCandidates";
    int n = 0;
    for (int attempt = 0;; attempt++) {
        const int rc = connected ? orbv_db_detect_loop(mDb, w.data(), x.data(), (int)w.size(), conn.data(), (int)conn.size(), minScore,
                                                       cand.data(), (int)cand.size(), &n, NULL, 0, NULL)
                                 : orbv_db_detect_reloc(mDb, w.data(), x.data(), (int)w.size(), cand.data(), (int)cand.size(), &n, NULL, 0, NULL);
        // another thread added keyframes between size() and the query: the call reports the count it needs
        if (rc == ORBX_ERR_ARG && n > (int)cand.size() && attempt < 4) { cand.resize((size_t)n * 2); continue; }
        check(rc, what);
        break;
    }
    return std::vector<int>(cand.begin(), cand.begin() + n);
}

std::vector<int> KeyFrameDatabaseHIP::DetectLoopCandidates(const DBoW2::BowVector &v, const std::set<int> &connected, float minScore) {
    return detect(v, &connected, minScore);
}

std::vector<int> KeyFrameDatabaseHIP::DetectRelocalizationCandidates(const DBoW2::BowVector &v) { return detect(v, NULL, 0.0f); }

std::vector<double> KeyFrameDatabaseHIP::Score(const DBoW2::BowVector &v, const std::vector<int> &ids) {
    std::vector<uint32_t> w; std::vector<double> x;
    flatten(v, w, x);
    std::vector<int32_t> a(ids.begin(), ids.end());
    std::vector<double> s(a.size());
    check(orbv_db_score(mDb, w.data(), x.data(), (int)w.size(), a.data(), (int)a.size(), s.data()), "KeyFrameDatabaseHIP::Score");
    return s;
}

}  // namespace ORB_SLAM2
