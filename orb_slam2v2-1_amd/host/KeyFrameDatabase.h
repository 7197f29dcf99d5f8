// KeyFrameDatabase.h — ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:31-309) executed on an
// MI355X through include/orbx.h (orbv_db_*).  Keyframes are named by id (KeyFrame::mnId): the caller keeps KeyFrame* <-> id,
// hands the database each keyframe's mBowVec on add, its GetBestCovisibilityKeyFrames(10) as ids before a query that should
// see them, and the query's GetConnectedKeyFrames() as ids with the loop query.
#ifndef ORBX_KEYFRAMEDATABASE_H
#define ORBX_KEYFRAMEDATABASE_H
#include <set>
#include <vector>
#include "ORBVocabulary.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class KeyFrameDatabaseHIP {
public:
    // KeyFrameDatabase(const ORBVocabulary &voc) (:33-37); device: ORBX_DEVICE or 0.  Throws std::runtime_error without a GPU.
    explicit KeyFrameDatabaseHIP(const ORBVocabulary &voc);
    explicit KeyFrameDatabaseHIP(unsigned int nwords, int initial_entries = 0);
    ~KeyFrameDatabaseHIP();
    // every member throws std::runtime_error with orbx_last_error() when the library reports an error
    void add(int id, const DBoW2::BowVector &v);     // :40-46
    void erase(int id);                              // :48-67
    void clear();                                    // :69-73
    void SetCovisible(int id, const std::vector<int> &ids);   // pKF->GetBestCovisibilityKeyFrames(10) as ids, at most 10
    // :76-197; connected = pKF->GetConnectedKeyFrames() as ids
    std::vector<int> DetectLoopCandidates(const DBoW2::BowVector &v, const std::set<int> &connected, float minScore);
    // :199-309
    std::vector<int> DetectRelocalizationCandidates(const DBoW2::BowVector &v);
    // mpVoc->score(v, keyframe) for the listed keyframes (src/LoopClosing.cc:135-147)
    std::vector<double> Score(const DBoW2::BowVector &v, const std::vector<int> &ids);
    int size() const;                                // keyframes in the database
    orbv_db_t *handle() const { return mDb; }
private:
    KeyFrameDatabaseHIP(const KeyFrameDatabaseHIP &);
    KeyFrameDatabaseHIP &operator=(const KeyFrameDatabaseHIP &);
    void create(unsigned int nwords, int initial_entries);
    std::vector<int> detect(const DBoW2::BowVector &v, const std::set<int> *connected, float minScore);
    orbv_db_t *mDb;
};

}  // namespace ORB_SLAM2
#endif
