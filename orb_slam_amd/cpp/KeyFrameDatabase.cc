// ORB_SLAM::KeyFrameDatabase on the MI355X (drop-in for reference src/KeyFrameDatabase.cc).
//
// Each search is one device query (include/orbd.h) followed by host C++ for what walks KeyFrame objects:
//   1. the exclusion list, from a host scan of the stored key frames: in DetectLoopCandidates the connected key frames
//      (:78, :92-97) and, in both searches, those whose query id already equals this query's (:90, :207): the reference
//      neither resets nor lists those, it only keeps counting;
//   2. the device query: the key frames sharing words in lKFsSharingWords order, their counts, minCommonWords and the double
//      scores above it;
//   3. write-back of every field the reference writes — listed: m*Query = id, mn*Words = count; excluded and touched: the
//      stored count plus the shared words when the query id repeats, else (a connected key frame in loop mode) 1, because
//      the reference resets it on every touch (:92-101); scored: m*Score = (float)score;
//   4. the reference's own accumulation over GetBestCovisibilityKeyFrames(10), the 0.75 retain rule and the set
//      de-duplication, in float (:137-187, :252-307).  Its quirks follow from running that code on the written-back fields:
//      in relocalisation a covisible key frame that shares words but was not scored still adds its old mRelocScore
//      (:272-275 checks only mnRelocQuery).
// The whole search is one critical section under mMutex (the reference guards only the inverted-file walk), so concurrent
// searches from Tracking and LoopClosing see consistent fields; every host thread has a private stream, as in ORBmatcher.cc.
// There is no CPU fallback: without a usable GPU the constructor throws std::runtime_error.
#include "KeyFrameDatabase.h"

#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>

namespace ORB_SLAM {

namespace {

void require(int rc, const char* what) {
    if (rc != ORBX_OK) throw std::runtime_error(std::string("KeyFrameDatabase: ") + what + " failed (" + std::to_string(rc) + ")");
}

// a private stream per host thread and device
class ThreadStream {
public:
    explicit ThreadStream(int device) : device_(device) { require(orbx_stream_create(device, &stream_), "orbx_stream_create"); }
    ~ThreadStream() { (void)orbx_stream_destroy(device_, stream_); }
    void* get() const { return stream_; }

private:
    int device_;
    void* stream_ = nullptr;
};

void* thread_stream(int device) {
    thread_local std::map<int, std::unique_ptr<ThreadStream> > per_thread;
    std::unique_ptr<ThreadStream>& s = per_thread[device];
    if (!s) s.reset(new ThreadStream(device));
    return s->get();
}

// a BowVector as the two arrays of include/orbd.h (std::map order: word ids ascending)
void flatten(const DBoW2::BowVector& v, std::vector<uint32_t>& ids, std::vector<double>& vals) {
    ids.clear();
    vals.clear();
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
        ids.push_back(it->first);
        vals.push_back(it->second);
    }
}

// the device part of one search
struct Shared {
    std::vector<int32_t> slot, words, excl_words;
    std::vector<double> score;
    int min_common = 0;
};

void query(orbd_database* db, int device, int out_cap, const DBoW2::BowVector& bow, const std::vector<int32_t>& excl, Shared& r) {
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(bow, ids, vals);
    const int cap = out_cap > 0 ? out_cap : 1;
    r.slot.resize(cap);
    r.words.resize(cap);
    r.score.resize(cap);
    r.excl_words.assign(excl.size() > 0 ? excl.size() : 1, 0);
    int n = 0;
    require(orbd_query(db, ids.data(), vals.data(), (int)ids.size(), excl.data(), (int)excl.size(), r.excl_words.data(), r.slot.data(),
                       r.words.data(), r.score.data(), cap, &n, &r.min_common, thread_stream(device)),
            "orbd_query");
    r.slot.resize(n);
    r.words.resize(n);
    r.score.resize(n);
}

// The float tail both searches share (:137-187, :252-307): every scored key frame adds the scores of those of its ten best
// covisible key frames that `counts` admits, and hands on the best-scoring of them; the best sum (at least `floor`) times 0.75
// is the bar, and the handed-on key frames above it are returned once each, in order.
template <class Counts, class ScoreOf>
std::vector<KeyFrame*> accumulate(const std::vector<std::pair<float, KeyFrame*> >& scored, float floor, Counts counts, ScoreOf score_of) {
    std::vector<std::pair<float, KeyFrame*> > sums;
    sums.reserve(scored.size());
    float best_sum = floor;
    for (size_t i = 0; i < scored.size(); i++) {
        float sum = scored[i].first, top = scored[i].first;
        KeyFrame* top_kf = scored[i].second;
        const std::vector<KeyFrame*> neighbours = scored[i].second->GetBestCovisibilityKeyFrames(10);
        for (size_t k = 0; k < neighbours.size(); k++) {
            if (!counts(neighbours[k])) continue;
            const float s = score_of(neighbours[k]);
            sum += s;
            if (s > top) { top = s; top_kf = neighbours[k]; }
        }
        sums.push_back(std::make_pair(sum, top_kf));
        if (sum > best_sum) best_sum = sum;
    }
    const float bar = 0.75f * best_sum;
    std::set<KeyFrame*> seen;
    std::vector<KeyFrame*> out;
    for (size_t i = 0; i < sums.size(); i++)
        if (sums[i].first > bar && seen.insert(sums[i].second).second) out.push_back(sums[i].second);
    return out;
}

}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc, int capacity, int device) : mpVoc(&voc), mpDB(nullptr), mDevice(device) {
    require(orbd_create(voc.handle(), capacity, device, &mpDB), "orbd_create");
    mKeyFrameOf.assign(capacity, nullptr);
    mFreeSlots.reserve(capacity);
    for (int s = capacity - 1; s >= 0; s--) mFreeSlots.push_back(s);
}

KeyFrameDatabase::~KeyFrameDatabase() { orbd_destroy(mpDB); }

void KeyFrameDatabase::add(KeyFrame* pKF) {
    std::lock_guard<std::mutex> lock(mMutex);
    if (mSlotOf.count(pKF)) return;              // the one deviation: a second add without an erase is not stored twice
    if (mFreeSlots.empty()) throw std::runtime_error("KeyFrameDatabase: capacity exceeded");
    const int slot = mFreeSlots.back();
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(pKF->mBowVec, ids, vals);
    require(orbd_add(mpDB, slot, ids.data(), vals.data(), (int)ids.size()), "orbd_add");
    mFreeSlots.pop_back();
    mSlotOf[pKF] = slot;
    mKeyFrameOf[slot] = pKF;
}

void KeyFrameDatabase::erase(KeyFrame* pKF) {
    std::lock_guard<std::mutex> lock(mMutex);
    std::map<KeyFrame*, int>::iterator it = mSlotOf.find(pKF);
    if (it == mSlotOf.end()) return;             // :56-63 finds nothing to erase
    require(orbd_erase(mpDB, it->second), "orbd_erase");
    mKeyFrameOf[it->second] = nullptr;
    mFreeSlots.push_back(it->second);
    mSlotOf.erase(it);
}

void KeyFrameDatabase::clear() {
    std::lock_guard<std::mutex> lock(mMutex);
    require(orbd_clear(mpDB), "orbd_clear");
    for (std::map<KeyFrame*, int>::iterator it = mSlotOf.begin(); it != mSlotOf.end(); ++it) {
        mKeyFrameOf[it->second] = nullptr;
        mFreeSlots.push_back(it->second);
    }
    mSlotOf.clear();
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore) {
    const std::set<KeyFrame*> connected = pKF->GetConnectedKeyFrames();
    const unsigned long id = pKF->mnId;
    std::lock_guard<std::mutex> lock(mMutex);
    std::vector<int32_t> excl;
    for (std::map<KeyFrame*, int>::const_iterator it = mSlotOf.begin(); it != mSlotOf.end(); ++it)
        if (it->first->mnLoopQuery == id || connected.count(it->first)) excl.push_back(it->second);
    Shared r;
    query(mpDB, mDevice, (int)mSlotOf.size(), pKF->mBowVec, excl, r);

    for (size_t k = 0; k < excl.size(); k++) {
        if (r.excl_words[k] == 0) continue;
        KeyFrame* kf = mKeyFrameOf[excl[k]];
        if (kf->mnLoopQuery == id) kf->mnLoopWords += r.excl_words[k];
        else kf->mnLoopWords = 1;                 // connected: the count restarts on every touch (:92-101)
    }
    std::vector<std::pair<float, KeyFrame*> > scored;
    for (size_t j = 0; j < r.slot.size(); j++) {
        KeyFrame* kf = mKeyFrameOf[r.slot[j]];
        kf->mnLoopQuery = id;
        kf->mnLoopWords = r.words[j];
        if (r.words[j] > r.min_common) {
            const float si = (float)r.score[j];
            kf->mLoopScore = si;
            if (si >= minScore) scored.push_back(std::make_pair(si, kf));
        }
    }
    const int min_common = r.min_common;
    return accumulate(scored, minScore,
                      [&](const KeyFrame* n) { return n->mnLoopQuery == id && n->mnLoopWords > min_common; },      // :158
                      [](const KeyFrame* n) { return n->mLoopScore; });
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalisationCandidates(Frame* F) {
    const unsigned long id = F->mnId;
    std::lock_guard<std::mutex> lock(mMutex);
    std::vector<int32_t> excl;
    for (std::map<KeyFrame*, int>::const_iterator it = mSlotOf.begin(); it != mSlotOf.end(); ++it)
        if (it->first->mnRelocQuery == id) excl.push_back(it->second);
    Shared r;
    query(mpDB, mDevice, (int)mSlotOf.size(), F->mBowVec, excl, r);

    for (size_t k = 0; k < excl.size(); k++) mKeyFrameOf[excl[k]]->mnRelocWords += r.excl_words[k];
    std::vector<std::pair<float, KeyFrame*> > scored;
    for (size_t j = 0; j < r.slot.size(); j++) {
        KeyFrame* kf = mKeyFrameOf[r.slot[j]];
        kf->mnRelocQuery = id;
        kf->mnRelocWords = r.words[j];
        if (r.words[j] > r.min_common) {
            const float si = (float)r.score[j];
            kf->mRelocScore = si;
            scored.push_back(std::make_pair(si, kf));
        }
    }
    return accumulate(scored, 0.0f,
                      [&](const KeyFrame* n) { return n->mnRelocQuery == id; },      // :272-275: no count check, stale scores add
                      [](const KeyFrame* n) { return n->mRelocScore; });
}

}  // namespace ORB_SLAM
