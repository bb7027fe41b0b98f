// ORB_SLAM::KeyFrameDatabase on the MI355X C ABI — the reference's class surface (reference include/KeyFrameDatabase.h:38-53):
// the constructor, add / erase / clear and the two candidate searches with the reference's signatures.  Drop-in for
// include/KeyFrameDatabase.h + src/KeyFrameDatabase.cc: compile KeyFrameDatabase.cc into the project with the SLAM headers on the
// include path and link liborbx.so.
//
// The inverted file and the map-sized part of both searches (shared-word counts, the 0.8 * max threshold, the scores) run on
// the device (include/orbd.h); KeyFrameDatabase.cc walks the KeyFrame objects: it builds the exclusion list, writes back every
// field the reference writes, and accumulates the covisibility scores exactly as the reference does.  It uses only public
// KeyFrame / Frame members: mnId, mBowVec, mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore
// (include/KeyFrame.h:160-165), GetConnectedKeyFrames and GetBestCovisibilityKeyFrames.
//
// One documented deviation: adding the same KeyFrame* twice without an erase in between stores it once (the reference would
// list it twice).  ORB_SLAM adds each key frame exactly once.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "orbd.h"
#include "orbx.h"
#include "ORBVocabulary.h"
#include "KeyFrame.h"
#include "Frame.h"

namespace ORB_SLAM {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    // reference :32-36; `capacity` = the most key frames stored at once, `device` = the GPU the database lives on
    explicit KeyFrameDatabase(const ORBVocabulary& voc, int capacity = 65536, int device = 0);
    ~KeyFrameDatabase();
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFrame* pKF);       // :39-45
    void erase(KeyFrame* pKF);     // :47-66
    void clear();                  // :68-72

    // Loop Detection (:75-187)
    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore);
    // Relocalisation (:189-307)
    std::vector<KeyFrame*> DetectRelocalisationCandidates(Frame* F);

protected:
    // Associated vocabulary
    const ORBVocabulary* mpVoc;
    orbd_database* mpDB;
    int mDevice;
    // slot bookkeeping: KeyFrame* <-> slot of the device database
    std::map<KeyFrame*, int> mSlotOf;
    std::vector<KeyFrame*> mKeyFrameOf;
    std::vector<int> mFreeSlots;
    // Mutex: guards the slots, the device database and the KeyFrame fields a search writes
    std::mutex mMutex;
};

}  // namespace ORB_SLAM
