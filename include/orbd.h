/* orbd.h — C ABI of the MI355X-native key-frame database (part of liborbx.so).
 *
 * The map-sized half of ORB_SLAM's KeyFrameDatabase: the word -> key frame inverted file lives in HBM next to the
 * BowVectors that orbv_transform_batch_device leaves there, and one query counts the shared words of every stored key
 * frame, takes the 0.8 * max threshold and scores the survivors.  What walks KeyFrame objects (covisibility
 * accumulation, the 0.75 retain rule, write-back of the KeyFrame fields) stays in host C++:
 * orb_slam_amd/cpp/KeyFrameDatabase.cc.
 *
 * Reference interfaces replaced (paths relative to the reference ORB_SLAM tree):
 *   orbd_create / orbd_destroy  <- KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary&)   src/KeyFrameDatabase.cc:32-36
 *   orbd_add[_batch_device]     <- KeyFrameDatabase::add(KeyFrame*)                            src/KeyFrameDatabase.cc:39-45
 *   orbd_erase                  <- KeyFrameDatabase::erase(KeyFrame*)                          src/KeyFrameDatabase.cc:47-66
 *   orbd_clear                  <- KeyFrameDatabase::clear()                                   src/KeyFrameDatabase.cc:68-72
 *   orbd_query[_batch_device]   <- the inverted-file walk, the common-word threshold and the scores of
 *                                  DetectLoopCandidates (src/KeyFrameDatabase.cc:86-134) and
 *                                  DetectRelocalisationCandidates (src/KeyFrameDatabase.cc:203-250)
 *
 * Key frames are named by caller-chosen slots 0 <= slot < capacity.  A BowVector is two parallel arrays (word ids
 * strictly ascending, double values), laid out as orbv_transform* writes them.
 *
 * Order of the candidate list.  The reference lists a key frame when the walk first touches it: query words in
 * ascending order, each word's inverted list in add order (push_back at :44; erase removes the first occurrence, so an
 * erased and re-added key frame goes to the end).  The list is therefore ordered by (rank of the first shared query
 * word, add sequence), which is what the query returns.
 *
 * Scores are bit-equal to orbv_score(query, key frame): one sequential double sum in ascending word order
 * (DBoW2/ScoringObject.cpp), from the same __host__ __device__ code (orb_slam_amd/csrc/orbv_score.h).  L1, L2,
 * chi-square, Bhattacharyya and dot product are supported; KL gives ORBX_ERR_ARG at create time.
 *
 * Thread safety: a database handle may be used from several host threads; its state is guarded by one mutex, and all
 * device work on it is chained across the callers' streams with events, so an add on one stream is seen by a later
 * query on another.  Every entry point selects the database's device itself and restores the caller's current device.
 * Status codes are orbx.h's; there is no CPU fallback: without a usable GPU every compute entry point returns
 * ORBX_ERR_DEVICE.
 */
#ifndef ORBD_H
#define ORBD_H

#include <stddef.h>
#include <stdint.h>

#include "orbv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBD_MAX_CAPACITY (1 << 22)   /* slots of one database */

typedef struct orbd_database orbd_database;

/* Scoring type and word count come from the vocabulary, which must outlive the database.  ORBX_ERR_ARG for a NULL
 * vocabulary, capacity outside [1, ORBD_MAX_CAPACITY] or the KL scoring type; ORBX_ERR_DEVICE without a usable GPU.
 * Device memory: 12 bytes per slot, plus the stored words (16 bytes each, with an add's reservation: n words for
 * orbd_add, `cap` for orbd_add_batch_device) and the inverted file. */
int orbd_create(const orbv_vocabulary* voc, int capacity, int device, orbd_database** out);
void orbd_destroy(orbd_database* db);
/* stored key frames (present slots) */
int orbd_size(const orbd_database* db);

/* add(pKF): host pointers, synchronous.  ORBX_ERR_ARG for a slot out of range or already present, n < 0, an id >= the
 * vocabulary's word count or ids that are not strictly ascending; the database is then unchanged. */
int orbd_add(orbd_database* db, int slot, const uint32_t* ids, const double* vals, int n);
/* add() for nframes key frames whose BowVectors are on the device: frame f has d_n_bow[f] words at offset f*cap, the
 * layout of orbv_transform_batch_device; it is stored in slots[f] (host array), added in frame order.  The slots are
 * checked on the host (ORBX_ERR_ARG: out of range, present, or repeated; nothing is added).  The words are checked on
 * the device: d_status[f] (optional device buffer) receives ORBX_OK, or ORBX_ERR_ARG for d_n_bow[f] outside [0, cap],
 * an id out of range or ids not ascending; such a slot stays present with an empty BowVector until it is erased.
 * Asynchronous on `stream` (the inputs are read when the stream reaches the call), except that an add that does not fit
 * the stored-word arena grows it first, synchronously: the live BowVectors are copied into an arena twice their size. */
int orbd_add_batch_device(orbd_database* db, const int32_t* slots, int nframes, const uint32_t* d_bow_id, const double* d_bow_val,
                          const int32_t* d_n_bow, int cap, int32_t* d_status, void* stream);
/* erase(pKF): an absent slot is a no-op, as in the reference.  clear(): every slot absent. */
int orbd_erase(orbd_database* db, int slot);
int orbd_clear(orbd_database* db);

/* The map-sized part of both Detect functions for nq query BowVectors (query q: d_n_bow[q] words at offset q*qcap).
 * All arrays are device buffers; outputs of query q at offset q*out_cap.
 *   d_excl_off[nq+1] / d_excl_slot: per-query exclusion list (CSR; both may be NULL): these slots are not listed, and
 *       d_excl_words[k] (may be NULL when there are no exclusions) receives the shared-word count of d_excl_slot[k].
 *   d_share_slot:  the listed key frames in the order of lKFsSharingWords (:86-104, :203-222).
 *   d_share_words: the shared-word count of each (mnLoopWords / mnRelocWords).
 *   d_min_common[q]: (int)(maxCommonWords * 0.8f) over the listed slots (:113-120, :228-234); 0 when none is listed.
 *   d_share_score: score(query, key frame) of every listed slot whose count is > d_min_common[q], else 0.
 *   d_n_share[q]: the number of listed slots.
 *   d_status[q]: ORBX_OK; ORBX_ERR_CAPACITY when d_n_share[q] > out_cap (the lists are then not written);
 *       ORBX_ERR_ARG for d_n_bow[q] outside [0, qcap], a bad query word, or an excluded slot outside [0, capacity).
 * Asynchronous on `stream`; never blocks the host and allocates nothing. */
int orbd_query_batch_device(orbd_database* db, int nq, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_n_bow, int qcap,
                            const int32_t* d_excl_off, const int32_t* d_excl_slot, int32_t* d_excl_words, int32_t* d_share_slot,
                            int32_t* d_share_words, double* d_share_score, int out_cap, int32_t* d_n_share, int32_t* d_min_common,
                            int32_t* d_status, void* stream);
/* One query, host pointers, synchronous (stream NULL: the database's own stream).  Returns the query's status; with
 * ORBX_ERR_CAPACITY, *n_share holds the true count.  excl_words may be NULL when n_excl == 0. */
int orbd_query(orbd_database* db, const uint32_t* ids, const double* vals, int n, const int32_t* excl_slot, int n_excl,
               int32_t* excl_words, int32_t* share_slot, int32_t* share_words, double* share_score, int out_cap, int* n_share,
               int* min_common, void* stream);

#ifdef __cplusplus
}
#endif
#endif
