/*
 * orbgpu_kfdb.h -- C ABI of the keyframe database on the device:
 * KeyFrameDatabase::DetectRelocalizationCandidates and DetectLoopCandidates for
 * a batch of queries, with the minScore of LoopClosing::DetectLoop, and the glue
 * that turns the relocalisation candidates into the tables of orbgpu_reloc.h.
 * With it the chain Frame::ComputeBoW -> DetectRelocalizationCandidates ->
 * SearchByBoW -> PnPsolver set-up -> candidate loop is calls on one stream with
 * nothing downloaded, built or uploaded between them.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   KeyFrameDatabase::DetectLoopCandidates            src/KeyFrameDatabase.cpp:96-226
 *   KeyFrameDatabase::DetectRelocalizationCandidates  src/KeyFrameDatabase.cpp:239-361
 *   LoopClosing::DetectLoop, minScore                 src/LoopClosing.cpp:136-151
 *   Tracking::Relocalization, the candidates          src/Tracking.cpp:1756, :1781
 *
 * The rule is the reference's result, quirks kept:
 *   - no inverted file: mvInvertedFile[w] is the keyframes that hold word w, added
 *     and not erased, in add() order, and a keyframe's mBowVec never changes after
 *     add().  lKFsSharingWords is therefore the in_db keyframes that share a word
 *     with the query, ordered by (index in the query BowVector of the first word
 *     they share, add_rank); mnRelocWords / mnLoopWords is the size of the
 *     intersection; the mnRelocQuery / mnLoopQuery marks are fresh for every query;
 *   - LOOP: keyframes in `connected` never enter the list and never count as a
 *     neighbour; maxCommonWords is over the list; minCommonWords =
 *     (int)(maxCommonWords * 0.8f); si = (float)score and an entry is kept when
 *     si >= minScore; a neighbour adds its score when it is in the list with
 *     words > minCommonWords, even if its own si < minScore (mLoopScore is set
 *     before that test); bestAccScore starts at minScore;
 *   - minScore of DetectLoop: with n_covisible >= 0 it is the float 1 lowered by
 *     (float)score(query, mBowVec[k]) over the covisibles that are not kf_bad,
 *     whether they are in_db or not, and the query's min_score is ignored;
 *   - RELOC: a neighbour that shares a word adds mRelocScore and competes for
 *     pBestKF even when its words <= minCommonWords (:323-331).  That value was
 *     written by an earlier query, or never.  It is reloc_score[k]: read for
 *     such a neighbour, written for every keyframe the query scores.  A batch
 *     behaves as the reference called once per query in batch order: a stale read
 *     sees the latest earlier RELOC query of the batch that scored the keyframe,
 *     otherwise the value the array held at the call.  A query's outputs do not
 *     depend on how the queries are split over calls; they do depend on the
 *     queries before them.  LOOP queries neither read nor write the array;
 *   - accScore is a float sum in covis order, the threshold 0.75f * bestAccScore,
 *     every comparison the reference's (strict > for the maxima and the retain);
 *   - the retain runs in list order: an entry passes when accScore >
 *     minScoreToRetain and its pBestKF has not been emitted yet;
 *   - an empty list or an empty lScoreAndMatch gives no candidates, status OK,
 *     best_acc_score its initial value (minScore for LOOP, 0 for RELOC) and the
 *     counts the reference never reached zero.
 *
 * Scores are TemplatedVocabulary::score in double, the terms added in ascending
 * word order as orbgpu_bow_score does (bit-exact for scoring 0, 1, 2, 4, 5; KL
 * uses the device log), then rounded to float.  Everything else is integers and
 * float comparisons: integer atomics and prefix sums only, so every output is a
 * function of the inputs alone.
 *
 * Conventions as in orbgpu.h and orbgpu_localmap.h.
 */
#ifndef ORBGPU_KFDB_H
#define ORBGPU_KFDB_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"
#include "orbgpu_bow.h"
#include "orbgpu_reloc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ordering pass sorts a query's scored keyframes inside one workgroup's LDS:
 * 8 bytes per keyframe. */
#define ORBGPU_KFDB_MAX_KEYFRAMES 8192
#define ORBGPU_KFDB_MAX_WORDS 4096     /* orbgpu_bow_transform_batch_device's stride limit */
#define ORBGPU_KFDB_COVIS 10           /* GetBestCovisibilityKeyFrames(10)                 */

/* A host struct of device pointers to plain arrays that the caller owns and
 * keeps current; keyframe indices are the map mirror's (orbgpu_localmap.h). */
typedef struct orbgpu_kfdb {
    int n_kf, scoring;          /* DBoW2 ScoringType 0..5                                  */
    int n_bow_total, pad;       /* length of bow_words / bow_values                        */
    const uint8_t* in_db;       /* add()ed and not erase()d                                */
    const int* add_rank;        /* order of the add() calls; NULL = ascending index        */
    const uint8_t* kf_bad;      /* isBad(): read by the minScore pass and by the emit only */
    const int* bow_offset;      /* mBowVec of EVERY keyframe, in the database or not:      */
    const int* n_bow;           /*   words ascending at bow_words[bow_offset[k] ..+n_bow)  */
    const int* bow_words;
    const double* bow_values;
    const int* covis;           /* 10 per keyframe, -1 padded: orbgpu_map_mirror.covis     */
    float* reloc_score;         /* mRelocScore per keyframe: READ AND WRITTEN, see above   */
} orbgpu_kfdb;

enum { ORBGPU_KFDB_RELOC = 0, ORBGPU_KFDB_LOOP = 1 };

typedef struct orbgpu_kfdb_query {
    int kind;
    int n_words;                /* entries of the query BowVector                          */
    int n_connected;            /* LOOP: GetConnectedKeyFrames(), any order (excluded)     */
    int n_covisible;            /* LOOP: GetVectorCovisibleKeyFrames(); -1 = take min_score as given */
    float min_score; int pad;
    const int* words; const double* values;   /* ascending, device                         */
    const int* d_n_words;       /* not NULL: read the count here (bow_transform's d_bow_n + b) instead of n_words */
    const int* connected; const int* covisible;
} orbgpu_kfdb_query;

enum {
    ORBGPU_KFDB_OK = 0,
    ORBGPU_KFDB_CAPACITY = 1,   /* more candidates than cand_stride: n_candidates is the true count,
                                   the first cand_stride are written                                  */
    ORBGPU_KFDB_BAD_JOB = 2     /* an unknown kind; a word count below 0 or above
                                   ORBGPU_KFDB_MAX_WORDS (-1 is a frame bow_transform rejected); an
                                   index in connected, covisible or a read covis row outside [0, n_kf)
                                   (-1 is padding in covis only); bow_offset + n_bow beyond
                                   n_bow_total; a NULL pointer the query needs.  The query ends alone
                                   with only its result written (every count 0)                       */
};

typedef struct orbgpu_kfdb_result {
    int status;                 /* OK, CAPACITY, BAD_JOB                                   */
    int n_sharing;              /* lKFsSharingWords.size()                                 */
    int max_common, min_common;
    int n_filtered;             /* words > min_common                                      */
    int n_scored;               /* lScoreAndMatch.size() (LOOP: also si >= minScore)       */
    int n_candidates;           /* the true count, also under CAPACITY                     */
    float min_score;            /* LOOP: the one used; RELOC: 0                            */
    float best_acc_score; int pad;
} orbgpu_kfdb_result;

/* Bytes of the opaque device block for n queries against n_kf keyframes; the
 * caller need not zero it. */
size_t orbgpu_kfdb_detect_workspace_bytes(int n, int n_kf);

/* d_candidates: int[n][cand_stride], each query's candidates in the reference's
 * order; entries past the count are not written.  d_words / d_scores (each
 * [n][n_kf] or NULL): d_words[q][k] is the common-word count of a listed
 * keyframe and 0 otherwise, d_scores[q][k] is si where the query scored k and 0
 * otherwise; the rows of a BAD_JOB query are not written.  `db` is a host
 * struct.  ORBGPU_ERR_ARG comes before the device is looked at: negative sizes,
 * cand_stride < 1, n_kf above ORBGPU_KFDB_MAX_KEYFRAMES, a scoring outside 0..5,
 * NULL db, d_results, d_candidates, d_queries or d_workspace.  n == 0 needs no
 * device and no table (a db that is given is still checked).  Asynchronous on `stream`: five
 * launches, no host synchronisation, none between workgroups inside a launch. */
int orbgpu_kfdb_detect_batch_device(int n, const orbgpu_kfdb_query* d_queries, const orbgpu_kfdb* db,
                                    int cand_stride, void* d_workspace, orbgpu_kfdb_result* d_results,
                                    int* d_candidates, int* d_words, float* d_scores, void* stream);

/* The relocalisation candidates as the tables of orbgpu_search_by_bow_batch_device,
 * orbgpu_reloc_setup_batch_device and orbgpu_relocalize_batch_device.  Query q
 * (lost frame d_frame_of_query[q]) owns entries [q * cand_stride, (q + 1) *
 * cand_stride) of d_cands, d_a and d_b; d_queries[q] gets first_cand and n_cand,
 * its rng is left as it is.  A used entry gets {frame, kf}, A = d_kf_bow[kf] and
 * B = d_frame_bow[frame].  An unused entry ({frame, 0}), and a candidate whose
 * keyframe is bad (d_kf_bad, Tracking.cpp:1781; NULL = none is), gets an all-zero
 * A: SearchByBoW then returns 0 matches without touching a pointer, and the
 * PnPsolver set-up gives n_corr = -1 before it reads the candidate.  A query
 * under CAPACITY or BAD_JOB gets n_cand = 0.  cand_stride is the detection's,
 * 1 .. ORBGPU_LOOP_MAX_CANDIDATES; n * cand_stride must fit an int. */
int orbgpu_kfdb_emit_reloc_batch_device(int n, const int* d_frame_of_query, const orbgpu_kfdb_result* d_results,
                                        const int* d_candidates, int cand_stride, const uint8_t* d_kf_bad,
                                        const orbgpu_bow_frame* d_kf_bow, const orbgpu_bow_frame* d_frame_bow,
                                        orbgpu_reloc_candidate* d_cands, orbgpu_reloc_query* d_queries,
                                        orbgpu_bow_frame* d_a, orbgpu_bow_frame* d_b, void* stream);

#ifdef __cplusplus
}
#endif
#endif
