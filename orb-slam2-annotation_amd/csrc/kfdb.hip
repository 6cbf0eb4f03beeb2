// kfdb.hip -- the keyframe database on the device (include/orbgpu_kfdb.h):
// KeyFrameDatabase::DetectRelocalizationCandidates / DetectLoopCandidates (src/KeyFrameDatabase.cpp:96-361)
// with DetectLoop's minScore (src/LoopClosing.cpp:136-151), batched over queries, and the glue from the
// relocalisation candidates to the tables of SearchByBoW and the PnPsolver set-up (src/Tracking.cpp:1756-1799).
//
//  orbgpu_kfdb_detect_batch_device, five launches:
//    1 kfdb_prepare_kernel   (query)        the query's checks; LOOP: the connected keyframes marked, and
//                                           minScore over the covisibles, one wave per covisible
//    2 kfdb_intersect_kernel (query, tile)  the query's words staged in LDS once per workgroup, with a hash
//                                           table over them; one wave per (query, keyframe) pair: each lane
//                                           looks one keyframe word up in the query (KL: binary-searches one
//                                           query word in the keyframe), the hits are taken in ballot
//                                           (= word) order and their terms added in that order; per pair
//                                           the common words, the first shared query word and si; per
//                                           query the list's size and maxCommonWords (integer atomics)
//    3 kfdb_order_kernel     (query)        minCommonWords; the scored keyframes' keys (first shared word,
//                                           add_rank, index) sorted in LDS: lScoreAndMatch in list order;
//                                           their covis rows checked
//    4 kfdb_select_kernel    (query)        accScore / pBestKF per entry, bestAccScore, the retain with the
//                                           first occurrence of each pBestKF (atomic min of positions), the
//                                           candidates compacted in order, the result, d_words / d_scores
//    5 kfdb_state_kernel     (keyframe)     reloc_score after the batch: the last query that scored it
//
// A stale mRelocScore read (launch 4) walks the earlier queries of the batch through the per-(query,
// keyframe) tables of launch 2, so the queries stay parallel and a query's result is the reference's
// called once per query in batch order.  Everything but the score is integers and float comparisons;
// there is no float atomic, and every index read from a query or the database is range-checked before
// it is used.  A BAD_JOB query writes nothing but its result: all output comes from launches 4 and 5,
// after the last check.
#include "../../include/orbgpu_kfdb.h"
#include "bow_score.h"
#include "device_state.h"
#include "host_common.h"
#include "ransac_device.h"

namespace orbgpu {

namespace {

using namespace ransacdev;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWords = ORBGPU_KFDB_MAX_WORDS;
constexpr int kMaxKf = ORBGPU_KFDB_MAX_KEYFRAMES;
constexpr int kCovis = ORBGPU_KFDB_COVIS;
constexpr int kPairThreads = 512;  // kfdb_intersect_kernel: eight waves share one staged query
constexpr int kTileKf = 64;  // keyframes per workgroup of the intersection: the query is staged once for them
constexpr int kUnroll = 8;   // stripes of 64 keyframe words a wave has in flight
constexpr int kPending = -1;
constexpr int kKfBits = 20;  // of a sort key; kMaxKf fits

static_assert(kMaxKf <= (1 << kKfBits) && kMaxWords <= (1 << 12), "the sort key's fields");

struct QState {  // a query between the launches
    int status;  // kPending or ORBGPU_KFDB_BAD_JOB
    int kind;
    int nq;          // the query's word count
    int max_common;  // launch 2, atomic max
    int n_sharing;   // launch 2, atomic add
    int bad;         // launch 2: a BowVector outside bow_words
    int min_common;
    int n_filtered;
    int m;  // lScoreAndMatch.size()
    float min_score;
};

struct KWork {  // the opaque block, carved
    QState* st;
    uint8_t* excl;  // per query and keyframe: in `connected` (LOOP)
    int* common;    // per query and keyframe: common words of a listed keyframe, else 0
    int* firstw;    // the query index of the first shared word
    float* si;      // (float)score
    int* list;      // per query: the scored keyframes in list order
    float* acc;     // per query and list position: accScore
    int* best;      // and pBestKF
};

inline KWork carve(void* base, int n, int n_kf, size_t* bytes) {
    const size_t N = (size_t)(n > 0 ? n : 1), NK = (size_t)(n_kf > 0 ? n_kf : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    KWork v;
    v.st = take<QState>(p, N);
    v.excl = take<uint8_t>(p, N * NK);
    v.common = take<int>(p, N * NK);
    v.firstw = take<int>(p, N * NK);
    v.si = take<float>(p, N * NK);
    v.list = take<int>(p, N * NK);
    v.acc = take<float>(p, N * NK);
    v.best = take<int>(p, N * NK);
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return v;
}

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

__device__ __forceinline__ bool span_ok(int off, int cnt, int total) {
    return off >= 0 && cnt >= 0 && (long long)off + cnt <= (long long)total;
}

// lane l's double, l the same in every lane
__device__ __forceinline__ double read_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// the first index of a[0, n) that is not below w
template <class P>
__device__ __forceinline__ int lower_bound(P a, int n, int w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct Pair {
    int common;    // words both hold
    int first;     // the query index of the first of them, -1 for none
    double score;  // TemplatedVocabulary::score
};

// The query in LDS: its words, and a hash table from a word to its index + 1 (0 = empty; open
// addressing, at most half full).  A keyframe word that the query lacks -- most of them -- costs one or
// two LDS reads instead of a binary search's twelve.  The query's words are distinct, so what a lookup
// returns does not depend on the order the workgroup inserted them in.
constexpr int kTabBits = 13;
constexpr int kTabSize = 1 << kTabBits;
static_assert(kTabSize >= 2 * kMaxWords, "the table stays at most half full");

struct QueryLds {
    int words[kMaxWords];
    int tab[kTabSize];
};

__device__ __forceinline__ unsigned tab_slot(int w) { return ((unsigned)w * 2654435761u) >> (32 - kTabBits); }

// every thread of the workgroup calls it; ends with a barrier
__device__ __forceinline__ void stage_query(const orbgpu_kfdb_query& Q, int nq, QueryLds& L) {
    for (int i = threadIdx.x; i < kTabSize; i += blockDim.x) L.tab[i] = 0;
    for (int i = threadIdx.x; i < nq; i += blockDim.x) L.words[i] = Q.words[i];
    __syncthreads();
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        unsigned h = tab_slot(L.words[i]);
        while (atomicCAS(&L.tab[h], 0, i + 1) != 0) h = (h + 1) & (kTabSize - 1);
    }
    __syncthreads();
}

// the index of w in the query, -1 for none
__device__ __forceinline__ int find_word(const QueryLds& L, int w) {
    unsigned h = tab_slot(w);
    for (;;) {
        const int t = L.tab[h];
        if (t == 0) return -1;
        if (L.words[t - 1] == w) return t - 1;
        h = (h + 1) & (kTabSize - 1);
    }
}

// One wave, one (query, keyframe) pair; the query's words are in LDS, its values (qv) and the
// keyframe's words and values (kw, kv, nk of them) in memory.  The terms are added in ascending word
// order by every lane alike.
__device__ Pair wave_pair(int scoring, const QueryLds& L, const double* __restrict__ qv, int nq,
                          const int* __restrict__ kw, const double* __restrict__ kv, int nk, int lane) {
    Pair r{0, -1, 0.0};
    double s = 0.0;
    const int* s_qw = L.words;
    if (scoring != 3) {  // only the common words count: a lane per keyframe word, looked up in the query
        // kUnroll stripes of 64 words at a time: their loads, then their look-ups, then the values of the
        // hits are each issued together, so a pair waits for memory twice per kUnroll * 64 words and not
        // twice per 64
        for (int b = 0; b < nk; b += 64 * kUnroll) {
            int w[kUnroll], idx[kUnroll];
            double t[kUnroll];
            bool add[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int j = b + 64 * u + lane;
                w[u] = j < nk ? kw[j] : -1;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) idx[u] = b + 64 * u + lane < nk ? find_word(L, w[u]) : -1;
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                add[u] = false;
                t[u] = 0.0;
                if (idx[u] >= 0) t[u] = bowscore::common_term(scoring, qv[idx[u]], kv[b + 64 * u + lane], &add[u]);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {  // stripe after stripe, lane after lane: ascending words
                const unsigned long long hits = __ballot(idx[u] >= 0);
                if (!hits) continue;
                if (r.first < 0) r.first = __shfl(idx[u], __ffsll((long long)hits) - 1);
                r.common += (int)__popcll(hits);
                unsigned long long m = __ballot(add[u]);
                while (m) {
                    s += read_lane(t[u], __ffsll((long long)m) - 1);
                    m &= m - 1;
                }
            }
        }
    } else {  // KL walks every query word: a lane per query word, found in the keyframe
        const double log_eps = bowscore::kl_log_eps();
        for (int b = 0; b < nq; b += 64) {
            const int i = b + lane;
            bool hit = false, add = false;
            double t = 0.0;
            if (i < nq) {
                const int a = s_qw[i];
                const double vi = qv[i];
                const int p = lower_bound(kw, nk, a);
                hit = p < nk && kw[p] == a;
                if (hit) {
                    t = bowscore::common_term(3, vi, kv[p], &add);
                } else if (p < nk || vi != 0) {  // past the keyframe's last word the reference skips a zero
                    t = bowscore::kl_query_only_term(vi, log_eps);
                    add = true;
                }
            }
            const unsigned long long hits = __ballot(hit);
            if (hits) {
                if (r.first < 0) r.first = b + __ffsll((long long)hits) - 1;
                r.common += (int)__popcll(hits);
            }
            unsigned long long m = __ballot(add);
            while (m) {
                s += read_lane(t, __ffsll((long long)m) - 1);
                m &= m - 1;
            }
        }
    }
    r.score = bowscore::finish(scoring, s);
    return r;
}

// ------------------------------------------------------------------ 1. the query

__global__ __launch_bounds__(kThreads) void kfdb_prepare_kernel(const orbgpu_kfdb_query* __restrict__ queries,
                                                                orbgpu_kfdb D, KWork V) {
    __shared__ QueryLds s_query;
    __shared__ float s_min[kWaves];
    __shared__ int s_status, s_nq, s_bad;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const orbgpu_kfdb_query& Q = queries[q];
    if (tid == 0) {
        const int nq = Q.d_n_words ? *Q.d_n_words : Q.n_words;
        bool bad = (Q.kind != ORBGPU_KFDB_RELOC && Q.kind != ORBGPU_KFDB_LOOP) || nq < 0 || nq > kMaxWords ||
                   (nq > 0 && (!Q.words || !Q.values));
        if (D.n_kf > 0)
            bad |= !D.in_db || !D.bow_offset || !D.n_bow || !D.covis || (D.n_bow_total > 0 && (!D.bow_words || !D.bow_values)) ||
                   (Q.kind == ORBGPU_KFDB_RELOC && !D.reloc_score);
        if (Q.kind == ORBGPU_KFDB_LOOP)
            bad |= Q.n_connected < 0 || (Q.n_connected > 0 && !Q.connected) || Q.n_covisible < -1 ||
                   (Q.n_covisible > 0 && (!Q.covisible || !D.kf_bad));
        s_status = bad ? ORBGPU_KFDB_BAD_JOB : kPending;
        s_nq = bad ? 0 : nq;
        s_bad = 0;
    }
    __syncthreads();
    int status = s_status;
    const int nq = s_nq;
    float min_score = 0.f;
    if (status == kPending && Q.kind == ORBGPU_KFDB_LOOP) {
        const size_t okf = (size_t)q * (D.n_kf > 0 ? D.n_kf : 1);
        for (int k = tid; k < D.n_kf; k += kThreads) V.excl[okf + k] = 0;
        __syncthreads();
        bool bad = false;
        for (int i = tid; i < Q.n_connected; i += kThreads) {
            const int k = Q.connected[i];
            if (!in_range(k, D.n_kf)) bad = true;
            else V.excl[okf + k] = 1;
        }
        min_score = Q.min_score;
        if (Q.n_covisible >= 0) {  // LoopClosing.cpp:136-151, a wave per covisible keyframe
            stage_query(Q, nq, s_query);
            float m = 1.f;
            for (int c = wave; c < Q.n_covisible; c += kWaves) {
                const int k = Q.covisible[c];
                if (!in_range(k, D.n_kf)) {
                    bad = true;
                    continue;
                }
                if (D.kf_bad[k]) continue;
                const int off = D.bow_offset[k], nk = D.n_bow[k];
                if (!span_ok(off, nk, D.n_bow_total)) {
                    bad = true;
                    continue;
                }
                const Pair p = wave_pair(D.scoring, s_query, Q.values, nq, D.bow_words + off, D.bow_values + off, nk, lane);
                const float score = (float)p.score;
                if (score < m) m = score;
            }
            if (lane == 0) s_min[wave] = m;
            __syncthreads();
            min_score = 1.f;
            for (int w = 0; w < kWaves; ++w)
                if (s_min[w] < min_score) min_score = s_min[w];
        }
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
        if (s_bad) status = ORBGPU_KFDB_BAD_JOB;
    }
    if (tid == 0) {
        QState& S = V.st[q];
        S.status = status;
        S.kind = Q.kind;
        S.nq = nq;
        S.max_common = S.n_sharing = S.bad = 0;
        S.min_common = S.n_filtered = S.m = 0;
        S.min_score = min_score;
    }
}

// ------------------------------------------------------------------ 2. the pairs

__global__ __launch_bounds__(kPairThreads) void kfdb_intersect_kernel(const orbgpu_kfdb_query* __restrict__ queries,
                                                                  orbgpu_kfdb D, KWork V) {
    __shared__ QueryLds s_query;
    const int q = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    QState& S = V.st[q];
    if (S.status != kPending) return;
    const orbgpu_kfdb_query& Q = queries[q];
    const int nq = S.nq;
    const bool loop = S.kind == ORBGPU_KFDB_LOOP;
    stage_query(Q, nq, s_query);
    const size_t okf = (size_t)q * D.n_kf;
    int n_sharing = 0, max_common = 0;
    bool bad = false;
    // the tile's keyframes lie a grid apart: neighbours on a path share their words with the same queries,
    // and the pairs with many hits should not all fall to one workgroup
    for (int i = wave; i < kTileKf; i += kPairThreads / 64) {
        const int k = i * (int)gridDim.y + tile;
        if (k >= D.n_kf) break;
        Pair p{0, -1, 0.0};
        if (nq > 0 && D.in_db[k] && !(loop && V.excl[okf + k])) {
            const int off = D.bow_offset[k], nk = D.n_bow[k];
            if (!span_ok(off, nk, D.n_bow_total)) bad = true;
            else p = wave_pair(D.scoring, s_query, Q.values, nq, D.bow_words + off, D.bow_values + off, nk, lane);
        }
        if (lane == 0) {
            V.common[okf + k] = p.common;
            V.firstw[okf + k] = p.first;
            V.si[okf + k] = p.common > 0 ? (float)p.score : 0.f;
        }
        if (p.common > 0) {
            ++n_sharing;
            max_common = max(max_common, p.common);
        }
    }
    if (lane == 0) {
        if (n_sharing) {
            atomicAdd(&S.n_sharing, n_sharing);
            atomicMax(&S.max_common, max_common);
        }
        if (bad) atomicOr(&S.bad, 1);
    }
}

// ------------------------------------------------------------------ 3. the list's order

__global__ __launch_bounds__(kThreads) void kfdb_order_kernel(orbgpu_kfdb D, KWork V, int n_sort) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_dyn);  // n_sort of them
    __shared__ int s_m, s_filtered, s_bad;
    const int q = blockIdx.x, tid = threadIdx.x;
    QState& S = V.st[q];
    if (S.status != kPending) return;
    if (S.bad) {  // uniform: written by launch 2
        if (tid == 0) S.status = ORBGPU_KFDB_BAD_JOB;
        return;
    }
    if (tid == 0) s_m = s_filtered = s_bad = 0;
    __syncthreads();
    const size_t okf = (size_t)q * (D.n_kf > 0 ? D.n_kf : 1);
    const bool loop = S.kind == ORBGPU_KFDB_LOOP;
    const int min_common = (int)((float)S.max_common * 0.8f);
    const float min_score = S.min_score;
    bool bad = false;
    for (int k = tid; k < D.n_kf; k += kThreads) {
        if (V.common[okf + k] <= min_common) continue;  // a listed keyframe has at least one
        atomicAdd(&s_filtered, 1);
        if (loop && !(V.si[okf + k] >= min_score)) continue;
        for (int j = 0; j < kCovis; ++j) {  // the row the accumulation reads
            const int c = D.covis[(size_t)k * kCovis + j];
            if (c != -1 && !in_range(c, D.n_kf)) bad = true;
        }
        const unsigned rank = (unsigned)(D.add_rank ? D.add_rank[k] : k) ^ 0x80000000u;
        s_key[atomicAdd(&s_m, 1)] = ((unsigned long long)(unsigned)V.firstw[okf + k] << (32 + kKfBits)) |
                                    ((unsigned long long)rank << kKfBits) | (unsigned)k;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    const int m = s_m;
    int P = 1;
    while (P < m) P <<= 1;  // <= n_sort
    for (int i = m + tid; i < P; i += kThreads) s_key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)  // the keys are distinct, so the sorted order is a function of the set
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = s_key[i], b = s_key[l];
                    if ((a > b) == ((i & k) == 0)) {
                        s_key[i] = b;
                        s_key[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < m; i += kThreads) V.list[okf + i] = (int)(s_key[i] & ((1u << kKfBits) - 1));
    if (tid == 0) {
        S.min_common = min_common;
        S.n_filtered = s_filtered;
        S.m = m;
        if (s_bad) S.status = ORBGPU_KFDB_BAD_JOB;
    }
    (void)n_sort;
}

// ------------------------------------------------------------------ 4. the candidates

// mRelocScore of keyframe k as query q finds it: written by the latest earlier relocalisation query
// of the batch that scored k, else what the array held at the call
__device__ __forceinline__ float stale_reloc_score(const orbgpu_kfdb& D, const KWork& V, int q, int k) {
    for (int e = q - 1; e >= 0; --e) {
        const QState& E = V.st[e];
        if (E.status == kPending && E.kind == ORBGPU_KFDB_RELOC && V.common[(size_t)e * D.n_kf + k] > E.min_common)
            return V.si[(size_t)e * D.n_kf + k];
    }
    return D.reloc_score[k];
}

__global__ __launch_bounds__(kThreads) void kfdb_select_kernel(orbgpu_kfdb D, KWork V, int cand_stride,
                                                               orbgpu_kfdb_result* __restrict__ results,
                                                               int* __restrict__ candidates, int* __restrict__ words,
                                                               float* __restrict__ scores) {
    __shared__ int s_first[kMaxKf];  // per keyframe: the first retained entry that names it as pBestKF
    __shared__ int s_wave[kWaves];
    __shared__ float s_best[kWaves];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const QState& S = V.st[q];
    orbgpu_kfdb_result& R = results[q];
    if (S.status != kPending) {
        if (tid == 0) {
            R.status = ORBGPU_KFDB_BAD_JOB;
            R.n_sharing = R.max_common = R.min_common = R.n_filtered = R.n_scored = R.n_candidates = R.pad = 0;
            R.min_score = R.best_acc_score = 0.f;
        }
        return;
    }
    const size_t okf = (size_t)q * (D.n_kf > 0 ? D.n_kf : 1);
    const bool loop = S.kind == ORBGPU_KFDB_LOOP;
    const int min_common = S.min_common, m = S.m;
    const int* common = V.common + okf;
    const float* si = V.si + okf;
    for (int k = tid; k < D.n_kf; k += kThreads) {
        const int c = common[k];
        if (words) words[okf + k] = c;
        if (scores) scores[okf + k] = c > min_common ? si[k] : 0.f;
        s_first[k] = 0x7fffffff;
    }
    // accScore and pBestKF of every entry (KeyFrameDatabase.cpp:170-196, :309-336)
    float best_acc = loop ? S.min_score : 0.f;
    for (int i = tid; i < m; i += kThreads) {
        const int kf = V.list[okf + i];
        float best = si[kf], acc = best;
        int best_kf = kf;
        for (int j = 0; j < kCovis; ++j) {
            const int nb = D.covis[(size_t)kf * kCovis + j];
            if (nb < 0) continue;  // padding; the range was checked by launch 3
            const int c = common[nb];
            float s2;
            if (loop) {
                if (c <= min_common) continue;
                s2 = si[nb];
            } else {
                if (c <= 0) continue;
                s2 = c > min_common ? si[nb] : stale_reloc_score(D, V, q, nb);
            }
            acc = acc + s2;
            if (s2 > best) {
                best_kf = nb;
                best = s2;
            }
        }
        V.acc[okf + i] = acc;
        V.best[okf + i] = best_kf;
        if (acc > best_acc) best_acc = acc;
    }
    for (int d = 32; d > 0; d >>= 1) {  // a maximum: the same in any order
        const float o = __shfl_xor(best_acc, d);
        if (o > best_acc) best_acc = o;
    }
    if (lane == 0) s_best[wave] = best_acc;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w)
        if (s_best[w] > best_acc) best_acc = s_best[w];
    const float keep = 0.75f * best_acc;
    for (int i = tid; i < m; i += kThreads)
        if (V.acc[okf + i] > keep) atomicMin(&s_first[V.best[okf + i]], i);
    __syncthreads();
    int n_cand = 0;
    for (int s = 0; s < m; s += kThreads) {  // the retain, in list order
        const int i = s + tid;
        int kf = -1;
        bool ok = false;
        if (i < m) {
            kf = V.best[okf + i];
            ok = V.acc[okf + i] > keep && s_first[kf] == i;
        }
        const int pos = compact_slot(ok, lane, wave, s_wave, n_cand);
        if (ok && pos < cand_stride) candidates[(size_t)q * cand_stride + pos] = kf;
        compact_advance<kThreads>(s_wave, n_cand);
        __syncthreads();
    }
    if (tid == 0) {
        const bool listed = S.n_sharing > 0;
        R.status = n_cand > cand_stride ? ORBGPU_KFDB_CAPACITY : ORBGPU_KFDB_OK;
        R.n_sharing = S.n_sharing;
        R.max_common = S.max_common;
        R.min_common = listed ? min_common : 0;
        R.n_filtered = S.n_filtered;
        R.n_scored = m;
        R.n_candidates = n_cand;
        R.min_score = loop ? S.min_score : 0.f;
        R.best_acc_score = best_acc;
        R.pad = 0;
    }
}

// ------------------------------------------------------------------ 5. mRelocScore after the batch

__global__ __launch_bounds__(kThreads) void kfdb_state_kernel(int n, orbgpu_kfdb D, KWork V) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= D.n_kf || !D.reloc_score) return;
    for (int q = n - 1; q >= 0; --q) {
        const QState& S = V.st[q];
        if (S.status == kPending && S.kind == ORBGPU_KFDB_RELOC && V.common[(size_t)q * D.n_kf + k] > S.min_common) {
            D.reloc_score[k] = V.si[(size_t)q * D.n_kf + k];
            return;
        }
    }
}

// ------------------------------------------------------------------ the glue to Relocalization()

__global__ __launch_bounds__(64) void kfdb_emit_reloc_kernel(const int* __restrict__ frame_of_query,
                                                             const orbgpu_kfdb_result* __restrict__ results,
                                                             const int* __restrict__ candidates, int cand_stride,
                                                             const uint8_t* __restrict__ kf_bad,
                                                             const orbgpu_bow_frame* __restrict__ kf_bow,
                                                             const orbgpu_bow_frame* __restrict__ frame_bow,
                                                             orbgpu_reloc_candidate* __restrict__ cands,
                                                             orbgpu_reloc_query* __restrict__ queries,
                                                             orbgpu_bow_frame* __restrict__ fa,
                                                             orbgpu_bow_frame* __restrict__ fb) {
    const int q = blockIdx.x, c = threadIdx.x;
    const orbgpu_kfdb_result& R = results[q];
    const int used = R.status == ORBGPU_KFDB_OK ? min(R.n_candidates, cand_stride) : 0;
    const int frame = frame_of_query[q];
    if (c == 0) {
        queries[q].first_cand = q * cand_stride;
        queries[q].n_cand = used;
    }
    if (c >= cand_stride) return;
    const size_t e = (size_t)q * cand_stride + c;
    const int kf = c < used ? candidates[e] : 0;
    orbgpu_bow_frame a;
    a.n = a.fv_n = 0;
    a.fv_nodes = a.fv_offsets = a.fv_features = nullptr;
    a.desc = a.valid = nullptr;
    a.angle = nullptr;
    if (c < used && !(kf_bad && kf_bad[kf])) a = kf_bow[kf];  // Tracking.cpp:1781: a bad keyframe is discarded
    cands[e].frame = frame;
    cands[e].kf = kf;
    fa[e] = a;
    fb[e] = frame_bow[frame];
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

size_t orbgpu_kfdb_detect_workspace_bytes(int n, int n_kf) {
    size_t bytes = 0;
    carve(nullptr, n, n_kf, &bytes);
    return bytes;
}

int orbgpu_kfdb_detect_batch_device(int n, const orbgpu_kfdb_query* d_queries, const orbgpu_kfdb* db,
                                    int cand_stride, void* d_workspace, orbgpu_kfdb_result* d_results,
                                    int* d_candidates, int* d_words, float* d_scores, void* stream) {
    if (n < 0 || cand_stride < 1) return fail(ORBGPU_ERR_ARG, "negative n or cand_stride below 1");
    if (n > 0 && (!db || !d_results || !d_candidates)) return fail(ORBGPU_ERR_ARG, "db, d_results or d_candidates is NULL");
    if (db) {
        if (db->n_kf < 0 || db->n_bow_total < 0) return fail(ORBGPU_ERR_ARG, "a database count is negative");
        if (db->n_kf > kMaxKf) return fail(ORBGPU_ERR_ARG, "n_kf above ORBGPU_KFDB_MAX_KEYFRAMES");
        if (db->scoring < 0 || db->scoring > 5) return fail(ORBGPU_ERR_ARG, "scoring outside 0..5");
    }
    if (n > 0 && (!d_queries || !d_workspace)) return fail(ORBGPU_ERR_ARG, "d_queries or d_workspace is NULL");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const orbgpu_kfdb D = *db;
    const KWork V = carve(d_workspace, n, D.n_kf, nullptr);
    const dim3 block(kThreads), per_query(n);
    hipLaunchKernelGGL(kfdb_prepare_kernel, per_query, block, 0, s, d_queries, D, V);
    ORB_HIP(hipGetLastError());
    if (D.n_kf > 0) {
        hipLaunchKernelGGL(kfdb_intersect_kernel, dim3(n, (D.n_kf + kTileKf - 1) / kTileKf), dim3(kPairThreads), 0, s, d_queries, D,
                           V);
        ORB_HIP(hipGetLastError());
    }
    const int n_sort = pow2_at_least(D.n_kf > 64 ? D.n_kf : 64);
    const size_t lds = (size_t)n_sort * sizeof(unsigned long long);
    static PerDeviceLdsLimit lds_limit;
    ORB_HIP(lds_limit.ensure(reinterpret_cast<const void*>(&kfdb_order_kernel), lds));
    hipLaunchKernelGGL(kfdb_order_kernel, per_query, block, lds, s, D, V, n_sort);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(kfdb_select_kernel, per_query, block, 0, s, D, V, cand_stride, d_results, d_candidates, d_words,
                       d_scores);
    ORB_HIP(hipGetLastError());
    if (D.n_kf > 0) {
        hipLaunchKernelGGL(kfdb_state_kernel, dim3((D.n_kf + kThreads - 1) / kThreads), block, 0, s, n, D, V);
        ORB_HIP(hipGetLastError());
    }
    return ORBGPU_OK;
}

int orbgpu_kfdb_emit_reloc_batch_device(int n, const int* d_frame_of_query, const orbgpu_kfdb_result* d_results,
                                        const int* d_candidates, int cand_stride, const uint8_t* d_kf_bad,
                                        const orbgpu_bow_frame* d_kf_bow, const orbgpu_bow_frame* d_frame_bow,
                                        orbgpu_reloc_candidate* d_cands, orbgpu_reloc_query* d_queries,
                                        orbgpu_bow_frame* d_a, orbgpu_bow_frame* d_b, void* stream) {
    if (n < 0 || cand_stride < 1 || cand_stride > ORBGPU_LOOP_MAX_CANDIDATES)
        return fail(ORBGPU_ERR_ARG, "negative n or cand_stride outside 1..ORBGPU_LOOP_MAX_CANDIDATES");
    if ((long long)n * cand_stride > 0x7fffffffLL) return fail(ORBGPU_ERR_ARG, "n * cand_stride overflows");
    if (n > 0 && (!d_frame_of_query || !d_results || !d_candidates || !d_kf_bow || !d_frame_bow || !d_cands ||
                  !d_queries || !d_a || !d_b))
        return fail(ORBGPU_ERR_ARG, "a table is NULL");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    static_assert(ORBGPU_LOOP_MAX_CANDIDATES <= 64, "one lane per entry");
    hipLaunchKernelGGL(kfdb_emit_reloc_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, d_frame_of_query, d_results,
                       d_candidates, cand_stride, d_kf_bad, d_kf_bow, d_frame_bow, d_cands, d_queries, d_a, d_b);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

}  // extern "C"
