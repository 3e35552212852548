// orbfe_kfdb.hip — place recognition on gfx950: a resident database of bag-of-words vectors and the
// L1 scoring kernel behind KeyFrameDatabase.detect_loop_candidates / detect_relocalization_candidates
// (KeyFrameDatabase.py:30-159) and TemplatedVocabulary.score (TemplatedVocabulary.py:99-106).
//
// The reference keeps an inverted file (word id -> list of keyframes) and, per query, walks it in Python
// (query word x keyframes holding it) and then calls GeneralScoring.l1_score per surviving keyframe
// (ScoringObject.py:8-28).  Here the vectors themselves stay on the device and every query sweeps all
// of them once: per stored vector the kernel intersects its sorted word ids with the query's and returns
//   common  number of shared words             (what the walk adds to mnLoopWords / mnRelocWords)
//   first   smallest shared word id, -1 if none (the walk's first-appearance order is (first, slot))
//   score   canonical L1 score                  (below)
//
// Canonical L1 score.  The reference sums over a Python set of ints, i.e. in CPython's hash-table order,
// which depends on set sizes and probing.  One admissible order is fixed instead (DBoW2's own): the terms
// (fabs(vi - wi) - fabs(vi)) - fabs(wi), vi the query's weight and wi the stored one, are added in
// ascending word id, sequentially, in IEEE double (no contraction: -ffp-contract=off), and the score is
// -sum / 2.0; no shared word gives -0.0 as in the reference.  Single pairs, many pairs and the database
// all run this one kernel, so they agree bit for bit whatever the database size, insertion order, erased
// neighbours, capacity growth or block count.
//
// Storage.  An append-only CSR arena (int32 word ids and f64 weights in separate arrays) plus a per-slot
// table {offset, length, live}.  The host holds the master copy: create / add / erase / clear / stats make
// no device call and work on a host without a GPU.  A query first copies what the device has not seen yet
// (the arena tail and the changed slot range).  When an array outgrows its capacity the capacity doubles
// and erased vectors are dropped from the arena at that moment (slot numbers never change); the device
// copy is then rebuilt at the next query.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "orbfe_host_util.h"

using namespace orbfe;

namespace orbfe {

struct KfdbSlot {
    int64_t off;   // first arena entry of the vector
    int32_t len;   // its word count (0 once dropped from the arena)
    int32_t live;  // 0 after erase
};
static_assert(sizeof(KfdbSlot) == 16, "slot table entry is 16 bytes");

constexpr int kBowWaves = 4;          // waves per 256-thread block, one stored vector per wave at a time
constexpr int kBowLdsWords = 8192;    // query word ids staged in LDS up to this length (32 KiB of dynamic LDS, so
                                      // five blocks still share a CU); longer queries are searched in global memory
constexpr int kBowMaxBlocks = 2048;   // 8 blocks per CU: a block loops over vectors so the staging is amortised

constexpr int kBowUnroll = 4;         // words per lane and pass: independent searches in flight per lane

// One pass of one stored vector against one query, the routine k_bow_score and k_bow_score_many share (so the
// two agree bit for bit by construction).  w[u] is the stored word at position u * 64 + lane of the pass (-1 past
// the vector's end: ids are non-negative, -1 matches nothing) and wt the pass's first weight.  Each lane
// binary-searches the nq > 0 query ids q (LDS or global) for its kBowUnroll words.  The search is the
// branchless halving form, whose trip count depends on nq alone: every lane runs the same steps, and the
// kBowUnroll searches of a lane are independent, so their reads overlap instead of queueing behind one another
// (the kernel is bound by that chain's latency).  Then, 64 words at a time in ascending
// order: the ballot of the hits gives common and first; only hit lanes fetch the two weights and form their
// term; the terms are added to the wave-uniform running sum in ascending lane order (= ascending word id) by
// walking the ballot's set bits with a lane read, so the sum is the sequential one whatever the chunking.
__device__ __forceinline__ void bow_pass(const int32_t* q, const double* __restrict__ q_weight, int nq,
                                         const int (&w)[kBowUnroll], const double* __restrict__ wt, int lane,
                                         int& common, int& first, double& sum) {
    int base[kBowUnroll];
#pragma unroll
    for (int u = 0; u < kBowUnroll; ++u) base[u] = 0;
    // q[base] ends as the last query id <= w (q[0] when there is none)
    for (int n = nq; n > 1;) {
        const int half = n >> 1;
#pragma unroll
        for (int u = 0; u < kBowUnroll; ++u) base[u] = q[base[u] + half] <= w[u] ? base[u] + half : base[u];
        n -= half;
    }
#pragma unroll
    for (int u = 0; u < kBowUnroll; ++u) {
        const bool hit = q[base[u]] == w[u];
        unsigned long long hits = __ballot(hit);
        if (hits == 0) continue;
        double term = 0.0;
        if (hit) {
            const double vi = q_weight[base[u]];
            const double wi = wt[u * 64 + lane];
            term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
        }
        if (first < 0) first = __shfl(w[u], __ffsll((long long)hits) - 1, 64);
        common += __popcll(hits);
        while (hits) {
            const int b = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            sum += __shfl(term, b, 64);
        }
    }
}

// The stored words of one pass: lane j takes words j, j + 64, ... of the 64 * kBowUnroll words from position c.
__device__ __forceinline__ void bow_load_pass(const int32_t* __restrict__ word, int64_t off, int c, int len, int lane,
                                              int (&w)[kBowUnroll]) {
#pragma unroll
    for (int u = 0; u < kBowUnroll; ++u) {
        const int j = c + u * 64 + lane;
        w[u] = j < len ? word[off + j] : -1;
    }
}

// One query, one stored vector per wave, passes of 64 * kBowUnroll words through bow_pass (query ids in LDS when
// LDS is true, global otherwise).
template <bool LDS>
__global__ __launch_bounds__(64 * kBowWaves) void k_bow_score(const int32_t* __restrict__ q_word,
                                                              const double* __restrict__ q_weight, int nq,
                                                              const KfdbSlot* __restrict__ slot,
                                                              const int32_t* __restrict__ word,
                                                              const double* __restrict__ weight, int64_t n_slots,
                                                              int32_t* __restrict__ out_common,
                                                              int32_t* __restrict__ out_first,
                                                              double* __restrict__ out_score) {
    extern __shared__ int32_t s_q[];  // nq word ids when LDS (sized by the launch: short queries leave the CU's
                                      // LDS to more resident blocks), unused otherwise
    if (LDS) {
        for (int i = threadIdx.x; i < nq; i += blockDim.x) s_q[i] = q_word[i];
        __syncthreads();
    }
    const int32_t* q = LDS ? s_q : q_word;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int64_t s = (int64_t)blockIdx.x * kBowWaves + wave; s < n_slots; s += (int64_t)gridDim.x * kBowWaves) {
        const KfdbSlot sl = slot[s];
        int common = 0, first = -1;
        double sum = 0.0;
        const int len = (sl.live && nq > 0) ? sl.len : 0;
        for (int c = 0; c < len; c += 64 * kBowUnroll) {
            int w[kBowUnroll];
            bow_load_pass(word, sl.off, c, len, lane, w);
            bow_pass(q, q_weight, nq, w, weight + sl.off + c, lane, common, first, sum);
        }
        if (lane == 0) {
            out_common[s] = common;
            out_first[s] = first;
            out_score[s] = -sum / 2.0;
        }
    }
}

// ---- many queries in one launch ---------------------------------------------------------------------------------
#ifdef ORBFE_BOW_TILE  // same-box A/B builds of other tile shapes
constexpr int kBowTile = ORBFE_BOW_TILE;
constexpr int kBowManyWaves = ORBFE_BOW_MANY_WAVES;
#else
constexpr int kBowTile = 4;        // queries whose word ids one block of k_bow_score_many stages in LDS
constexpr int kBowManyWaves = 8;   // waves of that block: they share the staged tile, one stored vector per wave
#endif                             // (4 x 8 by measurement)
constexpr int kBowTileLdsWords = 16000;  // LDS budget of a tile: 62.5 KiB of dynamic LDS at the most, within the
                                         // 64 KiB a launch gets without opting in, so two blocks still share a CU;
                                         // a tile of four 1 500-word queries takes 23.4 KiB: six blocks fit and
                                         // four of them fill the CU's 32 waves
constexpr int kGateThreads = 1024;  // k_bow_gate: one block per query,
constexpr int kGateItems = 4;       // consecutive slots per thread and step: 4 096 slots per compaction step
static_assert(kBowTile >= 1 && kBowTile <= 64, "lane t of a wave keeps the running results of the tile's query t");
static_assert(kBowManyWaves >= 1 && kBowManyWaves <= 16, "at most 1 024 threads per block");

// Where the queries of a many-query call are.  Host entry: query g is entries [off[g], off[g + 1]) of word /
// weight.  Device entry (off == nullptr): the count[g] entries from g * stride, what orbfe_vocab_bow_device
// wrote; the count is clamped to [0, stride] here, on the device.
struct BowQueries {
    const int32_t* word;
    const double* weight;
    const int64_t* off;
    const int32_t* count;
    int64_t stride;
};

__device__ __forceinline__ void query_span(const BowQueries& qs, int g, int64_t& start, int& len) {
    if (qs.off) {
        start = qs.off[g];
        len = (int)(qs.off[g + 1] - start);
    } else {
        start = (int64_t)g * qs.stride;
        const int64_t n = qs.count[g];
        len = (int)(n < 0 ? 0 : (n > qs.stride ? qs.stride : n));
    }
}

// Queries [q0, q0 + n_query) against every stored vector: block (x, y) takes the tile of kBowTile queries from
// q0 + y * kBowTile and the slots x * kBowManyWaves + wave, + gridDim.x * kBowManyWaves, ...  The tile's word ids
// are staged in LDS once per block, packed one after the other: a query longer than kBowLdsWords, or one that
// no longer fits in the launch's lds_words, is searched in global memory instead.  Per stored vector a wave loads
// each pass of 64 * kBowUnroll words once and runs bow_pass on it for every query of the tile, so the arena is
// streamed once per tile, not once per query.  The running common / first / sum of query t live in lane t
// between passes (they are wave-uniform inside bow_pass).  Results go to out_*[(y * kBowTile + t) * n_slots + s].
__global__ __launch_bounds__(64 * kBowManyWaves) void k_bow_score_many(
    BowQueries qs, int q0, int n_query, int lds_words, const KfdbSlot* __restrict__ slot,
    const int32_t* __restrict__ word, const double* __restrict__ weight, int64_t n_slots,
    int32_t* __restrict__ out_common, int32_t* __restrict__ out_first, double* __restrict__ out_score) {
    extern __shared__ int32_t s_q[];
    __shared__ int64_t s_start[kBowTile];
    __shared__ int s_len[kBowTile], s_at[kBowTile];  // s_at: where the query starts in s_q, -1 = not staged
    const int t0 = blockIdx.y * kBowTile;
    const int nt = min(kBowTile, n_query - t0);
    if (threadIdx.x == 0) {
        int used = 0;
        for (int t = 0; t < nt; ++t) {
            int64_t start;
            int len;
            query_span(qs, q0 + t0 + t, start, len);
            s_start[t] = start;
            s_len[t] = len;
            const bool fits = len <= kBowLdsWords && used + len <= lds_words;
            s_at[t] = fits ? used : -1;
            if (fits) used += len;
        }
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t)
        if (s_at[t] >= 0)
            for (int i = threadIdx.x; i < s_len[t]; i += blockDim.x) s_q[s_at[t] + i] = qs.word[s_start[t] + i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int64_t s = (int64_t)blockIdx.x * kBowManyWaves + wave; s < n_slots;
         s += (int64_t)gridDim.x * kBowManyWaves) {
        const KfdbSlot sl = slot[s];
        int my_common = 0, my_first = -1;  // lane t: query t of the tile
        double my_sum = 0.0;
        const int len = sl.live ? sl.len : 0;
        for (int c = 0; c < len; c += 64 * kBowUnroll) {
            int w[kBowUnroll];
            bow_load_pass(word, sl.off, c, len, lane, w);
            for (int t = 0; t < nt; ++t) {
                const int nq = s_len[t];
                if (nq == 0) continue;
                int common = __shfl(my_common, t, 64), first = __shfl(my_first, t, 64);
                double sum = __shfl(my_sum, t, 64);
                const double* qv = qs.weight + s_start[t];
                if (s_at[t] >= 0)
                    bow_pass(s_q + s_at[t], qv, nq, w, weight + sl.off + c, lane, common, first, sum);
                else
                    bow_pass(qs.word + s_start[t], qv, nq, w, weight + sl.off + c, lane, common, first, sum);
                if (lane == t) {
                    my_common = common;
                    my_first = first;
                    my_sum = sum;
                }
            }
        }
        if (lane < nt) {
            const int64_t o = (int64_t)(t0 + lane) * n_slots + s;
            out_common[o] = my_common;
            out_first[o] = my_first;
            out_score[o] = -my_sum / 2.0;
        }
    }
}

// whether slot s is in the ascending list e[0 .. n)
__device__ __forceinline__ bool excluded(const int32_t* __restrict__ e, int n, int s) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && e[lo] == s;
}

// The word gate of KeyFrameDatabase.detect_*_candidates (KeyFrameDatabase.py:60-66, 126-131) and the compaction
// of the survivors, one block per query of the chunk (row blockIdx.x of the dense arrays, query q0 + blockIdx.x
// of the call).  Step 1 reduces max_common (live slots that are not excluded) and n_sharing (live slots with
// common > 0) over the block.  Step 2 walks the slots in ascending order, kGateThreads * kGateItems at a time,
// each thread kGateItems consecutive ones: a hit is a live, not excluded slot with common > 0 and
// common > (int32_t)((double)max_common * gate_ratio); its place in the output is the count of hits before it,
// from a scan over the block (shuffles inside a wave, the wave totals through LDS), so the order is ascending
// slot whatever the scheduling.  Hits past hit_cap are counted, not written.
__global__ __launch_bounds__(kGateThreads) void k_bow_gate(
    const int32_t* __restrict__ common, const int32_t* __restrict__ first, const double* __restrict__ score,
    const KfdbSlot* __restrict__ slot, int64_t n_slots, int q0, const int64_t* __restrict__ excl_off,
    const int32_t* __restrict__ excl_slot, double gate_ratio, int hit_cap, int32_t* __restrict__ n_sharing,
    int32_t* __restrict__ max_common, int32_t* __restrict__ n_hits, int32_t* __restrict__ hit_slot,
    int32_t* __restrict__ hit_common, int32_t* __restrict__ hit_first, double* __restrict__ hit_score) {
    constexpr int kWaves = kGateThreads / 64;
    __shared__ int s_a[kWaves], s_b[kWaves];
    const int q = q0 + blockIdx.x;
    common += (int64_t)blockIdx.x * n_slots;
    first += (int64_t)blockIdx.x * n_slots;
    score += (int64_t)blockIdx.x * n_slots;
    const int32_t* ex = nullptr;
    int n_ex = 0;
    if (excl_off) {
        ex = excl_slot + excl_off[q];
        n_ex = (int)(excl_off[q + 1] - excl_off[q]);
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    int sharing = 0, mx = 0;
    for (int64_t s = threadIdx.x; s < n_slots; s += kGateThreads) {
        const int c = common[s];
        if (c > 0 && slot[s].live) {
            ++sharing;
            if (!excluded(ex, n_ex, (int)s)) mx = max(mx, c);
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        sharing += __shfl_xor(sharing, d, 64);
        mx = max(mx, __shfl_xor(mx, d, 64));
    }
    if (lane == 0) {
        s_a[wave] = sharing;
        s_b[wave] = mx;
    }
    __syncthreads();
    sharing = 0;
    mx = 0;
    for (int i = 0; i < kWaves; ++i) {
        sharing += s_a[i];
        mx = max(mx, s_b[i]);
    }
    __syncthreads();  // s_a is reused below
    const int gate = (int32_t)((double)mx * gate_ratio);

    int64_t total = 0;  // hits before the current step
    for (int64_t s0 = 0; s0 < n_slots; s0 += (int64_t)kGateThreads * kGateItems) {
        const int64_t mine = s0 + (int64_t)threadIdx.x * kGateItems;
        int c[kGateItems];
        bool hit[kGateItems];
        int n = 0;
#pragma unroll
        for (int k = 0; k < kGateItems; ++k) {
            const int64_t s = mine + k;
            c[k] = s < n_slots ? common[s] : 0;
            hit[k] = c[k] > 0 && c[k] > gate && slot[s].live && !excluded(ex, n_ex, (int)s);
            n += hit[k];
        }
        int incl = n;  // inclusive scan of n over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_a[wave] = incl;
        __syncthreads();
        int before = 0, step = 0;
        for (int i = 0; i < kWaves; ++i) {
            const int v = s_a[i];
            if (i < wave) before += v;
            step += v;
        }
        __syncthreads();
        int64_t at = total + before + incl - n;
#pragma unroll
        for (int k = 0; k < kGateItems; ++k) {
            if (!hit[k]) continue;
            if (at < hit_cap) {
                const int64_t o = (int64_t)q * hit_cap + at;
                hit_slot[o] = (int32_t)(mine + k);
                hit_common[o] = c[k];
                hit_first[o] = first[mine + k];
                hit_score[o] = score[mine + k];
            }
            ++at;
        }
        total += step;
    }
    if (threadIdx.x == 0) {
        n_sharing[q] = sharing;
        max_common[q] = mx;
        n_hits[q] = (int32_t)total;
    }
}

// Device scratch of one scorer: the query, the three result arrays, a stream and two events.
struct BowScratch {
    DevBuf<int32_t> d_qw, d_common, d_first;
    DevBuf<double> d_qv, d_score;
    TimedStream t;
    ~BowScratch() { t.destroy(); }
    // query upload, one launch over n_slots device-resident vectors, results to host buffers; synchronous
    void run(const int32_t* q_word, const double* q_weight, int32_t nq, const KfdbSlot* d_slot, const int32_t* d_word,
             const double* d_weight, int64_t n_slots, int32_t* common, int32_t* first, double* score) {
        hipStream_t stream = t.get();
        d_qw.ensure(nq);
        d_qv.ensure(nq);
        d_common.ensure(n_slots);
        d_first.ensure(n_slots);
        d_score.ensure(n_slots);
        if (nq) {
            HIPCK(hipMemcpyAsync(d_qw.p, q_word, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            HIPCK(hipMemcpyAsync(d_qv.p, q_weight, (size_t)nq * sizeof(double), hipMemcpyHostToDevice, stream));
        }
        const int64_t want = (n_slots + kBowWaves - 1) / kBowWaves;
        const unsigned blocks = (unsigned)std::min<int64_t>(want, kBowMaxBlocks);
        t.begin(stream);
        if (nq <= kBowLdsWords)
            hipLaunchKernelGGL(k_bow_score<true>, dim3(blocks), dim3(64 * kBowWaves), (size_t)nq * sizeof(int32_t),
                               stream, d_qw.p, d_qv.p, nq, d_slot, d_word, d_weight, n_slots, d_common.p, d_first.p,
                               d_score.p);
        else
            hipLaunchKernelGGL(k_bow_score<false>, dim3(blocks), dim3(64 * kBowWaves), 0, stream, d_qw.p, d_qv.p, nq,
                               d_slot, d_word, d_weight, n_slots, d_common.p, d_first.p, d_score.p);
        HIPCK(hipGetLastError());
        t.end(stream);
        HIPCK(hipMemcpyAsync(common, d_common.p, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIPCK(hipMemcpyAsync(first, d_first.p, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIPCK(hipMemcpyAsync(score, d_score.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCK(hipStreamSynchronize(stream));
        t.last_ms = t.elapsed_ms();
    }
};

constexpr int64_t kManyScratchDefault = 64LL << 20;  // default limit of the dense intermediate, bytes
constexpr int64_t kManyRowBytes = 16;                // common + first + score of one (query, slot)
constexpr int kManyMaxChunk = 1 << 16;               // queries per chunk at the most (grid y = tiles of a chunk)

// Device scratch of the many-query calls.  up: one page-locked block for everything a call uploads, down: one for
// everything but the dense arrays that it brings back; each travels in one copy.
struct ManyScratch {
    DevBuf<int32_t> d_common, d_first;
    DevBuf<double> d_score;
    DevBuf<char> d_up, d_down;
    HostBuf<char> h_up, h_down;
    TimedStream t;  // its events only: the calls run on the handle's stream
    int64_t limit = kManyScratchDefault;
    ~ManyScratch() { t.destroy(); }
};

}  // namespace orbfe

struct orbfe_kfdb {
    // host master copy
    std::vector<int32_t> word;
    std::vector<double> weight;
    std::vector<KfdbSlot> slot;
    int64_t kf_cap = 1, word_cap = 1;  // capacities of the slot table and of the arena (entries)
    int64_t n_live = 0, live_words = 0, regrows = 0;
    // device copy: arena entries [0, up_words) and slots outside [dirty_lo, dirty_hi) are current
    DevBuf<int32_t> d_word;
    DevBuf<double> d_weight;
    DevBuf<KfdbSlot> d_slot;
    int64_t up_words = 0, dirty_lo = 0, dirty_hi = 0;
    BowScratch sc;
    ManyScratch many;
    // Tracking (relocalisation), LocalMapping (KeyFrame.set_bad_flag -> erase) and LoopClosing share one
    // database (System.py:45): everything above is guarded by this mutex
    std::mutex mu;
};

namespace {

// ascending, distinct, non-negative word ids
void check_vector(const int32_t* word, const double* weight, int32_t n, const char* what) {
    if (n < 0 || (n > 0 && (!word || !weight))) throw Error(ORBFE_EINVAL, std::string(what) + ": bad argument");
    for (int32_t i = 0; i < n; ++i)
        if (word[i] < 0 || (i > 0 && word[i] <= word[i - 1]))
            throw Error(ORBFE_EINVAL, std::string(what) + ": word ids must be distinct, non-negative and ascending");
}

void mark_dirty(orbfe_kfdb& d, int64_t lo, int64_t hi) {
    if (d.dirty_lo >= d.dirty_hi) {
        d.dirty_lo = lo;
        d.dirty_hi = hi;
    } else {
        d.dirty_lo = std::min(d.dirty_lo, lo);
        d.dirty_hi = std::max(d.dirty_hi, hi);
    }
}

// Drop erased vectors from the arena (slot numbers stay, offsets move) and double the capacities until
// need_words arena entries and need_slots table entries fit.  The device copy is rebuilt at the next query.
void regrow(orbfe_kfdb& d, int64_t need_words, int64_t need_slots) {
    int64_t o = 0;
    for (KfdbSlot& s : d.slot) {
        if (!s.live) {
            s.off = 0;
            s.len = 0;
            continue;
        }
        if (s.off != o) {
            std::memmove(&d.word[o], &d.word[s.off], (size_t)s.len * sizeof(int32_t));
            std::memmove(&d.weight[o], &d.weight[s.off], (size_t)s.len * sizeof(double));
            s.off = o;
        }
        o += s.len;
    }
    d.word.resize(o);
    d.weight.resize(o);
    while (d.word_cap < need_words + o) d.word_cap *= 2;
    while (d.kf_cap < need_slots) d.kf_cap *= 2;
    d.word.reserve(d.word_cap);
    d.weight.reserve(d.word_cap);
    d.slot.reserve(d.kf_cap);
    d.up_words = 0;
    d.dirty_lo = 0;
    d.dirty_hi = (int64_t)d.slot.size();
    ++d.regrows;
}

// Bring the device copy up to date: only the arena tail and the changed slot range travel.
void sync_device(orbfe_kfdb& d) {
    d.sc.t.get();
    if ((size_t)d.word_cap > d.d_word.n || !d.d_word.p) {  // first use, or the arena regrew
        d.d_word.ensure(d.word_cap);
        d.d_weight.ensure(d.word_cap);
        d.up_words = 0;
    }
    if ((size_t)d.kf_cap > d.d_slot.n || !d.d_slot.p) {
        d.d_slot.ensure(d.kf_cap);
        d.dirty_lo = 0;
        d.dirty_hi = (int64_t)d.slot.size();
    }
    const int64_t nw = (int64_t)d.word.size();
    if (nw > d.up_words) {
        const size_t k = (size_t)(nw - d.up_words);
        HIPCK(hipMemcpyAsync(d.d_word.p + d.up_words, &d.word[d.up_words], k * sizeof(int32_t), hipMemcpyHostToDevice,
                             d.sc.t.stream));
        HIPCK(hipMemcpyAsync(d.d_weight.p + d.up_words, &d.weight[d.up_words], k * sizeof(double),
                             hipMemcpyHostToDevice, d.sc.t.stream));
    }
    const int64_t hi = std::min<int64_t>(d.dirty_hi, (int64_t)d.slot.size());
    if (hi > d.dirty_lo)
        HIPCK(hipMemcpyAsync(d.d_slot.p + d.dirty_lo, &d.slot[d.dirty_lo], (size_t)(hi - d.dirty_lo) * sizeof(KfdbSlot),
                             hipMemcpyHostToDevice, d.sc.t.stream));
    // the host vectors must not move before the copies have read them
    HIPCK(hipStreamSynchronize(d.sc.t.stream));
    d.up_words = nw;
    d.dirty_lo = d.dirty_hi = 0;
}

// scratch of orbfe_bow_score: process-wide, created on first use and never torn down (the HIP runtime may
// already be gone when static destructors run)
struct PairScorer {
    std::mutex mu;
    BowScratch sc;
    DevBuf<int32_t> d_word;
    DevBuf<double> d_weight;
    DevBuf<KfdbSlot> d_slot;
    std::vector<KfdbSlot> slot;
};
PairScorer& pair_scorer() {
    static PairScorer* p = new PairScorer;
    return *p;
}

// ---- many queries ---------------------------------------------------------------------------------------------
struct ManyCall {  // what the two entries share
    int32_t n_query;
    const int64_t* excl_off;
    const int32_t* excl_slot;
    double gate_ratio;
    int32_t hit_cap;
    int64_t dense_stride;
    const orbfe_kfdb_many_out* out;
};

struct HostQueries {
    const int64_t* off;
    const int32_t* word;
    const double* weight;
    int64_t total;
};

// Everything that can be refused, before any device call.  Returns false when the call is answered here: no
// query, or an empty database (zeros).
bool check_many(orbfe_kfdb& d, const ManyCall& a, const char* what) {
    const std::string w(what);
    const orbfe_kfdb_many_out* o = a.out;
    if (!(a.gate_ratio >= 0.0 && a.gate_ratio < 1.0)) throw Error(ORBFE_EINVAL, w + ": gate_ratio must be in [0, 1)");
    if (a.hit_cap < 0 || a.dense_stride < 0) throw Error(ORBFE_EINVAL, w + ": negative hit_cap or dense_stride");
    if (a.n_query > 0) {
        if (!o || !o->n_sharing || !o->max_common || !o->n_hits) throw Error(ORBFE_EINVAL, w + ": null result array");
        if (a.hit_cap > 0 && (!o->hit_slot || !o->hit_common || !o->hit_first || !o->hit_score))
            throw Error(ORBFE_EINVAL, w + ": null hit array");
    }
    const int64_t ns = (int64_t)d.slot.size();
    if (a.excl_off && a.n_query > 0) {
        if (a.excl_off[0] != 0) throw Error(ORBFE_EINVAL, w + ": excl_off[0] must be 0");
        for (int32_t g = 0; g < a.n_query; ++g) {
            const int64_t lo = a.excl_off[g], hi = a.excl_off[g + 1];
            if (hi < lo || hi - lo > 0x7FFFFFFF) throw Error(ORBFE_EINVAL, w + ": excl_off must not descend");
            if (hi > lo && !a.excl_slot) throw Error(ORBFE_EINVAL, w + ": null excl_slot");
            for (int64_t i = lo; i < hi; ++i)
                if (a.excl_slot[i] < 0 || a.excl_slot[i] >= ns || (i > lo && a.excl_slot[i] <= a.excl_slot[i - 1]))
                    throw Error(ORBFE_EINVAL, w + ": excluded slots must ascend and lie below n_slots");
        }
    }
    if (a.n_query > 0 && (o->common || o->first || o->score) && a.dense_stride < ns)
        throw Error(ORBFE_ECAPACITY, w + ": dense rows are shorter than the slot table");
    d.many.t.last_ms = 0.f;
    if (a.n_query == 0) return false;
    if (ns == 0) {
        std::memset(o->n_sharing, 0, (size_t)a.n_query * sizeof(int32_t));
        std::memset(o->max_common, 0, (size_t)a.n_query * sizeof(int32_t));
        std::memset(o->n_hits, 0, (size_t)a.n_query * sizeof(int32_t));
        return false;
    }
    return true;
}

// The device half of a many-query call, on `stream`; returns with the results in the host buffers of a.out.
// hq != nullptr: the queries are uploaded (dq is ignored); otherwise dq names them on the device.  Queries go
// through the kernels in chunks whose dense intermediate fits the handle's scratch limit (one query at the
// least); a chunk's rows are copied out before the next chunk overwrites them, in stream order.
void run_many(orbfe_kfdb& d, const HostQueries* hq, BowQueries dq, const ManyCall& a, int lds_words,
              hipStream_t stream) {
    ManyScratch& m = d.many;
    const int64_t ns = (int64_t)d.slot.size();
    const size_t nq = (size_t)a.n_query, cap = (size_t)a.hit_cap;

    // one upload: weights | q_off | excl_off | words | excl_slot
    const size_t n_ex = a.excl_off ? (size_t)a.excl_off[nq] : 0;
    const size_t b_wt = hq ? pad_to((size_t)hq->total * sizeof(double), 8) : 0;
    const size_t b_qo = hq ? (nq + 1) * sizeof(int64_t) : 0;
    const size_t b_eo = a.excl_off ? (nq + 1) * sizeof(int64_t) : 0;
    const size_t b_wd = hq ? pad_to((size_t)hq->total * sizeof(int32_t), 8) : 0;
    const size_t b_es = pad_to(n_ex * sizeof(int32_t), 8);
    const size_t o_qo = b_wt, o_eo = o_qo + b_qo, o_wd = o_eo + b_eo, o_es = o_wd + b_wd, up = o_es + b_es;
    if (up) {
        m.h_up.ensure(up);
        m.d_up.ensure(up);
        if (hq) {
            std::memcpy(m.h_up.p, hq->weight, (size_t)hq->total * sizeof(double));
            std::memcpy(m.h_up.p + o_qo, hq->off, b_qo);
            std::memcpy(m.h_up.p + o_wd, hq->word, (size_t)hq->total * sizeof(int32_t));
        }
        if (a.excl_off) {
            std::memcpy(m.h_up.p + o_eo, a.excl_off, b_eo);
            std::memcpy(m.h_up.p + o_es, a.excl_slot, n_ex * sizeof(int32_t));
        }
        HIPCK(hipMemcpyAsync(m.d_up.p, m.h_up.p, up, hipMemcpyHostToDevice, stream));
    }
    if (hq)
        dq = BowQueries{(const int32_t*)(m.d_up.p + o_wd), (const double*)m.d_up.p, (const int64_t*)(m.d_up.p + o_qo),
                        nullptr, 0};
    const int64_t* d_eo = a.excl_off ? (const int64_t*)(m.d_up.p + o_eo) : nullptr;
    const int32_t* d_es = a.excl_off ? (const int32_t*)(m.d_up.p + o_es) : nullptr;

    // one download: hit_score | n_sharing | max_common | n_hits | hit_slot | hit_common | hit_first
    const size_t o_int = nq * cap * sizeof(double);
    const size_t down = o_int + (3 * nq + 3 * nq * cap) * sizeof(int32_t);
    m.h_down.ensure(down);
    m.d_down.ensure(down);
    double* d_hscore = (double*)m.d_down.p;
    int32_t* d_int = (int32_t*)(m.d_down.p + o_int);
    int32_t *d_nsh = d_int, *d_max = d_int + nq, *d_nh = d_int + 2 * nq, *d_hslot = d_int + 3 * nq;
    int32_t *d_hcommon = d_hslot + nq * cap, *d_hfirst = d_hcommon + nq * cap;

    const int64_t fit = std::max<int64_t>(1, m.limit / (ns * kManyRowBytes));
    const int chunk = (int)std::min<int64_t>(std::min<int64_t>(fit, a.n_query), kManyMaxChunk);
    m.d_common.ensure((size_t)chunk * ns);
    m.d_first.ensure((size_t)chunk * ns);
    m.d_score.ensure((size_t)chunk * ns);

    const orbfe_kfdb_many_out& o = *a.out;
    float total_ms = 0.f;
    for (int q0 = 0; q0 < a.n_query; q0 += chunk) {
        const int n = std::min(chunk, a.n_query - q0);
        const int tiles = (n + kBowTile - 1) / kBowTile;
        const int64_t want = (ns + kBowManyWaves - 1) / kBowManyWaves;
        const unsigned gx = (unsigned)std::min<int64_t>(want, std::max(1, kBowMaxBlocks / tiles));
        m.t.begin(stream);
        hipLaunchKernelGGL(k_bow_score_many, dim3(gx, tiles), dim3(64 * kBowManyWaves),
                           (size_t)lds_words * sizeof(int32_t), stream, dq, q0, n, lds_words, d.d_slot.p, d.d_word.p,
                           d.d_weight.p, ns, m.d_common.p, m.d_first.p, m.d_score.p);
        HIPCK(hipGetLastError());
        hipLaunchKernelGGL(k_bow_gate, dim3(n), dim3(kGateThreads), 0, stream, m.d_common.p, m.d_first.p, m.d_score.p,
                           d.d_slot.p, ns, q0, d_eo, d_es, a.gate_ratio, a.hit_cap, d_nsh, d_max, d_nh, d_hslot,
                           d_hcommon, d_hfirst, d_hscore);
        HIPCK(hipGetLastError());
        m.t.end(stream);
        const auto rows_out = [&](void* dst, const void* src, size_t elem) {
            if (!dst) return;
            char* to = (char*)dst + (size_t)q0 * a.dense_stride * elem;
            if (a.dense_stride == ns) {
                HIPCK(hipMemcpyAsync(to, src, (size_t)n * ns * elem, hipMemcpyDeviceToHost, stream));
            } else {
                for (int r = 0; r < n; ++r)
                    HIPCK(hipMemcpyAsync(to + (size_t)r * a.dense_stride * elem, (const char*)src + (size_t)r * ns * elem,
                                         (size_t)ns * elem, hipMemcpyDeviceToHost, stream));
            }
        };
        rows_out(o.common, m.d_common.p, sizeof(int32_t));
        rows_out(o.first, m.d_first.p, sizeof(int32_t));
        rows_out(o.score, m.d_score.p, sizeof(double));
        if (q0 + n == a.n_query)
            HIPCK(hipMemcpyAsync(m.h_down.p, m.d_down.p, down, hipMemcpyDeviceToHost, stream));
        HIPCK(hipStreamSynchronize(stream));
        total_ms += m.t.elapsed_ms();
    }
    m.t.last_ms = total_ms;

    const int32_t* h_int = (const int32_t*)(m.h_down.p + o_int);
    std::memcpy(o.n_sharing, h_int, nq * sizeof(int32_t));
    std::memcpy(o.max_common, h_int + nq, nq * sizeof(int32_t));
    std::memcpy(o.n_hits, h_int + 2 * nq, nq * sizeof(int32_t));
    if (cap) {
        std::memcpy(o.hit_score, m.h_down.p, nq * cap * sizeof(double));
        std::memcpy(o.hit_slot, h_int + 3 * nq, nq * cap * sizeof(int32_t));
        std::memcpy(o.hit_common, h_int + 3 * nq + nq * cap, nq * cap * sizeof(int32_t));
        std::memcpy(o.hit_first, h_int + 3 * nq + 2 * nq * cap, nq * cap * sizeof(int32_t));
    }
}

}  // namespace

extern "C" {

int orbfe_kfdb_create(int64_t kf_capacity, int64_t word_capacity, orbfe_kfdb_handle* out) {
    return guarded([&] {
        if (!out || kf_capacity < 1 || word_capacity < 1) throw Error(ORBFE_EINVAL, "bad argument");
        if (kf_capacity > (1LL << 31) || word_capacity > (1LL << 40)) throw Error(ORBFE_EINVAL, "capacity too large");
        auto d = std::make_unique<orbfe_kfdb>();
        d->kf_cap = kf_capacity;
        d->word_cap = word_capacity;
        d->slot.reserve(kf_capacity);
        d->word.reserve(word_capacity);
        d->weight.reserve(word_capacity);
        *out = d.release();
    });
}

int orbfe_kfdb_destroy(orbfe_kfdb_handle h) {
    return guarded([&] { delete h; });
}

int orbfe_kfdb_add(orbfe_kfdb_handle h, const int32_t* word, const double* weight, int32_t n, int64_t* slot) {
    return guarded([&] {
        if (!h || !slot) throw Error(ORBFE_EINVAL, "null argument");
        check_vector(word, weight, n, "orbfe_kfdb_add");
        std::lock_guard<std::mutex> lk(h->mu);
        orbfe_kfdb& d = *h;
        const int64_t ns = (int64_t)d.slot.size();
        if (ns >= 0x7FFFFFFF) throw Error(ORBFE_ECAPACITY, "slot table is full");
        if ((int64_t)d.word.size() + n > d.word_cap || ns + 1 > d.kf_cap) regrow(d, n, ns + 1);
        const int64_t off = (int64_t)d.word.size();
        d.word.insert(d.word.end(), word, word + n);
        d.weight.insert(d.weight.end(), weight, weight + n);
        d.slot.push_back(KfdbSlot{off, n, 1});
        mark_dirty(d, ns, ns + 1);
        ++d.n_live;
        d.live_words += n;
        *slot = ns;
    });
}

int orbfe_kfdb_erase(orbfe_kfdb_handle h, int64_t slot) {
    return guarded([&] {
        if (!h) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        orbfe_kfdb& d = *h;
        if (slot < 0 || slot >= (int64_t)d.slot.size()) throw Error(ORBFE_EINVAL, "no such slot");
        KfdbSlot& s = d.slot[slot];
        if (!s.live) throw Error(ORBFE_ESTATE, "slot is already erased");
        s.live = 0;
        --d.n_live;
        d.live_words -= s.len;
        mark_dirty(d, slot, slot + 1);
    });
}

int orbfe_kfdb_clear(orbfe_kfdb_handle h) {
    return guarded([&] {
        if (!h) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        orbfe_kfdb& d = *h;
        d.word.clear();
        d.weight.clear();
        d.slot.clear();
        d.n_live = d.live_words = 0;
        d.up_words = d.dirty_lo = d.dirty_hi = 0;
    });
}

int orbfe_kfdb_stats(orbfe_kfdb_handle h, int64_t* n_slots, int64_t* n_live, int64_t* live_words, int64_t* kf_capacity,
                     int64_t* word_capacity, int64_t* regrows) {
    return guarded([&] {
        if (!h) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        if (n_slots) *n_slots = (int64_t)h->slot.size();
        if (n_live) *n_live = h->n_live;
        if (live_words) *live_words = h->live_words;
        if (kf_capacity) *kf_capacity = h->kf_cap;
        if (word_capacity) *word_capacity = h->word_cap;
        if (regrows) *regrows = h->regrows;
    });
}

int orbfe_kfdb_query(orbfe_kfdb_handle h, const int32_t* q_word, const double* q_weight, int32_t nq, int32_t* common,
                     int32_t* first, double* score, int64_t cap) {
    return guarded([&] {
        if (!h || cap < 0) throw Error(ORBFE_EINVAL, "bad argument");
        check_vector(q_word, q_weight, nq, "orbfe_kfdb_query");
        std::lock_guard<std::mutex> lk(h->mu);
        orbfe_kfdb& d = *h;
        const int64_t ns = (int64_t)d.slot.size();
        if (cap < ns) throw Error(ORBFE_ECAPACITY, "result arrays are shorter than the slot table");
        d.sc.t.last_ms = 0.f;
        if (ns == 0) return;
        if (!common || !first || !score) throw Error(ORBFE_EINVAL, "null result array");
        sync_device(d);
        d.sc.run(q_word, q_weight, nq, d.d_slot.p, d.d_word.p, d.d_weight.p, ns, common, first, score);
    });
}

int orbfe_bow_score(const int32_t* q_word, const double* q_weight, int32_t nq, const int64_t* off, const int32_t* word,
                    const double* weight, int32_t n_vec, int32_t* common, int32_t* first, double* score) {
    return guarded([&] {
        if (n_vec < 0 || (n_vec > 0 && (!off || !common || !first || !score)))
            throw Error(ORBFE_EINVAL, "bad argument");
        check_vector(q_word, q_weight, nq, "orbfe_bow_score");
        if (n_vec == 0) return;
        if (off[0] != 0) throw Error(ORBFE_EINVAL, "off[0] must be 0");
        PairScorer& p = pair_scorer();
        std::lock_guard<std::mutex> lk(p.mu);
        p.slot.resize(n_vec);
        for (int32_t v = 0; v < n_vec; ++v) {
            const int64_t len = off[v + 1] - off[v];
            if (len < 0 || len > 0x7FFFFFFF) throw Error(ORBFE_EINVAL, "offsets must ascend");
            check_vector(len ? word + off[v] : nullptr, len ? weight + off[v] : nullptr, (int32_t)len,
                         "orbfe_bow_score");
            p.slot[v] = KfdbSlot{off[v], (int32_t)len, 1};
        }
        const int64_t total = off[n_vec];
        p.sc.t.get();
        p.d_word.ensure(total);
        p.d_weight.ensure(total);
        p.d_slot.ensure(n_vec);
        if (total) {
            HIPCK(hipMemcpyAsync(p.d_word.p, word, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice,
                                 p.sc.t.stream));
            HIPCK(hipMemcpyAsync(p.d_weight.p, weight, (size_t)total * sizeof(double), hipMemcpyHostToDevice,
                                 p.sc.t.stream));
        }
        HIPCK(hipMemcpyAsync(p.d_slot.p, p.slot.data(), (size_t)n_vec * sizeof(KfdbSlot), hipMemcpyHostToDevice,
                             p.sc.t.stream));
        p.sc.run(q_word, q_weight, nq, p.d_slot.p, p.d_word.p, p.d_weight.p, n_vec, common, first, score);
    });
}

int orbfe_kfdb_query_many(orbfe_kfdb_handle h, const int64_t* q_off, const int32_t* q_word, const double* q_weight,
                          int32_t n_query, const int64_t* excl_off, const int32_t* excl_slot, double gate_ratio,
                          int32_t hit_cap, int64_t dense_stride, const orbfe_kfdb_many_out* out) {
    return guarded([&] {
        if (!h) throw Error(ORBFE_EINVAL, "null handle");
        if (n_query < 0 || (n_query > 0 && !q_off)) throw Error(ORBFE_EINVAL, "bad argument");
        int64_t total = 0;
        if (n_query > 0) {
            if (q_off[0] != 0) throw Error(ORBFE_EINVAL, "q_off[0] must be 0");
            for (int32_t g = 0; g < n_query; ++g) {
                const int64_t len = q_off[g + 1] - q_off[g];
                if (len < 0 || len > 0x7FFFFFFF) throw Error(ORBFE_EINVAL, "q_off must not descend");
            }
            total = q_off[n_query];
            if (total > 0 && (!q_word || !q_weight)) throw Error(ORBFE_EINVAL, "null query arrays");
            for (int32_t g = 0; g < n_query; ++g) {
                const int64_t len = q_off[g + 1] - q_off[g];
                check_vector(len ? q_word + q_off[g] : nullptr, len ? q_weight + q_off[g] : nullptr, (int32_t)len,
                             "orbfe_kfdb_query_many");
            }
        }
        std::lock_guard<std::mutex> lk(h->mu);
        ManyCall a{n_query, excl_off, excl_slot, gate_ratio, hit_cap, dense_stride, out};
        if (!check_many(*h, a, "orbfe_kfdb_query_many")) return;
        // the LDS a tile needs: its queries packed one after the other, as the kernel packs them
        int lds_words = 0;
        for (int32_t g0 = 0; g0 < n_query; g0 += kBowTile) {
            int used = 0;
            for (int32_t g = g0; g < std::min(n_query, g0 + kBowTile); ++g) {
                const int64_t len = q_off[g + 1] - q_off[g];
                if (len <= kBowLdsWords && used + len <= kBowTileLdsWords) used += (int)len;
            }
            lds_words = std::max(lds_words, used);
        }
        sync_device(*h);
        HostQueries hq{q_off, q_word, q_weight, total};
        run_many(*h, &hq, BowQueries{}, a, lds_words, h->sc.t.stream);
    });
}

int orbfe_kfdb_query_many_device(orbfe_kfdb_handle h, const orbfe_bow_out* d_bow, int64_t bow_stride, int32_t n_query,
                                 const int64_t* excl_off, const int32_t* excl_slot, double gate_ratio,
                                 int32_t hit_cap, int64_t dense_stride, const orbfe_kfdb_many_out* out,
                                 void* hip_stream) {
    return guarded([&] {
        if (!h) throw Error(ORBFE_EINVAL, "null handle");
        if (n_query < 0 || bow_stride < 0 || bow_stride > 0x7FFFFFFF) throw Error(ORBFE_EINVAL, "bad argument");
        if (n_query > 0 && (!d_bow || !d_bow->n_words || (bow_stride > 0 && (!d_bow->bow_word || !d_bow->bow_weight))))
            throw Error(ORBFE_EINVAL, "null BoW arrays");
        std::lock_guard<std::mutex> lk(h->mu);
        ManyCall a{n_query, excl_off, excl_slot, gate_ratio, hit_cap, dense_stride, out};
        if (!check_many(*h, a, "orbfe_kfdb_query_many_device")) return;
        sync_device(*h);
        const int lds_words = (int)std::min<int64_t>(kBowTile * std::min<int64_t>(bow_stride, kBowLdsWords),
                                                     kBowTileLdsWords);
        run_many(*h, nullptr, BowQueries{d_bow->bow_word, d_bow->bow_weight, nullptr, d_bow->n_words, bow_stride}, a,
                 lds_words, (hipStream_t)hip_stream);
    });
}

int orbfe_kfdb_set_scratch_limit(orbfe_kfdb_handle h, int64_t bytes) {
    return guarded([&] {
        if (!h || bytes < 0) throw Error(ORBFE_EINVAL, "bad argument");
        std::lock_guard<std::mutex> lk(h->mu);
        h->many.limit = bytes;
    });
}

int orbfe_kfdb_many_last_ms(orbfe_kfdb_handle h, float* ms) {
    return guarded([&] {
        if (!h || !ms) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *ms = h->many.t.last_ms;
    });
}

int orbfe_kfdb_last_ms(orbfe_kfdb_handle h, float* ms) {
    return guarded([&] {
        if (!h || !ms) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *ms = h->sc.t.last_ms;
    });
}

}  // extern "C"
