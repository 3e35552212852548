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

// One stored vector per wave.  Per pass of 64 * kBowUnroll words, lane j takes words j, j + 64, ... of the
// pass and binary-searches the query for each (LDS copy when LDS is true, global otherwise).  The search is
// the branchless halving form, whose trip count depends on nq alone: every lane runs the same steps, and the
// kBowUnroll searches of a lane are independent, so their reads overlap instead of queueing behind one
// another (the kernel is bound by that chain's latency).  Then, 64 words at a time in
// ascending order: the ballot of the hits gives common and first; only hit lanes fetch the two weights and
// form their term; the terms are added to the wave-uniform running sum in ascending lane order (= ascending
// word id) by walking the ballot's set bits with a lane read, so the sum is the sequential one whatever the
// chunking.
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
            int w[kBowUnroll], base[kBowUnroll];
#pragma unroll
            for (int u = 0; u < kBowUnroll; ++u) {
                const int j = c + u * 64 + lane;
                w[u] = j < len ? word[sl.off + j] : -1;  // ids are non-negative: -1 matches nothing
                base[u] = 0;
            }
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
                    const double wi = weight[sl.off + c + u * 64 + lane];
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
        if (lane == 0) {
            out_common[s] = common;
            out_first[s] = first;
            out_score[s] = -sum / 2.0;
        }
    }
}

// Device scratch of one scorer: the query, the three result arrays, a stream and two events.
struct BowScratch {
    DevBuf<int32_t> d_qw, d_common, d_first;
    DevBuf<double> d_qv, d_score;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.f;
    ~BowScratch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
    void init() {
        if (!stream) HIPCK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (hipEvent_t& e : ev)
            if (!e) HIPCK(hipEventCreate(&e));
    }
    // query upload, one launch over n_slots device-resident vectors, results to host buffers; synchronous
    void run(const int32_t* q_word, const double* q_weight, int32_t nq, const KfdbSlot* d_slot, const int32_t* d_word,
             const double* d_weight, int64_t n_slots, int32_t* common, int32_t* first, double* score) {
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
        HIPCK(hipEventRecord(ev[0], stream));
        if (nq <= kBowLdsWords)
            hipLaunchKernelGGL(k_bow_score<true>, dim3(blocks), dim3(64 * kBowWaves), (size_t)nq * sizeof(int32_t),
                               stream, d_qw.p, d_qv.p, nq, d_slot, d_word, d_weight, n_slots, d_common.p, d_first.p,
                               d_score.p);
        else
            hipLaunchKernelGGL(k_bow_score<false>, dim3(blocks), dim3(64 * kBowWaves), 0, stream, d_qw.p, d_qv.p, nq,
                               d_slot, d_word, d_weight, n_slots, d_common.p, d_first.p, d_score.p);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(ev[1], stream));
        HIPCK(hipMemcpyAsync(common, d_common.p, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIPCK(hipMemcpyAsync(first, d_first.p, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIPCK(hipMemcpyAsync(score, d_score.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCK(hipStreamSynchronize(stream));
        HIPCK(hipEventElapsedTime(&last_ms, ev[0], ev[1]));
    }
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
    d.sc.init();
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
                             d.sc.stream));
        HIPCK(hipMemcpyAsync(d.d_weight.p + d.up_words, &d.weight[d.up_words], k * sizeof(double),
                             hipMemcpyHostToDevice, d.sc.stream));
    }
    const int64_t hi = std::min<int64_t>(d.dirty_hi, (int64_t)d.slot.size());
    if (hi > d.dirty_lo)
        HIPCK(hipMemcpyAsync(d.d_slot.p + d.dirty_lo, &d.slot[d.dirty_lo], (size_t)(hi - d.dirty_lo) * sizeof(KfdbSlot),
                             hipMemcpyHostToDevice, d.sc.stream));
    // the host vectors must not move before the copies have read them
    HIPCK(hipStreamSynchronize(d.sc.stream));
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
        d.sc.last_ms = 0.f;
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
        p.sc.init();
        p.d_word.ensure(total);
        p.d_weight.ensure(total);
        p.d_slot.ensure(n_vec);
        if (total) {
            HIPCK(hipMemcpyAsync(p.d_word.p, word, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice,
                                 p.sc.stream));
            HIPCK(hipMemcpyAsync(p.d_weight.p, weight, (size_t)total * sizeof(double), hipMemcpyHostToDevice,
                                 p.sc.stream));
        }
        HIPCK(hipMemcpyAsync(p.d_slot.p, p.slot.data(), (size_t)n_vec * sizeof(KfdbSlot), hipMemcpyHostToDevice,
                             p.sc.stream));
        p.sc.run(q_word, q_weight, nq, p.d_slot.p, p.d_word.p, p.d_weight.p, n_vec, common, first, score);
    });
}

int orbfe_kfdb_last_ms(orbfe_kfdb_handle h, float* ms) {
    return guarded([&] {
        if (!h || !ms) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *ms = h->sc.last_ms;
    });
}

}  // extern "C"
