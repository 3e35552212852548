// orbfe_vocabtrain.hip — training a bag-of-words vocabulary tree on gfx950 (DBoW2's create: hierarchical k-means
// with kmeans++ seeding over 256-bit ORB descriptors), and the text writer.
//
// The build is level-synchronous: one set of launches serves every node of a depth that is being split.  The
// members of the nodes of a depth lie contiguously in `order` (indices into D, ascending inside a node), and a node
// with more than k members is cut into chunks of at most kTrainChunk positions; one 256-thread workgroup takes one
// chunk, so a workgroup never spans two nodes and a large node spans many workgroups.  Everything is integer
// (Hamming distances, popcounts, per-bit counts), so every sum is independent of the order it is formed in.  The
// host drives `seed; repeat (mean, assign) until no node changed or max_iter` and reads back only per-node words
// (S of the seeding, the changed flags) and per-chunk cluster counts.  No kernel waits on another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host_util.h"

using namespace orbfe;

namespace orbfe {

constexpr int kTrainThreads = 256;  // workgroup size of every kernel here
constexpr int kTrainChunk = 2048;   // positions one workgroup takes: 8 per thread
constexpr int kTrainMaxK = 20;

// a node with more than k members that is being split (positions into `order`)
struct TrainSeg {
    int32_t start, len;
    int32_t ncent;  // centres the seeding gave (<= k)
    int32_t slot;   // index of its global bit counters when it spans several chunks, else -1
};
struct TrainChunk {
    int32_t seg, begin, end, pad;
};

// Sum over the workgroup; every thread gets it.  wsum: kTrainThreads / 64 words of LDS, free again on return.
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* wsum, int tid) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = v;
    __syncthreads();
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kTrainThreads / 64; ++w) t += wsum[w];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(kTrainThreads) void k_train_iota(int32_t* __restrict__ order, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kTrainThreads + threadIdx.x;
    if (i < n) order[i] = (int32_t)i;
}

// Seeding, the pick of centre j.  One workgroup per node.  direct: cutv[s] is the member's rank (centre 0).
// Otherwise cutv[s] is the cut (0: the node's seeding has stopped), and the pick is the first member, in member
// order, whose running sum of md reaches it: the workgroup scans its node kTrainChunk members at a time.
__global__ __launch_bounds__(kTrainThreads) void k_train_seed_pick(const TrainSeg* __restrict__ seg,
                                                                   const int64_t* __restrict__ cutv, int direct, int j,
                                                                   int k, const uint32_t* __restrict__ md,
                                                                   const int32_t* __restrict__ order,
                                                                   const uint4* __restrict__ D, uint4* __restrict__ cent,
                                                                   int32_t* __restrict__ pick) {
    __shared__ unsigned wsum[kTrainThreads / 64];
    __shared__ int s_found;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TrainSeg sg = seg[s];
    const int64_t cut = cutv[s];
    int pos = -1;
    if (direct) {
        if (cut >= 0 && cut < sg.len) pos = sg.start + (int)cut;
    } else if (cut > 0) {
        if (tid == 0) s_found = -1;
        __syncthreads();
        constexpr int kItems = kTrainChunk / kTrainThreads;
        int64_t running = 0;
        for (int64_t base = 0; base < sg.len; base += kTrainChunk) {  // 64-bit: base + 2 047 may pass 2^31
            const int64_t i0 = base + tid * kItems;
            unsigned v[kItems], sum = 0;
#pragma unroll
            for (int it = 0; it < kItems; ++it) {
                v[it] = i0 + it < sg.len ? md[sg.start + i0 + it] : 0u;
                sum += v[it];
            }
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned x = __shfl_up(incl, o, 64);
                if (lane >= o) incl += x;
            }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kTrainThreads / 64; ++w) {
                if (w < wave) before += wsum[w];
                total += wsum[w];
            }
            int64_t pre = running + before + (incl - sum);
            if (pre < cut && pre + sum >= cut) {  // the crossing lies in this thread's items: one thread at most
#pragma unroll
                for (int it = 0; it < kItems; ++it) {
                    if (pre < cut && pre + v[it] >= cut) s_found = (int)(sg.start + i0 + it);
                    pre += v[it];
                }
            }
            __syncthreads();
            if (s_found >= 0) break;
            running += total;
        }
        pos = s_found;
    }
    if (pos >= 0 && tid < 2) cent[((int64_t)s * k + j) * 2 + tid] = D[(int64_t)order[pos] * 2 + tid];
    if (tid == 0) pick[s] = pos;
}

// Seeding, after centre j was picked: md_i = min(md_i, distance to centre j) and S = sum of md, one 64-bit atomic
// per workgroup.  Nodes whose seeding has stopped (pick < 0) are left alone.
__global__ __launch_bounds__(kTrainThreads) void k_train_seed_dist(const TrainChunk* __restrict__ chunk, int j, int k,
                                                                   const int32_t* __restrict__ pick,
                                                                   const int32_t* __restrict__ order,
                                                                   const uint4* __restrict__ D,
                                                                   const uint4* __restrict__ cent,
                                                                   uint32_t* __restrict__ md,
                                                                   unsigned long long* __restrict__ S) {
    __shared__ unsigned wsum[kTrainThreads / 64];
    const TrainChunk c = chunk[blockIdx.x];
    const int tid = threadIdx.x;
    if (pick[c.seg] < 0) return;  // the whole workgroup leaves together
    const uint4 c0 = cent[((int64_t)c.seg * k + j) * 2], c1 = cent[((int64_t)c.seg * k + j) * 2 + 1];
    unsigned sum = 0;
    for (int o = tid; o < c.end - c.begin; o += kTrainThreads) {  // by offset: pos + 256 may pass 2^31
        const int pos = c.begin + o;
        const int64_t i = order[pos];
        unsigned d = hamming256(D[i * 2], D[i * 2 + 1], c0, c1);
        if (j > 0) d = min(d, md[pos]);
        md[pos] = d;
        sum += d;
    }
    sum = block_sum(sum, wsum, tid);
    if (tid == 0 && sum) atomicAdd(&S[c.seg], (unsigned long long)sum);
}

// Assignment: every member against its node's centres, lowest cluster index on ties.  changed[s] is set when any
// member of node s moved.
__global__ __launch_bounds__(kTrainThreads) void k_train_assign(const TrainChunk* __restrict__ chunk,
                                                                const TrainSeg* __restrict__ seg, int k,
                                                                const int32_t* __restrict__ order,
                                                                const uint4* __restrict__ D,
                                                                const uint4* __restrict__ cent,
                                                                uint8_t* __restrict__ assign,
                                                                int32_t* __restrict__ changed) {
    __shared__ uint4 sc[kTrainMaxK * 2];
    const TrainChunk c = chunk[blockIdx.x];
    const int tid = threadIdx.x;
    const int nc = min(seg[c.seg].ncent, kTrainMaxK);
    if (tid < nc * 2) sc[tid] = cent[(int64_t)c.seg * k * 2 + tid];
    __syncthreads();
    int moved = 0;
    for (int o = tid; o < c.end - c.begin; o += kTrainThreads) {
        const int pos = c.begin + o;
        const int64_t i = order[pos];
        const uint4 q0 = D[i * 2], q1 = D[i * 2 + 1];
        int best = 0, bd = (int)hamming256(q0, q1, sc[0], sc[1]);
        for (int cc = 1; cc < nc; ++cc) {
            const int d = (int)hamming256(q0, q1, sc[2 * cc], sc[2 * cc + 1]);
            if (d < bd) bd = d, best = cc;
        }
        if (assign[pos] != (uint8_t)best) {
            assign[pos] = (uint8_t)best;
            moved = 1;
        }
    }
    if (__syncthreads_or(moved) && tid == 0) changed[c.seg] = 1;
}

// bit `tid` of centre c from its count: FORB.meanValue's threshold n / 2 + n % 2.  Lane 0 of every wave stores the
// wave's 64 bits.
__device__ __forceinline__ void store_majority(uint32_t* cent32, int64_t centre, int tid, unsigned cnt, unsigned n) {
    const unsigned long long bits = __ballot(cnt >= n / 2 + n % 2);
    if ((tid & 63) == 0) {
        cent32[centre * 8 + (tid >> 6) * 2] = (uint32_t)bits;
        cent32[centre * 8 + (tid >> 6) * 2 + 1] = (uint32_t)(bits >> 32);
    }
}

// Mean step: thread t counts bit t (bit t & 31 of 32-bit word t >> 5) of the chunk's members per cluster, in its
// own column of LDS counters.  A node of one chunk gets its new centres here; a node of several chunks adds its
// non-zero counters to the node's global ones (one atomic per workgroup, cluster and counter) and
// k_train_mean_final takes the majority.  A cluster without members keeps its centre.
__global__ __launch_bounds__(kTrainThreads) void k_train_mean(const TrainChunk* __restrict__ chunk,
                                                              const TrainSeg* __restrict__ seg, int k,
                                                              const int32_t* __restrict__ order,
                                                              const uint32_t* __restrict__ D32,
                                                              const uint8_t* __restrict__ assign,
                                                              uint32_t* __restrict__ cent32,
                                                              uint32_t* __restrict__ gcnt, uint32_t* __restrict__ gn) {
    __shared__ unsigned cnt[kTrainMaxK * kTrainThreads];
    __shared__ uint32_t tile[kTrainThreads * 8];
    __shared__ uint8_t ta[kTrainThreads];
    __shared__ unsigned sn[kTrainMaxK];
    const TrainChunk c = chunk[blockIdx.x];
    const TrainSeg sg = seg[c.seg];
    const int tid = threadIdx.x;
    const int nc = min(sg.ncent, kTrainMaxK);
    for (int cc = 0; cc < nc; ++cc) cnt[cc * kTrainThreads + tid] = 0;
    unsigned mine = 0;  // members of cluster `tid` (threads below nc)
    for (int o = 0; o < c.end - c.begin; o += kTrainThreads) {
        const int base = c.begin + o;
        const int m = min(kTrainThreads, c.end - base);
        __syncthreads();  // the previous tile has been read
        for (int x = tid; x < m * 8; x += kTrainThreads) tile[x] = D32[(int64_t)order[base + (x >> 3)] * 8 + (x & 7)];
        if (tid < m) ta[tid] = assign[base + tid];
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const int cc = min((int)ta[i], nc - 1);
            cnt[cc * kTrainThreads + tid] += (tile[i * 8 + (tid >> 5)] >> (tid & 31)) & 1u;
            mine += cc == tid;
        }
    }
    if (tid < nc) sn[tid] = mine;
    __syncthreads();
    if (sg.slot < 0) {
        for (int cc = 0; cc < nc; ++cc) {
            const unsigned n = sn[cc];  // uniform: the whole workgroup skips an empty cluster together
            if (n) store_majority(cent32, (int64_t)c.seg * k + cc, tid, cnt[cc * kTrainThreads + tid], n);
        }
    } else {
        for (int cc = 0; cc < nc; ++cc) {
            const unsigned v = cnt[cc * kTrainThreads + tid];
            if (v) atomicAdd(&gcnt[((int64_t)sg.slot * k + cc) * kTrainThreads + tid], v);
        }
        if (tid < nc && mine) atomicAdd(&gn[(int64_t)sg.slot * k + tid], mine);
    }
}

// The majority of the nodes that span several chunks, one workgroup per node; the counters are left at zero for
// the next iteration.
__global__ __launch_bounds__(kTrainThreads) void k_train_mean_final(const int32_t* __restrict__ slot_seg,
                                                                    const TrainSeg* __restrict__ seg, int k,
                                                                    uint32_t* __restrict__ cent32,
                                                                    uint32_t* __restrict__ gcnt,
                                                                    uint32_t* __restrict__ gn) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int s = slot_seg[slot];
    const int nc = min(seg[s].ncent, kTrainMaxK);
    for (int cc = 0; cc < nc; ++cc) {
        const unsigned n = gn[(int64_t)slot * k + cc];
        if (!n) continue;
        const int64_t at = ((int64_t)slot * k + cc) * kTrainThreads + tid;
        store_majority(cent32, (int64_t)s * k + cc, tid, gcnt[at], n);
        gcnt[at] = 0;
    }
    __syncthreads();  // every thread has read gn
    if (tid < nc) gn[(int64_t)slot * k + tid] = 0;
}

// Members per cluster of every chunk: row blockIdx.x of ccount, k entries.
__global__ __launch_bounds__(kTrainThreads) void k_train_count(const TrainChunk* __restrict__ chunk, int k,
                                                               const uint8_t* __restrict__ assign,
                                                               int32_t* __restrict__ ccount) {
    __shared__ int hist[kTrainMaxK];
    const TrainChunk c = chunk[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid < kTrainMaxK) hist[tid] = 0;
    __syncthreads();
    for (int o = tid; o < c.end - c.begin; o += kTrainThreads) {
        const int cc = assign[c.begin + o];
        if (cc < k) atomicAdd(&hist[cc], 1);
    }
    __syncthreads();
    if (tid < k) ccount[(int64_t)blockIdx.x * k + tid] = hist[tid];
}

// Stable partition of a depth's members by child: cbase[chunk][c] is where the chunk's members of cluster c go in
// the next depth's order (-1: that child is not split further, its members are dropped).  Inside a chunk the
// members keep their order: per tile of 256, a member's rank among its cluster is its rank inside its wave (ballot
// of the cluster, popcount below the lane) plus the counts of the waves before it.
__global__ __launch_bounds__(kTrainThreads) void k_train_scatter(const TrainChunk* __restrict__ chunk, int k,
                                                                 const int32_t* __restrict__ order,
                                                                 const uint8_t* __restrict__ assign,
                                                                 const int32_t* __restrict__ cbase,
                                                                 int32_t* __restrict__ next_order) {
    __shared__ int run[kTrainMaxK];
    __shared__ int wcnt[kTrainThreads / 64][kTrainMaxK];
    const TrainChunk c = chunk[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < k) run[tid] = cbase[(int64_t)blockIdx.x * k + tid];
    for (int o = 0; o < c.end - c.begin; o += kTrainThreads) {
        const bool in = o + tid < c.end - c.begin;
        const int pos = in ? c.begin + o + tid : c.begin;
        int cc = in ? (int)assign[pos] : -1;
        if (cc >= k) cc = -1;
        int rank = 0;
        for (int x = 0; x < k; ++x) {
            const unsigned long long m = __ballot(cc == x);
            if (cc == x) rank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[wave][x] = __popcll(m);
        }
        __syncthreads();  // wcnt, and run[] of the previous tile
        if (cc >= 0 && run[cc] >= 0) {
            int at = run[cc] + rank;
            for (int w = 0; w < wave; ++w) at += wcnt[w][cc];
            next_order[at] = order[pos];
        }
        __syncthreads();
        if (tid < k && run[tid] >= 0)
            for (int w = 0; w < kTrainThreads / 64; ++w) run[tid] += wcnt[w][tid];
        __syncthreads();  // wcnt is free for the next tile
    }
}

// The descriptors of a depth's children: src >= 0 is a centre (node * k + cluster), src < 0 the member at position
// -src - 1 of order (nodes with n <= k, whose members are their clusters).
__global__ __launch_bounds__(kTrainThreads) void k_train_emit(const int64_t* __restrict__ src, int64_t n,
                                                              const int32_t* __restrict__ order,
                                                              const uint4* __restrict__ D,
                                                              const uint4* __restrict__ cent, uint4* __restrict__ out) {
    const int64_t x = (int64_t)blockIdx.x * kTrainThreads + threadIdx.x;
    if (x >= n * 2) return;
    const int64_t sv = src[x >> 1];
    out[x] = sv >= 0 ? cent[sv * 2 + (x & 1)] : D[(int64_t)order[-sv - 1] * 2 + (x & 1)];
}

// Ni: the first descriptor of image f to reach word w claims the pair in an open-addressing table (at most n keys
// in at least 2 n places, so a probe sequence ends) and counts the image for the word.
__global__ __launch_bounds__(kTrainThreads) void k_train_mark(const int32_t* __restrict__ word, int64_t n,
                                                              const int64_t* __restrict__ off, int n_frames,
                                                              unsigned long long* __restrict__ table,
                                                              unsigned long long mask, int32_t* __restrict__ ni) {
    const int64_t i = (int64_t)blockIdx.x * kTrainThreads + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_frames;  // the last f with off[f] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const int w = word[i];
    const unsigned long long key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)w;
    unsigned long long h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
        const unsigned long long at = (h + probe) & mask;
        const unsigned long long prev = atomicCAS(&table[at], ~0ull, key);
        if (prev == ~0ull) {
            atomicAdd(&ni[w], 1);
            return;
        }
        if (prev == key) return;
    }
}

}  // namespace orbfe

namespace {

uint64_t splitmix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

uint64_t draw(uint64_t seed, int64_t node, int j) {
    return splitmix64(seed + (32ull * (uint64_t)node + (uint64_t)j + 1ull) * 0x9E3779B97F4A7C15ull);
}

struct HostSeg {  // a node of the current depth that is being split
    int32_t node, start, len;
    int32_t large;  // index among the nodes with more than k members, or -1
};

struct Trainer {
    hipStream_t s = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    DevBuf<uint4> D, cent, out;
    DevBuf<int32_t> order[2], pick, changed, ccount, cbase, slot_seg, word, node, ni;
    DevBuf<uint8_t> assign;
    DevBuf<uint32_t> md, gcnt, gn;
    DevBuf<unsigned long long> S, table;
    DevBuf<int64_t> cutv, src, off;
    DevBuf<double> w;
    DevBuf<TrainSeg> seg;
    DevBuf<TrainChunk> chunk;
    ~Trainer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
    }
    template <class T>
    void up(T* dst, const std::vector<T>& v) {  // the vector may change once this returns
        if (v.empty()) return;
        HIPCK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        HIPCK(hipStreamSynchronize(s));
    }
    template <class T>
    void down(std::vector<T>& v, const T* src, size_t n) {
        v.resize(n);
        if (n) HIPCK(hipMemcpyAsync(v.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
};

unsigned blocks_for(int64_t n) { return (unsigned)((n + kTrainThreads - 1) / kTrainThreads); }

void train(const uint8_t* desc32, bool on_device, const int64_t* start, const int32_t* count, int32_t n_frames,
           const orbfe_vocab_train_params& p, orbfe_vocab_handle* out, orbfe_vocab_train_stats& st) {
    const int k = p.k, L = p.L;
    std::vector<int64_t> off((size_t)n_frames + 1, 0);
    for (int32_t f = 0; f < n_frames; ++f) off[f + 1] = off[f] + count[f];
    const int64_t N = off[n_frames];
    st.n_desc = N;

    // the tree, per node (node 0 = root)
    std::vector<int32_t> parent(1, 0);
    std::vector<uint8_t> desc(32, 0);
    auto finish = [&](const std::vector<double>* weight) {
        const int64_t nn = (int64_t)parent.size();
        std::vector<uint8_t> leaf(nn, 1);
        for (int64_t i = 1; i < nn; ++i) leaf[parent[i]] = 0;
        leaf[0] = 0;
        std::vector<double> zero;
        if (!weight) zero.assign(nn, 0.0);
        orbfe_vocab_handle h = nullptr;
        const int rc = orbfe_vocab_create(k, L, p.scoring, p.weighting, nn, parent.data(), leaf.data(), desc.data(),
                                          weight ? weight->data() : zero.data(), &h);
        if (rc != ORBFE_OK) throw Error(rc, g_err);
        return h;
    };
    if (N == 0) {
        st.n_nodes = 1;
        *out = finish(nullptr);
        return;
    }

    Trainer t;
    HIPCK(hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking));
    for (hipEvent_t& e : t.ev) HIPCK(hipEventCreate(&e));
    t.D.ensure((size_t)N * 2);
    for (int32_t f = 0; f < n_frames;) {  // one copy per run of images that are adjacent in desc32
        int32_t g = f;
        while (g + 1 < n_frames && start[g + 1] == start[g] + count[g]) ++g;
        const int64_t len = off[g + 1] - off[f];
        if (len)
            HIPCK(hipMemcpyAsync(t.D.p + off[f] * 2, desc32 + start[f] * 32, (size_t)len * 32,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, t.s));
        f = g + 1;
    }
    t.order[0].ensure(N);
    t.order[1].ensure(N);
    t.assign.ensure(N);
    t.md.ensure(N);
    hipLaunchKernelGGL(k_train_iota, dim3(blocks_for(N)), dim3(kTrainThreads), 0, t.s, t.order[0].p, N);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(t.s));  // desc32 has been read

    std::vector<HostSeg> segs{{0, 0, (int32_t)N, -1}};
    int cur = 0;
    for (int depth = 0; depth < L && !segs.empty(); ++depth) {
        HIPCK(hipEventRecord(t.ev[0], t.s));
        int32_t* order = t.order[cur].p;
        // the nodes that iterate, their chunks
        std::vector<TrainSeg> lseg;
        std::vector<int32_t> lnode, slot_seg;
        int64_t npos = 0;
        for (HostSeg& h : segs) {
            npos = std::max<int64_t>(npos, (int64_t)h.start + h.len);
            if (h.len <= k) continue;
            h.large = (int32_t)lseg.size();
            int32_t slot = -1;
            if (h.len > kTrainChunk) {
                slot = (int32_t)slot_seg.size();
                slot_seg.push_back(h.large);
            }
            lseg.push_back(TrainSeg{h.start, h.len, 0, slot});
            lnode.push_back(h.node);
        }
        const size_t nl = lseg.size();
        std::vector<TrainChunk> chunks;
        std::vector<char> live(nl, 1);
        auto build_chunks = [&] {
            chunks.clear();
            for (size_t s = 0; s < nl; ++s)
                if (live[s])
                    for (int32_t b = 0; b < lseg[s].len; b += kTrainChunk)
                        chunks.push_back(TrainChunk{(int32_t)s, lseg[s].start + b,
                                                    lseg[s].start + std::min(b + kTrainChunk, lseg[s].len), 0});
            t.chunk.ensure(chunks.size());
            t.up(t.chunk.p, chunks);
        };
        std::vector<int32_t> iters(nl, 0);
        std::vector<char> capped(nl, 0);
        if (nl) {
            build_chunks();
            const unsigned nch_all = (unsigned)chunks.size();
            t.seg.ensure(nl);
            t.up(t.seg.p, lseg);
            t.cent.ensure(nl * (size_t)k * 2);
            t.pick.ensure(nl);
            t.cutv.ensure(nl);
            t.S.ensure(nl);
            t.changed.ensure(nl);
            // ---- seeding ----
            std::vector<int64_t> cutv(nl);
            std::vector<char> seeding(nl, 1);
            for (size_t s = 0; s < nl; ++s) {
                cutv[s] = (int64_t)(draw(p.seed, lnode[s], 0) % (uint64_t)lseg[s].len);
                lseg[s].ncent = 1;
            }
            t.up(t.cutv.p, cutv);
            hipLaunchKernelGGL(k_train_seed_pick, dim3((unsigned)nl), dim3(kTrainThreads), 0, t.s, t.seg.p, t.cutv.p, 1,
                               0, k, t.md.p, order, t.D.p, t.cent.p, t.pick.p);
            HIPCK(hipGetLastError());
            std::vector<unsigned long long> S;
            for (int j = 1; j < k; ++j) {
                HIPCK(hipMemsetAsync(t.S.p, 0, nl * sizeof(unsigned long long), t.s));
                hipLaunchKernelGGL(k_train_seed_dist, dim3(nch_all), dim3(kTrainThreads), 0, t.s, t.chunk.p, j - 1, k,
                                   t.pick.p, order, t.D.p, t.cent.p, t.md.p, t.S.p);
                HIPCK(hipGetLastError());
                t.down(S, t.S.p, nl);
                bool any = false;
                for (size_t s = 0; s < nl; ++s) {
                    cutv[s] = 0;
                    if (!seeding[s]) continue;
                    if (S[s] == 0) {
                        seeding[s] = 0;
                        continue;
                    }
                    cutv[s] = (int64_t)(1 + draw(p.seed, lnode[s], j) % (uint64_t)S[s]);
                    lseg[s].ncent = j + 1;
                    any = true;
                }
                if (!any) break;
                t.up(t.cutv.p, cutv);
                hipLaunchKernelGGL(k_train_seed_pick, dim3((unsigned)nl), dim3(kTrainThreads), 0, t.s, t.seg.p,
                                   t.cutv.p, 0, j, k, t.md.p, order, t.D.p, t.cent.p, t.pick.p);
                HIPCK(hipGetLastError());
            }
            for (size_t s = 0; s < nl; ++s) st.short_seeded[depth] += lseg[s].ncent < k;
            t.up(t.seg.p, lseg);
            // ---- Lloyd iterations ----
            if (!slot_seg.empty()) {
                t.slot_seg.ensure(slot_seg.size());
                t.up(t.slot_seg.p, slot_seg);
                t.gcnt.ensure(slot_seg.size() * (size_t)k * kTrainThreads);
                t.gn.ensure(slot_seg.size() * (size_t)k);
                HIPCK(hipMemsetAsync(t.gcnt.p, 0, slot_seg.size() * (size_t)k * kTrainThreads * sizeof(uint32_t), t.s));
                HIPCK(hipMemsetAsync(t.gn.p, 0, slot_seg.size() * (size_t)k * sizeof(uint32_t), t.s));
            }
            HIPCK(hipMemsetAsync(t.assign.p, 0xFF, (size_t)npos, t.s));
            std::vector<int32_t> changed;
            size_t n_live = nl;
            for (int it = 1; it <= p.max_iter && n_live; ++it) {
                const unsigned nch = (unsigned)chunks.size();
                if (it > 1) {
                    hipLaunchKernelGGL(k_train_mean, dim3(nch), dim3(kTrainThreads), 0, t.s, t.chunk.p, t.seg.p, k,
                                       order, reinterpret_cast<const uint32_t*>(t.D.p), t.assign.p,
                                       reinterpret_cast<uint32_t*>(t.cent.p), t.gcnt.p, t.gn.p);
                    HIPCK(hipGetLastError());
                    if (!slot_seg.empty()) {
                        hipLaunchKernelGGL(k_train_mean_final, dim3((unsigned)slot_seg.size()), dim3(kTrainThreads), 0,
                                           t.s, t.slot_seg.p, t.seg.p, k, reinterpret_cast<uint32_t*>(t.cent.p),
                                           t.gcnt.p, t.gn.p);
                        HIPCK(hipGetLastError());
                    }
                }
                HIPCK(hipMemsetAsync(t.changed.p, 0, nl * sizeof(int32_t), t.s));
                hipLaunchKernelGGL(k_train_assign, dim3(nch), dim3(kTrainThreads), 0, t.s, t.chunk.p, t.seg.p, k, order,
                                   t.D.p, t.cent.p, t.assign.p, t.changed.p);
                HIPCK(hipGetLastError());
                t.down(changed, t.changed.p, nl);
                bool fewer = false;
                for (size_t s = 0; s < nl; ++s) {
                    if (!live[s]) continue;
                    iters[s] = it;
                    if (!changed[s]) {
                        live[s] = 0;
                        --n_live;
                        fewer = true;
                    } else if (it == p.max_iter) {
                        capped[s] = 1;
                    }
                }
                if (fewer && n_live && it < p.max_iter) build_chunks();
            }
            // ---- members per cluster ----
            std::fill(live.begin(), live.end(), 1);
            build_chunks();
            t.ccount.ensure(chunks.size() * (size_t)k);
            hipLaunchKernelGGL(k_train_count, dim3((unsigned)chunks.size()), dim3(kTrainThreads), 0, t.s, t.chunk.p, k,
                               t.assign.p, t.ccount.p);
            HIPCK(hipGetLastError());
        }
        std::vector<int32_t> ccount;
        if (nl) t.down(ccount, t.ccount.p, chunks.size() * (size_t)k);
        std::vector<int64_t> ctot(nl * (size_t)k, 0);
        for (size_t c = 0; c < chunks.size(); ++c)
            for (int x = 0; x < k; ++x) ctot[(size_t)chunks[c].seg * k + x] += ccount[c * k + x];

        // ---- the children, in node order ----
        std::vector<HostSeg> next;
        std::vector<int64_t> src;
        std::vector<int32_t> child_start(nl * (size_t)k, -1);  // where a continuing child's members go
        int64_t next_pos = 0;
        const bool deeper = depth + 1 < L;
        st.nodes_split[depth] = (int64_t)segs.size();
        for (const HostSeg& h : segs) {
            if (h.large < 0) {
                for (int32_t i = 0; i < h.len; ++i) {
                    parent.push_back(h.node);
                    src.push_back(-((int64_t)h.start + i) - 1);
                }
                continue;
            }
            const size_t s = (size_t)h.large;
            st.iter_sum[depth] += iters[s];
            st.iter_max[depth] = std::max<int64_t>(st.iter_max[depth], iters[s]);
            st.capped[depth] += capped[s];
            for (int x = 0; x < lseg[s].ncent; ++x) {
                const int64_t n = ctot[s * k + x];
                if (n == 0) {
                    ++st.empty_dropped[depth];
                    continue;
                }
                const int32_t id = (int32_t)parent.size();
                parent.push_back(h.node);
                src.push_back((int64_t)s * k + x);
                if (deeper && n > 1) {
                    child_start[s * k + x] = (int32_t)next_pos;
                    next.push_back(HostSeg{id, (int32_t)next_pos, (int32_t)n, -1});
                    next_pos += n;
                }
            }
        }
        if (parent.size() > (size_t)0x7FFFFFF0) throw Error(ORBFE_ECAPACITY, "more than 2^31 nodes");
        // child descriptors
        const size_t first_child = desc.size() / 32, nchild = src.size();
        t.src.ensure(nchild);
        t.up(t.src.p, src);
        t.out.ensure(nchild * 2);
        hipLaunchKernelGGL(k_train_emit, dim3(blocks_for((int64_t)nchild * 2)), dim3(kTrainThreads), 0, t.s, t.src.p,
                           (int64_t)nchild, order, t.D.p, t.cent.p, t.out.p);
        HIPCK(hipGetLastError());
        desc.resize((first_child + nchild) * 32);
        HIPCK(hipMemcpyAsync(&desc[first_child * 32], t.out.p, nchild * 32, hipMemcpyDeviceToHost, t.s));
        // the next depth's order
        if (!next.empty()) {
            std::vector<int32_t> cbase(chunks.size() * (size_t)k, -1);
            std::vector<int32_t> fill(child_start);
            for (size_t c = 0; c < chunks.size(); ++c)
                for (int x = 0; x < k; ++x) {
                    int32_t& f = fill[(size_t)chunks[c].seg * k + x];
                    if (f < 0) continue;
                    cbase[c * k + x] = f;
                    f += ccount[c * k + x];
                }
            t.cbase.ensure(cbase.size());
            t.up(t.cbase.p, cbase);
            hipLaunchKernelGGL(k_train_scatter, dim3((unsigned)chunks.size()), dim3(kTrainThreads), 0, t.s, t.chunk.p,
                               k, order, t.assign.p, t.cbase.p, t.order[cur ^ 1].p);
            HIPCK(hipGetLastError());
            cur ^= 1;
        }
        HIPCK(hipEventRecord(t.ev[1], t.s));
        HIPCK(hipStreamSynchronize(t.s));
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        st.depth_ms[depth] = ms;
        st.kernel_ms += ms;
        segs.swap(next);
    }

    // ---- weights ----
    const int64_t nn = (int64_t)parent.size();
    std::vector<uint8_t> leaf(nn, 1);
    for (int64_t i = 1; i < nn; ++i) leaf[parent[i]] = 0;
    leaf[0] = 0;
    int64_t nw = 0;
    for (int64_t i = 1; i < nn; ++i) nw += leaf[i];
    st.n_nodes = nn;
    st.n_words = nw;
    std::vector<double> weight(nn, 0.0);
    if (p.weighting == 1 || p.weighting == 3) {
        for (int64_t i = 1; i < nn; ++i)
            if (leaf[i]) weight[i] = 1.0;
    } else {
        orbfe_vocab_handle tree = finish(nullptr);
        struct Drop {
            orbfe_vocab_handle h;
            ~Drop() { orbfe_vocab_destroy(h); }
        } drop{tree};
        t.word.ensure(N);
        t.node.ensure(N);
        t.w.ensure(N);
        t.ni.ensure(nw);
        t.off.ensure(off.size());
        uint64_t places = 64;
        while (places < 2 * (uint64_t)N) places <<= 1;
        t.table.ensure(places);
        t.up(t.off.p, off);
        HIPCK(hipEventRecord(t.ev[0], t.s));
        HIPCK(hipMemsetAsync(t.ni.p, 0, (size_t)nw * sizeof(int32_t), t.s));
        HIPCK(hipMemsetAsync(t.table.p, 0xFF, places * sizeof(unsigned long long), t.s));
        const int rc = orbfe_vocab_transform_device(tree, reinterpret_cast<const uint8_t*>(t.D.p), N, -1, t.word.p,
                                                    t.node.p, t.w.p, t.s);
        if (rc != ORBFE_OK) throw Error(rc, g_err);
        hipLaunchKernelGGL(k_train_mark, dim3(blocks_for(N)), dim3(kTrainThreads), 0, t.s, t.word.p, N, t.off.p,
                           n_frames, t.table.p, (unsigned long long)(places - 1), t.ni.p);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(t.ev[1], t.s));
        std::vector<int32_t> ni;
        t.down(ni, t.ni.p, (size_t)nw);
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        st.weight_ms = ms;
        st.kernel_ms += ms;
        int64_t wid = 0;
        for (int64_t i = 1; i < nn; ++i)
            if (leaf[i]) {
                const int32_t c = ni[wid++];
                weight[i] = c > 0 ? std::log((double)n_frames / (double)c) : 0.0;
            }
    }
    *out = finish(&weight);
}

// the shortest decimal that reads back as the same double, written the way Python's repr writes it for the values
// a vocabulary holds ("1.0", "0.0", "2.4849066497880004", "1e-05")
std::string shortest(double x) {
    char buf[40];
    for (int prec = 1; prec <= 17; ++prec) {
        std::snprintf(buf, sizeof(buf), "%.*g", prec, x);
        if (std::strtod(buf, nullptr) == x || x != x) break;
    }
    std::string s(buf);
    if (s.find_first_of(".enai") == std::string::npos) s += ".0";
    return s;
}

}  // namespace

extern "C" {

int orbfe_vocab_train(const uint8_t* desc32, int32_t desc_on_device, const int64_t* start, const int32_t* count,
                      int32_t n_frames, const orbfe_vocab_train_params* params, orbfe_vocab_handle* out,
                      orbfe_vocab_train_stats* stats) {
    return guarded([&] {
        if (!start || !count || !params || !out) throw Error(ORBFE_EINVAL, "null argument");
        const orbfe_vocab_train_params& p = *params;
        if (p.k < 2 || p.k > kTrainMaxK) throw Error(ORBFE_EINVAL, "k must be 2 .. 20");
        if (p.L < 1 || p.L > ORBFE_VOCAB_TRAIN_MAX_L) throw Error(ORBFE_EINVAL, "L must be 1 .. 10");
        if (p.weighting < 0 || p.weighting > 3) throw Error(ORBFE_EINVAL, "weighting must be 0 .. 3");
        if (p.scoring < 0 || p.scoring > 5) throw Error(ORBFE_EINVAL, "scoring must be 0 .. 5");
        if (p.max_iter < 1) throw Error(ORBFE_EINVAL, "max_iter must be at least 1");
        if (n_frames < 1) throw Error(ORBFE_EINVAL, "n_frames must be at least 1");
        int64_t total = 0;
        for (int32_t f = 0; f < n_frames; ++f) {
            if (count[f] < 0 || start[f] < 0) throw Error(ORBFE_EINVAL, "negative start or count");
            total += count[f];
            if (total > 0x7FFFFFFFll) throw Error(ORBFE_EINVAL, "more than 2^31 - 1 descriptors");
        }
        if (total > 0 && !desc32) throw Error(ORBFE_EINVAL, "null argument");
        orbfe_vocab_train_stats st{};
        *out = nullptr;
        train(desc32, desc_on_device != 0, start, count, n_frames, p, out, st);
        if (stats) *stats = st;
    });
}

int orbfe_vocab_save_text(orbfe_vocab_handle v, const char* path) {
    return guarded([&] {
        if (!v || !path) throw Error(ORBFE_EINVAL, "null argument");
        orbfe_vocab_info info;
        int rc = orbfe_vocab_get_info(v, &info);
        if (rc != ORBFE_OK) throw Error(rc, g_err);
        const size_t n = (size_t)info.n_nodes;
        std::vector<int32_t> parent(n);
        std::vector<uint8_t> leaf(n), desc(n * 32);
        std::vector<double> weight(n);
        rc = orbfe_vocab_get_nodes(v, parent.data(), leaf.data(), desc.data(), weight.data(), nullptr);
        if (rc != ORBFE_OK) throw Error(rc, g_err);
        FILE* f = std::fopen(path, "wb");
        if (!f) throw Error(ORBFE_EINVAL, std::string("cannot write vocabulary file: ") + path);
        std::string line = std::to_string(info.k) + " " + std::to_string(info.L) + " " + std::to_string(info.scoring) +
                           " " + std::to_string(info.weighting) + "\n";
        bool ok = std::fputs(line.c_str(), f) >= 0;
        for (size_t i = 1; i < n && ok; ++i) {
            line = std::to_string(parent[i]) + " " + std::to_string((int)leaf[i]);
            for (int b = 0; b < 32; ++b) line += " " + std::to_string((int)desc[i * 32 + b]);
            line += " " + shortest(weight[i]) + "\n";
            ok = std::fputs(line.c_str(), f) >= 0;
        }
        ok = (std::fclose(f) == 0) && ok;
        if (!ok) throw Error(ORBFE_EINVAL, std::string("cannot write vocabulary file: ") + path);
    });
}

}  // extern "C"
