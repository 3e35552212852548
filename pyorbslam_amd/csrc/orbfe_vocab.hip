// orbfe_vocab.hip — bag-of-words vocabulary tree on gfx950: native text loader, device node tables and
// the batched descent kernel behind pyDBoW.TemplatedVocabulary.transform (TemplatedVocabulary.py:108-160).
//
// Layout.  The reference keeps Python Node objects with a child-id list each and, per level of a
// descent, computes a per-byte Python popcount against every child (FORB.distance, FORB.py:30-32).
// Here the children of every node occupy one contiguous run of "slots" (slot order = child order), so a
// level of a descent reads count x 32 descriptor bytes in one coalesced sweep:
//   slot_desc[s]  32 B   descriptor of the child in slot s
//   slot_info[s]  16 B   {child node id, its first slot, its child count, its word id}
//   weight[node]  f64    node weight (TemplatedVocabulary.py:67, a Python float)
// The root's run is passed by value.  Host copies of the parsed tables stay in the object (for
// orbfe_vocab_get_nodes and the CPU tests); the device copy is made on first use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host_util.h"

using namespace orbfe;

struct orbfe_vocab {
    orbfe_vocab_info info{};
    // per node (id order, entry 0 = root)
    std::vector<int32_t> parent;
    std::vector<uint8_t> leaf_flag;
    std::vector<uint8_t> desc;      // 32 B per node
    std::vector<double> weight;
    std::vector<int32_t> word;
    // per slot
    std::vector<int4> slot_info;
    int32_t root_count = 0;
    // device
    bool uploaded = false;
    DevBuf<uint4> d_slot_desc;
    DevBuf<int4> d_slot_info;
    DevBuf<double> d_weight;
    DevBuf<uint8_t> d_q;
    DevBuf<int32_t> d_word, d_node;
    DevBuf<double> d_w;
    TimedStream t;  // orbfe_vocab_transform
    // orbfe_vocab_bow: frame offsets, the i32 outputs (4 per-entry arrays, 3 per-frame arrays) and the weights
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_bow_i;
    DevBuf<double> d_bow_w;
    TimedStream t_bow;  // orbfe_vocab_bow: its events only, on t's stream
    // transform callers share one vocabulary across threads (Frame.compute_BoW on the tracking thread,
    // KeyFrame.compute_bow on the mapping thread: Frame.py:125, KeyFrame.py:119): the scratch buffers,
    // the stream and the events above are guarded by this mutex
    std::mutex mu;
    ~orbfe_vocab() {
        t_bow.destroy();
        t.destroy();
    }
};

namespace orbfe {

constexpr int kVocabPerBlock = 8;  // descriptors per 256-thread block: 32 lanes each

// One descent per 32-lane group.  Per level, lane j takes child j (j, j+32, ... when a node has more
// than 32 children), XORs its 32 descriptor bytes with the query and counts bits (v_bcnt accumulate);
// the group minimum of key = dist << 16 | child position is the reference's first strict minimum
// (TemplatedVocabulary.py:143-150).  The winner's slot_info was loaded by its own lane together with
// the descriptor, so the next level needs no dependent table read: one memory round trip per level.
__device__ __forceinline__ void descend_one(const uint8_t* __restrict__ qi, int lane, int root_count,
                                            const uint4* __restrict__ slot_desc, const int4* __restrict__ slot_info,
                                            int nid_level, int& node, int& word, int& nid) {
    const uint4* qp = reinterpret_cast<const uint4*>(qi);
    const uint4 qa = qp[0], qb = qp[1];
    int start = 0, count = root_count;
    node = 0, word = 0, nid = -1;
    for (int level = 1; count > 0; ++level) {
        unsigned best = 0xFFFFFFFFu;
        int4 mine = make_int4(0, 0, 0, 0);
        for (int c0 = 0; c0 < count; c0 += 32) {
            const int j = c0 + lane;
            if (j < count) {
                const uint4 a = slot_desc[2 * (start + j)];
                const uint4 b = slot_desc[2 * (start + j) + 1];
                const int4 inf = slot_info[start + j];
                const unsigned d = hamming256(a, b, qa, qb);
                const unsigned key = (d << 16) | (unsigned)j;
                if (key < best) {
                    best = key;
                    mine = inf;
                }
            }
        }
#pragma unroll
        for (int o = 16; o; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 32));
        const int wl = (int)(best & 31u);
        node = __shfl(mine.x, wl, 32);
        start = __shfl(mine.y, wl, 32);
        count = __shfl(mine.z, wl, 32);
        word = __shfl(mine.w, wl, 32);
        if (level == nid_level) nid = node;
    }
}

__global__ __launch_bounds__(256) void k_vocab_descend(const uint8_t* __restrict__ q, int64_t n, int root_count,
                                                       const uint4* __restrict__ slot_desc,
                                                       const int4* __restrict__ slot_info,
                                                       const double* __restrict__ weight, int nid_level,
                                                       int32_t* __restrict__ out_word, int32_t* __restrict__ out_node,
                                                       double* __restrict__ out_w) {
    const int lane = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * kVocabPerBlock + (threadIdx.x >> 5);
    if (i >= n) return;  // the whole 32-lane group leaves together
    int node, word, nid;
    descend_one(q + i * 32, lane, root_count, slot_desc, slot_info, nid_level, node, word, nid);
    if (lane == 0) {
        out_word[i] = word;
        out_node[i] = nid;
        out_w[i] = weight[node];
    }
}

// ---- BoW / feature vector assembly (TemplatedVocabulary.py:108-129, BowVector.py:8-28, FeatureVector.py:8-19) ----

// How a launch finds its frames.  Ragged (off != nullptr, the host entry): frame f is descents
// [off[f], off[f + 1]) and its outputs are packed at off[f].  Strided (the device entry): frame f is
// count[f * count_stride] descriptors from descriptor f * frame_stride, its outputs start at f * out_stride.
struct BowFrames {
    const int64_t* off;
    const int32_t* count;
    int64_t frame_stride, count_stride, out_stride;
};

// The length a strided frame is processed with, and which bounds its count broke (ORBFE_BOW_* flags).
__device__ __forceinline__ int bow_frame_count(const BowFrames& fr, int f, int& flags) {
    int64_t c = fr.count[(int64_t)f * fr.count_stride];
    flags = 0;
    if (c < 0) flags |= ORBFE_BOW_NEGATIVE, c = 0;
    if (c > fr.out_stride) flags |= ORBFE_BOW_OVER_OUT, c = fr.out_stride;
    if (c > ORBFE_BOW_MAX_FRAME) flags |= ORBFE_BOW_OVER_MAX, c = ORBFE_BOW_MAX_FRAME;
    if (c > fr.frame_stride) flags |= ORBFE_BOW_OVER_FRAME, c = fr.frame_stride;
    return (int)c;
}

// k_vocab_descend over strided frames with device-side counts: block (f, y) takes descriptors 8y .. 8y + 7 of
// frame f and leaves past the frame's count, so nothing behind a count is read.
__global__ __launch_bounds__(256) void k_vocab_descend_frames(const uint8_t* __restrict__ q, BowFrames fr,
                                                              int root_count, const uint4* __restrict__ slot_desc,
                                                              const int4* __restrict__ slot_info,
                                                              const double* __restrict__ weight, int nid_level,
                                                              int32_t* __restrict__ out_word,
                                                              int32_t* __restrict__ out_node,
                                                              double* __restrict__ out_w) {
    const int lane = threadIdx.x & 31;
    const int f = blockIdx.x;
    const int i = blockIdx.y * kVocabPerBlock + (threadIdx.x >> 5);
    int flags;
    if (i >= bow_frame_count(fr, f, flags)) return;
    const int64_t at = (int64_t)f * fr.frame_stride + i;
    int node, word, nid;
    descend_one(q + at * 32, lane, root_count, slot_desc, slot_info, nid_level, node, word, nid);
    if (lane == 0) {
        out_word[at] = word;
        out_node[at] = nid;
        out_w[at] = weight[node];
    }
}

constexpr int kBowItems = 8;  // positions per lane: a frame of up to CAP features takes a block of CAP / 8 threads

__device__ __forceinline__ unsigned key_hi(unsigned long long k) { return (unsigned)(k >> 32); }
__device__ __forceinline__ int key_lo(unsigned long long k) { return (int)(unsigned)k; }

// Appends the keys of the lanes with `keep` to key[] (order among them is arbitrary: the keys are unique and
// get sorted).  One LDS atomic per wave; every lane of the wave must call it.
__device__ __forceinline__ void bow_append(unsigned long long* key, int* cnt, bool keep, unsigned long long k,
                                           int lane) {
    const unsigned long long mask = __ballot(keep);
    int base = 0;
    if (lane == 0 && mask) base = atomicAdd(cnt, __popcll(mask));
    base = __shfl(base, 0, 64);
    if (keep) key[base + __popcll(mask & ((1ull << lane) - 1ull))] = k;
}

// Bitonic sort of key[0 .. nk) in LDS, ascending, padded to the next power of two P >= 2 with all-ones keys
// (a real key's top bit is clear).  Of the log2(P) (log2(P) + 1) / 2 compare-exchange steps, those at a distance
// of 64 or more go through LDS with a barrier each; the steps at distances 32 .. 1 that end a stage stay inside
// one wave, so the lane holding elements tid, tid + T, .. in registers does them with lane exchanges, one LDS round
// trip and one barrier per stage (and one for all the stages up to 64 together).
template <int T>
__device__ void bow_sort(unsigned long long* key, int nk, int tid) {
    int P = 2;
    while (P < nk) P <<= 1;
    for (int i = nk + tid; i < P; i += T) key[i] = ~0ull;
    __syncthreads();
    unsigned long long r[kBowItems];
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 64; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const unsigned long long a = key[i], b = key[p];
                if ((a > b) == ((i & k) == 0)) {
                    key[i] = b;
                    key[p] = a;
                }
            }
            __syncthreads();
        }
        if (k < 64 && k < P) continue;  // the stages below 64 run together with stage 64 (or with the last one)
#pragma unroll
        for (int it = 0; it < kBowItems; ++it) r[it] = it * T + tid < P ? key[it * T + tid] : ~0ull;
        for (int kk = k <= 64 ? 2 : k; kk <= k; kk <<= 1)
            for (int j = min(kk >> 1, 32); j > 0; j >>= 1) {
#pragma unroll
                for (int it = 0; it < kBowItems; ++it) {
                    const int i = it * T + tid;
                    const unsigned long long a = r[it], b = __shfl_xor(a, j, 64);
                    const bool low = ((i & j) == 0) == ((i & kk) == 0);  // this side keeps the smaller key
                    r[it] = (low == (a < b)) ? a : b;
                }
            }
#pragma unroll
        for (int it = 0; it < kBowItems; ++it)
            if (it * T + tid < P) key[it * T + tid] = r[it];
        __syncthreads();
    }
}

// Run heads of the sorted keys (a position whose high word differs from its predecessor's).  Lane tid owns
// positions 8 tid .. 8 tid + 7: bit `it` of headmask marks a head at 8 tid + it.  Returns the rank of the lane's
// first head among all heads, and their number in total.
template <int T>
__device__ int bow_heads(const unsigned long long* key, int nk, int tid, int* wtot, unsigned& headmask, int& total) {
    const int lane = tid & 63, wave = tid >> 6, p0 = tid * kBowItems;
    headmask = 0;
    unsigned prev = (p0 > 0 && p0 < nk) ? key_hi(key[p0 - 1]) : 0u;
#pragma unroll
    for (int it = 0; it < kBowItems; ++it) {
        const int p = p0 + it;
        if (p < nk) {
            const unsigned h = key_hi(key[p]);
            if (p == 0 || h != prev) headmask |= 1u << it;
            prev = h;
        }
    }
    const int c = __popc(headmask);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < T / 64; ++w) {
        const int x = wtot[w];
        if (w < wave) base += x;
        total += x;
    }
    __syncthreads();  // wtot is free again
    return base + incl - c;
}

// One workgroup per frame, the frame's keys in LDS.  Kept features (weight > 0) are sorted by (word, index), each
// run of one word is summed by the lane at its head in ascending feature index, one lane adds the raw weights in
// ascending word id, all lanes divide; then the kept features are sorted by (threaded node, index) and the runs
// become the CSR feature vector.  Every f64 sum is the reference's plain left-to-right sum.
template <int CAP>
__global__ __launch_bounds__(CAP / kBowItems) void k_bow_assemble(BowFrames fr, const int32_t* __restrict__ d_word,
                                                                  const int32_t* __restrict__ d_node,
                                                                  const double* __restrict__ d_w, orbfe_bow_out out) {
    constexpr int T = CAP / kBowItems;
    __shared__ unsigned long long key[CAP];
    __shared__ double wl[CAP];
    __shared__ int wtot[T / 64];
    __shared__ int s_cnt;
    __shared__ double s_total;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p0 = tid * kBowItems;
    int flags = 0, n;
    int64_t in0, out0;
    if (fr.off) {
        in0 = out0 = fr.off[f];
        n = (int)(fr.off[f + 1] - in0);
    } else {
        n = bow_frame_count(fr, f, flags);
        in0 = (int64_t)f * fr.frame_stride;
        out0 = (int64_t)f * fr.out_stride;
    }
    if (n > CAP) n = CAP;  // the launcher picks CAP above every length it admits
    if (tid == 0 && flags) atomicOr(out.status, flags);
    if (n <= 0) {  // the whole block leaves together
        if (tid == 0) out.n_words[f] = out.n_nodes[f] = out.n_kept[f] = 0;
        return;
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();

    // keep mask and (word, index) keys
#pragma unroll
    for (int it = 0; it < kBowItems; ++it) {
        const int i = it * T + tid;
        double w = 0.0;
        int word = 0;
        if (i < n) {
            w = d_w[in0 + i];
            word = d_word[in0 + i];
            wl[i] = w;
        }
        bow_append(key, &s_cnt, w > 0.0, ((unsigned long long)(unsigned)word << 32) | (unsigned)i, lane);
    }
    __syncthreads();
    const int nk = s_cnt;
    bow_sort<T>(key, nk, tid);

    unsigned heads;
    int n_words;
    int rank0 = bow_heads<T>(key, nk, tid, wtot, heads, n_words);
    double raw[kBowItems];
#pragma unroll
    for (int it = 0; it < kBowItems; ++it) {
        raw[it] = 0.0;
        if (heads >> it & 1u) {
            const int p = p0 + it;
            const unsigned long long k0 = key[p];
            double s = wl[key_lo(k0)];
            for (int q = p + 1; q < nk; ++q) {  // a run may be as long as the frame
                const unsigned long long k1 = key[q];
                if (key_hi(k1) != key_hi(k0)) break;
                s = s + wl[key_lo(k1)];
            }
            raw[it] = s;
            out.bow_word[out0 + rank0 + __popc(heads & ((1u << it) - 1u))] = (int32_t)key_hi(k0);
        }
    }
    __syncthreads();  // every walk has read its keys: the raw weights take their place
    double* rawl = reinterpret_cast<double*>(key);
#pragma unroll
    for (int it = 0; it < kBowItems; ++it)
        if (heads >> it & 1u) rawl[rank0 + __popc(heads & ((1u << it) - 1u))] = raw[it];
    __syncthreads();
    if (tid == 0) {  // the reference's sum(): a serial chain of n_words dependent adds
        double t = 0.0;
        int i = 0;
        for (; i + 16 <= n_words; i += 16) {  // 16 LDS reads in flight, then their adds in order
            double x[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = rawl[i + j];
#pragma unroll
            for (int j = 0; j < 16; ++j) t = t + x[j];
        }
        for (; i < n_words; ++i) t = t + rawl[i];
        s_total = t;
        s_cnt = 0;
        out.n_words[f] = n_words;
        out.n_kept[f] = nk;
    }
    __syncthreads();
    const double total = s_total;
    for (int i = tid; i < n_words; i += T) {
        const double x = rawl[i];
        out.bow_weight[out0 + i] = total > 0.0 ? x / total : x;
    }

    // node threading: a feature whose descent stopped above the node level takes the last valid node before it
    // in the frame (0 when there is none), dropped features included
    int nd[kBowItems], last = -1;
#pragma unroll
    for (int it = 0; it < kBowItems; ++it) {
        const int i = p0 + it;
        nd[it] = i < n ? d_node[in0 + i] : -1;
        if (nd[it] >= 0) last = nd[it];
    }
    int incl = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o && incl < 0) incl = v;
    }
    int cur = __shfl_up(incl, 1, 64);
    if (lane == 0) cur = -1;
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();  // also: rawl has been read, key[] is free
    for (int w = wave - 1; w >= 0 && cur < 0; --w) cur = wtot[w];
    if (cur < 0) cur = 0;
#pragma unroll
    for (int it = 0; it < kBowItems; ++it) {
        const int i = p0 + it;
        if (nd[it] >= 0) cur = nd[it];
        bow_append(key, &s_cnt, i < n && wl[i] > 0.0, ((unsigned long long)(unsigned)cur << 32) | (unsigned)i, lane);
    }
    __syncthreads();
    bow_sort<T>(key, nk, tid);

    int n_nodes;
    rank0 = bow_heads<T>(key, nk, tid, wtot, heads, n_nodes);
#pragma unroll
    for (int it = 0; it < kBowItems; ++it) {
        const int p = p0 + it;
        if (p < nk) {
            const unsigned long long k0 = key[p];
            out.fv_idx[out0 + p] = key_lo(k0);
            if (heads >> it & 1u) {
                const int r = rank0 + __popc(heads & ((1u << it) - 1u));
                out.fv_node[out0 + r] = (int32_t)key_hi(k0);
                if (r > 0) out.fv_end[out0 + r - 1] = p;
            }
        }
    }
    if (tid == 0) {
        out.n_nodes[f] = n_nodes;
        if (n_nodes > 0) out.fv_end[out0 + n_nodes - 1] = nk;
    }
}

}  // namespace orbfe

namespace {

// Build children runs, word ids, depth from the per-node arrays (validated).
void finish(orbfe_vocab& v) {
    const int64_t n = (int64_t)v.parent.size();
    std::vector<int32_t> nch(n, 0);
    for (int64_t i = 1; i < n; ++i) nch[v.parent[i]]++;
    std::vector<int32_t> first(n, 0);
    int64_t s = 0;
    for (int64_t i = 0; i < n; ++i) {
        first[i] = (int32_t)s;
        s += nch[i];
    }
    v.word.assign(n, 0);
    int64_t nw = 0;
    for (int64_t i = 1; i < n; ++i)
        if (v.leaf_flag[i]) v.word[i] = (int32_t)nw++;
    std::vector<int32_t> fill(n, 0), depth(n, 0);
    v.slot_info.assign(std::max<int64_t>(n - 1, 0), make_int4(0, 0, 0, 0));
    int maxd = 0;
    for (int64_t i = 1; i < n; ++i) {
        const int32_t p = v.parent[i];
        v.slot_info[first[p] + fill[p]++] = make_int4((int)i, first[i], nch[i], v.word[i]);
        depth[i] = depth[p] + 1;
        maxd = std::max(maxd, depth[i]);
    }
    v.root_count = n > 0 ? nch[0] : 0;
    v.info.n_nodes = n;
    v.info.n_words = nw;
    v.info.depth = maxd;
    v.info.max_children = n > 0 ? *std::max_element(nch.begin(), nch.end()) : 0;
    if (v.info.max_children > 65535) throw Error(ORBFE_EINVAL, "more than 65535 children under one node");
}

void upload(orbfe_vocab& v) {
    if (v.uploaded) return;
    v.t.get();
    const size_t ns = v.slot_info.size();
    std::vector<uint8_t> sd(std::max<size_t>(ns, 1) * 32, 0);
    for (size_t s = 0; s < ns; ++s) std::memcpy(&sd[s * 32], &v.desc[(size_t)v.slot_info[s].x * 32], 32);
    v.d_slot_desc.ensure(std::max<size_t>(ns, 1) * 2);
    v.d_slot_info.ensure(std::max<size_t>(ns, 1));
    v.d_weight.ensure(v.weight.size());
    HIPCK(hipMemcpy(v.d_slot_desc.p, sd.data(), sd.size(), hipMemcpyHostToDevice));
    if (ns) HIPCK(hipMemcpy(v.d_slot_info.p, v.slot_info.data(), ns * sizeof(int4), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(v.d_weight.p, v.weight.data(), v.weight.size() * sizeof(double), hipMemcpyHostToDevice));
    v.uploaded = true;
}

void launch_descend(orbfe_vocab& v, const uint8_t* d_q, int64_t n, int nid_level, int32_t* d_word, int32_t* d_node,
                    double* d_w, hipStream_t s) {
    if (n <= 0) return;
    const int64_t blocks = (n + kVocabPerBlock - 1) / kVocabPerBlock;
    if (blocks > 0x7FFFFFFF) throw Error(ORBFE_EINVAL, "too many descriptors for one launch");
    hipLaunchKernelGGL(k_vocab_descend, dim3((unsigned)blocks), dim3(256), 0, s, d_q, n, v.root_count,
                       v.d_slot_desc.p, v.d_slot_info.p, v.d_weight.p, nid_level, d_word, d_node, d_w);
    HIPCK(hipGetLastError());
}

// Frames of at most 2 048 features take the 256-thread kernel (32 KiB of LDS, several frames per CU), longer ones
// the 1 024-thread kernel (128 KiB).  `longest` bounds every frame of the launch.
constexpr int kBowSmall = 2048;

void launch_assemble(const BowFrames& fr, int n_frames, int64_t longest, const int32_t* d_word, const int32_t* d_node,
                     const double* d_w, const orbfe_bow_out& out, hipStream_t s) {
    if (longest <= kBowSmall)
        hipLaunchKernelGGL(k_bow_assemble<kBowSmall>, dim3((unsigned)n_frames), dim3(kBowSmall / kBowItems), 0, s, fr,
                           d_word, d_node, d_w, out);
    else
        hipLaunchKernelGGL(k_bow_assemble<ORBFE_BOW_MAX_FRAME>, dim3((unsigned)n_frames),
                           dim3(ORBFE_BOW_MAX_FRAME / kBowItems), 0, s, fr, d_word, d_node, d_w, out);
    HIPCK(hipGetLastError());
}

// descents of a launch's n entries in one scratch block: weights, then words, then nodes
struct BowScratch {
    double* w;
    int32_t *word, *node;
    BowScratch(void* p, int64_t n)
        : w(static_cast<double*>(p)), word(reinterpret_cast<int32_t*>(w + n)), node(word + n) {}
};

// ---- text loader (TemplatedVocabulary.load_from_text_file, TemplatedVocabulary.py:43-81) ----------

// Python int(token): optional sign, decimal digits only.
bool parse_int(const char* b, const char* e, long long& out) {
    if (b == e) return false;
    const char* p = b;
    bool neg = false;
    if (*p == '+' || *p == '-') neg = *p++ == '-';
    if (p == e) return false;
    long long v = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (*p - '0');
        if (v > (1LL << 40)) return false;
    }
    out = neg ? -v : v;
    return true;
}

// Python float(token) via strtod on a NUL-terminated copy (tokens are short).
bool parse_float(const char* b, const char* e, double& out) {
    char buf[64];
    const size_t len = (size_t)(e - b);
    if (len == 0 || len >= sizeof(buf)) return false;
    std::memcpy(buf, b, len);
    buf[len] = 0;
    char* end = nullptr;
    errno = 0;
    out = std::strtod(buf, &end);
    return end == buf + len;
}

struct Tokens {
    const char* b[40];
    const char* e[40];
    int n = 0;
};

// str.strip().split() of one line, at most 40 tokens (more -> n = 41 marks "too many")
void split(const char* p, const char* end, Tokens& t) {
    t.n = 0;
    while (p < end) {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\v' || *p == '\f')) ++p;
        if (p >= end) break;
        const char* s = p;
        while (p < end && !(*p == ' ' || *p == '\t' || *p == '\r' || *p == '\v' || *p == '\f')) ++p;
        if (t.n == 40) {
            t.n = 41;
            return;
        }
        t.b[t.n] = s;
        t.e[t.n] = p;
        ++t.n;
    }
}

std::unique_ptr<orbfe_vocab> load_text(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw Error(ORBFE_EINVAL, std::string("cannot open vocabulary file: ") + path);
    std::string text;
    {
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, r);
        std::fclose(f);
    }
    const char* p = text.data();
    const char* end = p + text.size();
    auto next_line = [&](const char*& b, const char*& e) -> bool {
        if (p >= end) return false;
        b = p;
        const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
        e = nl ? nl : end;
        p = nl ? nl + 1 : end;
        return true;
    };
    auto v = std::make_unique<orbfe_vocab>();
    const char *lb, *le;
    Tokens t;
    if (!next_line(lb, le)) throw Error(ORBFE_EFORMAT, "empty vocabulary file");
    split(lb, le, t);
    long long hv[4];
    if (t.n < 4) throw Error(ORBFE_EFORMAT, "vocabulary header needs 4 integers");
    for (int k = 0; k < 4; ++k)
        if (!parse_int(t.b[k], t.e[k], hv[k])) throw Error(ORBFE_EFORMAT, "vocabulary header is not integer");
    v->info.k = (int32_t)hv[0];
    v->info.L = (int32_t)hv[1];
    v->info.scoring = (int32_t)hv[2];
    v->info.weighting = (int32_t)hv[3];
    if (hv[0] < 0 || hv[0] > 20 || hv[1] < 1 || hv[1] > 10 || hv[2] < 0 || hv[2] > 5 || hv[3] < 0 || hv[3] > 3)
        throw Error(ORBFE_EREJECT, "Vocabulary loading failure: Invalid parameters in file!");
    v->parent.push_back(0);
    v->leaf_flag.push_back(0);
    v->desc.resize(32, 0);
    v->weight.push_back(0.0);
    int64_t line_no = 1;
    while (next_line(lb, le)) {
        ++line_no;
        split(lb, le, t);
        if (t.n != 35)
            throw Error(ORBFE_EFORMAT, "vocabulary line " + std::to_string(line_no) + ": expected 35 fields");
        long long par, leaf;
        if (!parse_int(t.b[0], t.e[0], par) || !parse_int(t.b[1], t.e[1], leaf))
            throw Error(ORBFE_EFORMAT, "vocabulary line " + std::to_string(line_no) + ": bad parent / leaf flag");
        const int64_t id = (int64_t)v->parent.size();
        if (par < 0 || par >= id)
            throw Error(ORBFE_EFORMAT, "vocabulary line " + std::to_string(line_no) + ": parent is not an earlier node");
        uint8_t d[32];
        for (int k = 0; k < 32; ++k) {
            double x;
            if (!parse_float(t.b[2 + k], t.e[2 + k], x) || !(x > -1.0 && x < 256.0))
                throw Error(ORBFE_EFORMAT, "vocabulary line " + std::to_string(line_no) + ": descriptor byte");
            d[k] = (uint8_t)(int)x;  // numpy astype(int): truncation
        }
        double w;
        if (!parse_float(t.b[34], t.e[34], w))
            throw Error(ORBFE_EFORMAT, "vocabulary line " + std::to_string(line_no) + ": weight");
        v->parent.push_back((int32_t)par);
        v->leaf_flag.push_back(leaf > 0 ? 1 : 0);
        v->desc.insert(v->desc.end(), d, d + 32);
        v->weight.push_back(w);
    }
    finish(*v);
    return v;
}

}  // namespace

extern "C" {

int orbfe_vocab_load_text(const char* path, orbfe_vocab_handle* out) {
    return guarded([&] {
        if (!path || !out) throw Error(ORBFE_EINVAL, "null argument");
        *out = load_text(path).release();
    });
}

int orbfe_vocab_create(int32_t k, int32_t L, int32_t scoring, int32_t weighting, int64_t n_nodes,
                       const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc32, const double* weight,
                       orbfe_vocab_handle* out) {
    return guarded([&] {
        if (!out || n_nodes < 1 || (n_nodes > 1 && (!parent || !is_leaf || !desc32 || !weight)))
            throw Error(ORBFE_EINVAL, "bad argument");
        auto v = std::make_unique<orbfe_vocab>();
        v->info.k = k;
        v->info.L = L;
        v->info.scoring = scoring;
        v->info.weighting = weighting;
        v->parent.assign(n_nodes, 0);
        v->leaf_flag.assign(n_nodes, 0);
        v->desc.assign((size_t)n_nodes * 32, 0);
        v->weight.assign(n_nodes, 0.0);
        for (int64_t i = 1; i < n_nodes; ++i) {
            if (parent[i] < 0 || parent[i] >= i) throw Error(ORBFE_EINVAL, "parent must be an earlier node");
            v->parent[i] = parent[i];
            v->leaf_flag[i] = is_leaf[i] ? 1 : 0;
            std::memcpy(&v->desc[(size_t)i * 32], desc32 + (size_t)i * 32, 32);
            v->weight[i] = weight[i];
        }
        finish(*v);
        *out = v.release();
    });
}

int orbfe_vocab_destroy(orbfe_vocab_handle v) {
    return guarded([&] { delete v; });
}

int orbfe_vocab_get_info(orbfe_vocab_handle v, orbfe_vocab_info* info) {
    return guarded([&] {
        if (!v || !info) throw Error(ORBFE_EINVAL, "null argument");
        *info = v->info;
    });
}

int orbfe_vocab_get_nodes(orbfe_vocab_handle v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc32, double* weight,
                          int32_t* word_id) {
    return guarded([&] {
        if (!v) throw Error(ORBFE_EINVAL, "null argument");
        const size_t n = v->parent.size();
        if (parent) std::memcpy(parent, v->parent.data(), n * sizeof(int32_t));
        if (is_leaf) std::memcpy(is_leaf, v->leaf_flag.data(), n);
        if (desc32) std::memcpy(desc32, v->desc.data(), n * 32);
        if (weight) std::memcpy(weight, v->weight.data(), n * sizeof(double));
        if (word_id) std::memcpy(word_id, v->word.data(), n * sizeof(int32_t));
    });
}

int orbfe_vocab_transform(orbfe_vocab_handle v, const uint8_t* desc32, int64_t n, int32_t nid_level, int32_t* word_id,
                          int32_t* node_id, double* weight) {
    return guarded([&] {
        if (!v || n < 0 || (n > 0 && (!desc32 || !word_id || !node_id || !weight)))
            throw Error(ORBFE_EINVAL, "bad argument");
        if (n == 0) return;
        std::lock_guard<std::mutex> lk(v->mu);
        upload(*v);
        v->d_q.ensure((size_t)n * 32);
        v->d_word.ensure(n);
        v->d_node.ensure(n);
        v->d_w.ensure(n);
        HIPCK(hipMemcpyAsync(v->d_q.p, desc32, (size_t)n * 32, hipMemcpyHostToDevice, v->t.stream));
        v->t.begin(v->t.stream);
        launch_descend(*v, v->d_q.p, n, nid_level, v->d_word.p, v->d_node.p, v->d_w.p, v->t.stream);
        v->t.end(v->t.stream);
        HIPCK(hipMemcpyAsync(word_id, v->d_word.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, v->t.stream));
        HIPCK(hipMemcpyAsync(node_id, v->d_node.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, v->t.stream));
        HIPCK(hipMemcpyAsync(weight, v->d_w.p, n * sizeof(double), hipMemcpyDeviceToHost, v->t.stream));
        HIPCK(hipStreamSynchronize(v->t.stream));
        v->t.last_ms = v->t.elapsed_ms();
    });
}

int orbfe_vocab_transform_device(orbfe_vocab_handle v, const uint8_t* d_desc32, int64_t n, int32_t nid_level,
                                 int32_t* d_word_id, int32_t* d_node_id, double* d_weight, void* hip_stream) {
    return guarded([&] {
        if (!v || n < 0 || (n > 0 && (!d_desc32 || !d_word_id || !d_node_id || !d_weight)))
            throw Error(ORBFE_EINVAL, "bad argument");
        if (reinterpret_cast<uintptr_t>(d_desc32) & 15) throw Error(ORBFE_EINVAL, "descriptors must be 16-byte aligned");
        std::lock_guard<std::mutex> lk(v->mu);
        upload(*v);
        launch_descend(*v, d_desc32, n, nid_level, d_word_id, d_node_id, d_weight,
                       static_cast<hipStream_t>(hip_stream));
    });
}

int orbfe_vocab_bow_scratch_bytes(int32_t n_frames, int64_t frame_stride, int64_t* bytes) {
    return guarded([&] {
        if (!bytes || n_frames < 0 || frame_stride < 0 ||
            (frame_stride > 0 && n_frames > (INT64_MAX / 16) / frame_stride))
            throw Error(ORBFE_EINVAL, "bad argument");
        *bytes = (int64_t)n_frames * frame_stride * 16;
    });
}

int orbfe_vocab_bow_device(orbfe_vocab_handle v, const uint8_t* d_desc32, int64_t frame_stride,
                           const int32_t* d_count, int64_t count_stride, int32_t n_frames, int32_t nid_level,
                           int64_t out_stride, const orbfe_bow_out* d_out, void* d_scratch, int64_t scratch_bytes,
                           void* hip_stream) {
    return guarded([&] {
        if (!v || n_frames < 0 || frame_stride < 0 || count_stride < 1 || out_stride < 0)
            throw Error(ORBFE_EINVAL, "bad argument");
        if (n_frames == 0) return;
        if (!d_desc32 || !d_count || !d_out || !d_scratch || !d_out->n_words || !d_out->bow_word ||
            !d_out->bow_weight || !d_out->n_nodes || !d_out->fv_node || !d_out->fv_end || !d_out->fv_idx ||
            !d_out->n_kept || !d_out->status)
            throw Error(ORBFE_EINVAL, "null argument");
        if (reinterpret_cast<uintptr_t>(d_desc32) & 15) throw Error(ORBFE_EINVAL, "descriptors must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(d_scratch) & 7) throw Error(ORBFE_EINVAL, "scratch must be 8-byte aligned");
        if (frame_stride > 0 && n_frames > (INT64_MAX / 32) / frame_stride)
            throw Error(ORBFE_EINVAL, "too many descriptors for one launch");
        const int64_t entries = (int64_t)n_frames * frame_stride;
        if (scratch_bytes < entries * 16)
            throw Error(ORBFE_EINVAL, "scratch is smaller than orbfe_vocab_bow_scratch_bytes");
        std::lock_guard<std::mutex> lk(v->mu);
        upload(*v);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        const BowFrames fr{nullptr, d_count, frame_stride, count_stride, out_stride};
        const BowScratch sc(d_scratch, entries);
        const int64_t longest = std::min<int64_t>({frame_stride, out_stride, (int64_t)ORBFE_BOW_MAX_FRAME});
        if (longest > 0) {
            const unsigned chunks = (unsigned)((longest + kVocabPerBlock - 1) / kVocabPerBlock);
            hipLaunchKernelGGL(k_vocab_descend_frames, dim3((unsigned)n_frames, chunks), dim3(256), 0, s, d_desc32, fr,
                               v->root_count, v->d_slot_desc.p, v->d_slot_info.p, v->d_weight.p, nid_level, sc.word,
                               sc.node, sc.w);
            HIPCK(hipGetLastError());
        }
        launch_assemble(fr, n_frames, longest, sc.word, sc.node, sc.w, *d_out, s);
    });
}

int orbfe_vocab_bow(orbfe_vocab_handle v, const uint8_t* desc32, const int64_t* off, int32_t n_frames,
                    int32_t nid_level, const orbfe_bow_out* out) {
    return guarded([&] {
        if (!v || n_frames < 0) throw Error(ORBFE_EINVAL, "bad argument");
        if (n_frames == 0) return;
        if (!off || !out || !out->n_words || !out->n_nodes || !out->n_kept) throw Error(ORBFE_EINVAL, "null argument");
        if (off[0] != 0) throw Error(ORBFE_EINVAL, "off[0] must be 0");
        int64_t longest = 0;
        for (int32_t f = 0; f < n_frames; ++f) {
            const int64_t len = off[f + 1] - off[f];
            if (len < 0) throw Error(ORBFE_EINVAL, "off must not decrease");
            if (len > ORBFE_BOW_MAX_FRAME)
                throw Error(ORBFE_EINVAL, "frame " + std::to_string(f) + " has " + std::to_string(len) +
                                              " descriptors, more than the limit of " +
                                              std::to_string(ORBFE_BOW_MAX_FRAME) + " per frame");
            longest = std::max(longest, len);
        }
        const int64_t n = off[n_frames];
        if (out->status) *out->status = 0;
        if (n == 0) {
            for (int32_t f = 0; f < n_frames; ++f) out->n_words[f] = out->n_nodes[f] = out->n_kept[f] = 0;
            return;
        }
        if (!desc32 || !out->bow_word || !out->bow_weight || !out->fv_node || !out->fv_end || !out->fv_idx)
            throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(v->mu);
        upload(*v);
        v->d_q.ensure((size_t)n * 32);
        v->d_word.ensure(n);
        v->d_node.ensure(n);
        v->d_w.ensure(n);
        v->d_off.ensure((size_t)n_frames + 1);
        v->d_bow_i.ensure((size_t)n * 4 + (size_t)n_frames * 3);
        v->d_bow_w.ensure(n);
        orbfe_bow_out d{};
        d.bow_word = v->d_bow_i.p;
        d.fv_node = d.bow_word + n;
        d.fv_end = d.fv_node + n;
        d.fv_idx = d.fv_end + n;
        d.n_words = d.fv_idx + n;
        d.n_nodes = d.n_words + n_frames;
        d.n_kept = d.n_nodes + n_frames;
        d.bow_weight = v->d_bow_w.p;
        hipStream_t s = v->t.stream;
        HIPCK(hipMemcpyAsync(v->d_q.p, desc32, (size_t)n * 32, hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(v->d_off.p, off, ((size_t)n_frames + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        v->t_bow.begin(s);
        launch_descend(*v, v->d_q.p, n, nid_level, v->d_word.p, v->d_node.p, v->d_w.p, s);
        launch_assemble(BowFrames{v->d_off.p, nullptr, 0, 0, 0}, n_frames, longest, v->d_word.p, v->d_node.p, v->d_w.p,
                        d, s);
        v->t_bow.end(s);
        const size_t ni = (size_t)n * sizeof(int32_t), nf = (size_t)n_frames * sizeof(int32_t);
        HIPCK(hipMemcpyAsync(out->bow_word, d.bow_word, ni, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->bow_weight, d.bow_weight, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->fv_node, d.fv_node, ni, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->fv_end, d.fv_end, ni, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->fv_idx, d.fv_idx, ni, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->n_words, d.n_words, nf, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->n_nodes, d.n_nodes, nf, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->n_kept, d.n_kept, nf, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        v->t_bow.last_ms = v->t_bow.elapsed_ms();
    });
}

int orbfe_vocab_bow_last_ms(orbfe_vocab_handle v, float* ms) {
    return guarded([&] {
        if (!v || !ms) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(v->mu);
        *ms = v->t_bow.last_ms;
    });
}

int orbfe_vocab_last_ms(orbfe_vocab_handle v, float* ms) {
    return guarded([&] {
        if (!v || !ms) throw Error(ORBFE_EINVAL, "null argument");
        std::lock_guard<std::mutex> lk(v->mu);
        *ms = v->t.last_ms;
    });
}

}  // extern "C"
