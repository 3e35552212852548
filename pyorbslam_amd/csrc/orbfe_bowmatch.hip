// orbfe_bowmatch.hip — the BoW-guided descriptor match of ORBMatcher.search_by_BoW_kf_f / _kf_kf
// (ORBMatcher.py:21-213) for many frame pairs in one launch on gfx950.
//
// The reference walks the two frames' DBoW2 feature vectors (node id -> feature indices) in step and, inside
// every node both hold, gives each eligible feature of frame 1 (in run order) its best eligible, not yet
// matched feature of frame 2 by Hamming distance, subject to a distance threshold and a best / second-best
// ratio; a matched feature of frame 2 is blocked for the later features of frame 1.  Runs are disjoint, so
// the only order dependence is inside one node's run: nodes and pairs are independent.
//
// k_bow_match: one workgroup per pair, one wave per common node at a time (waves take frame 1's nodes from
// a counter in LDS, runs being of uneven length, and find each in frame 2's ascending list by binary search).
// Inside a node the wave walks frame 1's run sequentially with that feature's descriptor wave-uniform (the run
// is staged 64 features at a time, one per lane, and read back lane by lane, so the walk waits for no global
// load), while the 64 lanes hold 64 features of frame 2's run (the first 64 stay in registers for the whole
// node, 8 dwords each; longer runs re-read the further chunks per feature of frame 1).  A lane's key is
// dist << 16 | position in the run, 256 << 16 | position when it holds no candidate; one butterfly keeps the
// two smallest keys of the wave, which are best (first in run order on ties, keys being distinct) and the
// second smallest distance of the multiset; a running
// pair is merged across chunks.  Blocked flags are one byte per feature of frame 2 in LDS, preset with the
// complement of side 2's eligibility, so a candidate test is one LDS read.  The rotation histogram is kept
// in LDS and written once.  Integer work throughout except the ratio product and the rotation bin, which are
// single IEEE double operations (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host_util.h"

using namespace orbfe;

namespace orbfe {

constexpr int kBmWaves = 8;  // waves per workgroup: common nodes in flight per pair

// How a launch finds its frames.  Ragged (off != nullptr, the host entry): frame f is features
// [off[f], off[f + 1]), its nodes are entries [fv_off[f], fv_off[f + 1]) of fv_node / fv_end, its fv_idx block
// starts at off[f], and eligibility / angles are indexed by off[f] + i.  Strided (the device entry): frame f is
// count[f * count_stride] features from feature f * frame_stride; its feature vector is n_nodes[f] entries
// from f * fv_stride of the three fv arrays; eligibility of side s from f * elig_stride[s].
struct BmFrames {
    const int64_t *off, *fv_off;
    const int32_t* count;
    int64_t frame_stride, count_stride, fv_stride, out_stride;
    const uint8_t* desc;
    const float* angle;
    int64_t angle_stride;
    const uint8_t* elig[2];
    int64_t elig_stride[2];
    const int32_t *n_nodes, *fv_node, *fv_end, *fv_idx;
    int32_t n_frames;
};

struct BmOut {
    int32_t *match12, *match21;
    int8_t* bin12;
    int32_t *hist, *n_raw, *status;
};

// One side of a pair, resolved: every pointer is the frame's own block.
struct BmSide {
    int n;    // features, clamped
    int nn;   // nodes, clamped
    int cap;  // entries of the frame's fv_idx block that may be read
    const uint4* desc;
    const float* angle;
    int64_t astride;
    const uint8_t* elig;
    const int32_t *node, *end, *idx;
};

__device__ __forceinline__ BmSide bm_side(const BmFrames& fr, int side, int f, int& flags) {
    BmSide s{};
    if (f < 0 || f >= fr.n_frames) {
        flags |= ORBFE_BOW_BAD_PAIR;
        return s;  // n = nn = 0: nothing of this side is read or written
    }
    int64_t base, nbase, ebase, n, nn, cap;
    if (fr.off) {
        base = fr.off[f];
        n = fr.off[f + 1] - base;
        nbase = fr.fv_off[f];
        nn = fr.fv_off[f + 1] - nbase;
        ebase = base;
        cap = n;
        s.idx = fr.fv_idx + base;
    } else {
        base = (int64_t)f * fr.frame_stride;
        n = fr.count[(int64_t)f * fr.count_stride];
        if (n < 0) flags |= ORBFE_BOW_NEGATIVE, n = 0;
        if (n > fr.out_stride) flags |= ORBFE_BOW_OVER_OUT, n = fr.out_stride;
        if (n > ORBFE_BOW_MAX_FRAME) flags |= ORBFE_BOW_OVER_MAX, n = ORBFE_BOW_MAX_FRAME;
        if (n > fr.frame_stride) flags |= ORBFE_BOW_OVER_FRAME, n = fr.frame_stride;
        nbase = (int64_t)f * fr.fv_stride;
        cap = fr.fv_stride;
        nn = fr.n_nodes[f];
        nn = nn < 0 ? 0 : (nn > cap ? cap : nn);
        ebase = (int64_t)f * fr.elig_stride[side];
        s.idx = fr.fv_idx + nbase;
    }
    s.n = (int)n;
    s.nn = (int)nn;
    s.cap = (int)(cap > ORBFE_BOW_MAX_FRAME ? ORBFE_BOW_MAX_FRAME : cap);
    s.desc = reinterpret_cast<const uint4*>(fr.desc + base * 32);
    s.astride = fr.angle_stride;
    s.angle = fr.angle + base * fr.angle_stride;
    s.elig = fr.elig[side] ? fr.elig[side] + ebase : nullptr;
    s.node = fr.fv_node + nbase;
    s.end = fr.fv_end + nbase;
    return s;
}

// node r's run [a, b) of the frame's fv_idx block, clamped to what may be read
__device__ __forceinline__ void bm_run(const BmSide& s, int r, int& a, int& b) {
    a = r ? s.end[r - 1] : 0;
    b = s.end[r];
    a = a < 0 ? 0 : (a > s.cap ? s.cap : a);
    b = b < a ? a : (b > s.cap ? s.cap : b);
}

// the two smallest of the wave's 64 distinct keys (m1 in, m2 = all ones in), in every lane
__device__ __forceinline__ void bm_min2(unsigned& m1, unsigned& m2) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned a1 = (unsigned)__shfl_xor((int)m1, o, 64);
        const unsigned a2 = (unsigned)__shfl_xor((int)m2, o, 64);
        const unsigned hi = max(m1, a1);
        m1 = min(m1, a1);
        m2 = min(hi, min(m2, a2));
    }
}

__global__ __launch_bounds__(64 * kBmWaves) void k_bow_match(BmFrames fr, const int32_t* __restrict__ pairs, int th,
                                                             int inclusive, double nnratio, BmOut out) {
    __shared__ uint8_t s_blk[ORBFE_BOW_MAX_FRAME];  // frame 2's features: ineligible or matched in this pair
    __shared__ int s_hist[32];
    __shared__ int s_raw, s_next;
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    int flags = 0;
    const BmSide s1 = bm_side(fr, 0, pairs[2 * (int64_t)p], flags);
    const BmSide s2 = bm_side(fr, 1, pairs[2 * (int64_t)p + 1], flags);
    const int n1 = s1.n, n2 = s2.n;
    int32_t* m12 = out.match12 + (int64_t)p * fr.out_stride;
    int32_t* m21 = out.match21 + (int64_t)p * fr.out_stride;
    int8_t* b12 = out.bin12 + (int64_t)p * fr.out_stride;
    for (int i = tid; i < n1; i += 64 * kBmWaves) {
        m12[i] = -1;
        b12[i] = -1;
    }
    for (int i = tid; i < n2; i += 64 * kBmWaves) {
        m21[i] = -1;
        s_blk[i] = (s2.elig && !s2.elig[i]) ? 1 : 0;
    }
    if (tid < 32) s_hist[tid] = 0;
    if (tid == 0) s_raw = s_next = 0;
    // the fills above and a match written below may be stores of different waves to one address
    __threadfence();
    __syncthreads();
    const bool live = !(flags & ORBFE_BOW_BAD_PAIR);
    volatile uint8_t* blk = s_blk;
    int raw = 0;
    int my_i1 = -1;
    uint4 ma = make_uint4(0, 0, 0, 0), mb = ma;
    float ang1 = 0.f;
    // waves take frame 1's nodes from a shared counter: runs differ in length, a fixed stride leaves waves idle
    for (;;) {
        int r = 0;
        if (lane == 0) r = atomicAdd(&s_next, 1);
        r = __builtin_amdgcn_readfirstlane(r);
        if (!live || r >= s1.nn) break;
        const int node = s1.node[r];
        int lo = 0, hi = s2.nn;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s2.node[mid] < node)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo >= s2.nn || s2.node[lo] != node) continue;
        int a1, e1, a2, e2;
        bm_run(s1, r, a1, e1);
        bm_run(s2, lo, a2, e2);
        const int len2 = e2 - a2;
        // the run's first 64 features of frame 2 stay in registers for the whole node
        int i2_0 = -1;
        uint4 ea = make_uint4(0, 0, 0, 0), eb = ea;
        float ang2_0 = 0.f;
        if (lane < len2) {
            i2_0 = s2.idx[a2 + lane];
            if ((unsigned)i2_0 >= (unsigned)n2) i2_0 = -1;
        }
        if (i2_0 >= 0) {
            ea = s2.desc[2 * i2_0];
            eb = s2.desc[2 * i2_0 + 1];
            ang2_0 = s2.angle[i2_0 * s2.astride];
        }
        // frame 1's run, 64 features at a time: lane j stages feature j of the chunk (index, descriptor, angle; -1
        // when it is out of range or ineligible) in one round of loads, and the walk below takes them lane by
        // lane with v_readlane, so the sequential part waits for no global load
        for (int k = a1; k < e1; ++k) {
            const int j = __builtin_amdgcn_readfirstlane((k - a1) & 63);
            if (j == 0) {
                my_i1 = -1;
                if (k + lane < e1) {
                    const int i = s1.idx[k + lane];
                    if ((unsigned)i < (unsigned)n1 && !(s1.elig && !s1.elig[i])) my_i1 = i;
                }
                if (my_i1 >= 0) {
                    ma = s1.desc[2 * my_i1];
                    mb = s1.desc[2 * my_i1 + 1];
                    ang1 = s1.angle[my_i1 * s1.astride];
                }
            }
            const int i1 = __builtin_amdgcn_readlane(my_i1, j);
            if (i1 < 0) continue;
            const uint4 qa = make_uint4(lane_value(ma.x, j), lane_value(ma.y, j), lane_value(ma.z, j), lane_value(ma.w, j));
            const uint4 qb = make_uint4(lane_value(mb.x, j), lane_value(mb.y, j), lane_value(mb.z, j), lane_value(mb.w, j));
            int best1 = 256, best2 = 256, bestpos = -1;
            for (int c = 0; c < len2; c += 64) {
                const int pos = c + lane;
                unsigned d = 256;
                if (c == 0) {
                    if (i2_0 >= 0 && !blk[i2_0]) d = hamming256(ea, eb, qa, qb);
                } else if (pos < len2) {
                    const int i2 = s2.idx[a2 + pos];
                    if ((unsigned)i2 < (unsigned)n2 && !blk[i2]) d = hamming256(s2.desc[2 * i2], s2.desc[2 * i2 + 1], qa, qb);
                }
                unsigned m1 = (d << 16) | (unsigned)pos, m2 = 0xFFFFFFFFu;
                bm_min2(m1, m2);
                const int c1 = (int)(m1 >> 16), c2 = min((int)(m2 >> 16), 256);
                if (c1 < best1) {
                    best2 = min(best1, c2);
                    best1 = c1;
                    bestpos = (int)(m1 & 0xFFFFu);
                } else {
                    best2 = min(best2, c1);
                }
            }
            const bool near = inclusive ? best1 <= th : best1 < th;
            if (bestpos >= 0 && near && (double)best1 < nnratio * (double)best2) {
                const int bp = __builtin_amdgcn_readfirstlane(bestpos);
                int i2;
                float a2f;
                if (bp < 64) {
                    i2 = __builtin_amdgcn_readlane(i2_0, bp);
                    a2f = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ang2_0), bp));
                } else {
                    i2 = s2.idx[a2 + bp];
                    a2f = s2.angle[i2 * s2.astride];
                }
                const float a1f = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ang1), j));
                double rot = (double)a1f - (double)a2f;
                if (rot < 0.0) rot += 360.0;
                const double q = rint(rot * (1.0 / 30));
                int bin = (q >= 0.0 && q <= 30.0) ? (int)q : 31;  // 31: angles outside [0, 360], never a kept bin
                if (bin == 30) bin = 0;
                if (lane == 0) {
                    m12[i1] = i2;
                    m21[i2] = i1;
                    b12[i1] = (int8_t)bin;
                    blk[i2] = 1;
                    atomicAdd(&s_hist[bin], 1);
                }
                ++raw;
            }
        }
    }
    if (lane == 0 && raw) atomicAdd(&s_raw, raw);
    __syncthreads();
    if (tid < 32) out.hist[(int64_t)p * 32 + tid] = s_hist[tid];
    if (tid == 0) {
        out.n_raw[p] = s_raw;
        if (flags) atomicOr(out.status, flags);
    }
}

}  // namespace orbfe

namespace {

void launch_match(const BmFrames& fr, const int32_t* d_pairs, int32_t n_pairs, int32_t th, int32_t inclusive,
                  double nnratio, const BmOut& out, hipStream_t s) {
    hipLaunchKernelGGL(k_bow_match, dim3((unsigned)n_pairs), dim3(64 * kBmWaves), 0, s, fr, d_pairs, (int)th,
                       (int)inclusive, nnratio, out);
    HIPCK(hipGetLastError());
}

// scratch of orbfe_bow_match: process-wide, created on first use and never torn down (the HIP runtime may
// already be gone when static destructors run); callers on several threads take turns
struct Matcher {
    std::mutex mu;
    DevBuf<uint8_t> d_desc, d_elig[2];
    DevBuf<float> d_angle;
    DevBuf<int64_t> d_off;     // off, then fv_off
    DevBuf<int32_t> d_fv;      // fv_node, fv_end, fv_idx, pairs
    DevBuf<int32_t> d_out;     // match12, match21, hist, n_raw, status
    DevBuf<int8_t> d_bin;
    std::vector<int32_t> h_match;  // host staging of match12, match21
    std::vector<int8_t> h_bin;
    TimedStream t;
};
Matcher& matcher() {
    static Matcher* m = new Matcher;
    return *m;
}

}  // namespace

extern "C" {

int orbfe_bow_match_device(const uint8_t* d_desc32, int64_t frame_stride, const int32_t* d_count, int64_t count_stride,
                           int32_t n_frames, const float* d_angle, int64_t angle_stride, const uint8_t* d_elig1,
                           int64_t elig1_stride, const uint8_t* d_elig2, int64_t elig2_stride,
                           const orbfe_bow_out* d_fv, int64_t fv_stride, const int32_t* d_pairs, int32_t n_pairs,
                           int32_t th, int32_t inclusive, double nnratio, const orbfe_bow_match_out* d_out,
                           int64_t out_stride, void* hip_stream) {
    return guarded([&] {
        if (n_frames < 0 || n_pairs < 0 || frame_stride < 0 || count_stride < 1 || angle_stride < 1 ||
            fv_stride < 0 || out_stride < 0 || elig1_stride < 0 || elig2_stride < 0)
            throw Error(ORBFE_EINVAL, "bad argument");
        if (n_pairs == 0) return;
        if (!d_pairs || !d_out || !d_out->match12 || !d_out->match21 || !d_out->bin12 || !d_out->hist ||
            !d_out->n_raw || !d_out->status)
            throw Error(ORBFE_EINVAL, "null argument");
        if (n_frames > 0 && (!d_desc32 || !d_count || !d_angle || !d_fv || !d_fv->n_nodes || !d_fv->fv_node ||
                             !d_fv->fv_end || !d_fv->fv_idx))
            throw Error(ORBFE_EINVAL, "null argument");
        if (reinterpret_cast<uintptr_t>(d_desc32) & 15) throw Error(ORBFE_EINVAL, "descriptors must be 16-byte aligned");
        BmFrames fr{};
        fr.count = d_count;
        fr.frame_stride = frame_stride;
        fr.count_stride = count_stride;
        fr.fv_stride = fv_stride;
        fr.out_stride = out_stride;
        fr.desc = d_desc32;
        fr.angle = d_angle;
        fr.angle_stride = angle_stride;
        fr.elig[0] = d_elig1;
        fr.elig[1] = d_elig2;
        fr.elig_stride[0] = elig1_stride;
        fr.elig_stride[1] = elig2_stride;
        if (n_frames > 0) {
            fr.n_nodes = d_fv->n_nodes;
            fr.fv_node = d_fv->fv_node;
            fr.fv_end = d_fv->fv_end;
            fr.fv_idx = d_fv->fv_idx;
        }
        fr.n_frames = n_frames;
        const BmOut out{d_out->match12, d_out->match21, d_out->bin12, d_out->hist, d_out->n_raw, d_out->status};
        launch_match(fr, d_pairs, n_pairs, th, inclusive, nnratio, out, static_cast<hipStream_t>(hip_stream));
    });
}

int orbfe_bow_match(const uint8_t* desc32, const float* angle, const uint8_t* elig1, const uint8_t* elig2,
                    const int64_t* off, int32_t n_frames, const int64_t* fv_off, const int32_t* fv_node,
                    const int32_t* fv_end, const int32_t* fv_idx, const int32_t* pairs, int32_t n_pairs, int32_t th,
                    int32_t inclusive, double nnratio, const orbfe_bow_match_out* out, int64_t out_stride) {
    return guarded([&] {
        if (n_frames < 0 || n_pairs < 0 || out_stride < 0) throw Error(ORBFE_EINVAL, "bad argument");
        if (n_pairs == 0) return;
        if (!pairs || !out || !out->hist || !out->n_raw) throw Error(ORBFE_EINVAL, "null argument");
        if (n_frames > 0 && (!off || !fv_off)) throw Error(ORBFE_EINVAL, "null argument");
        if (n_frames > 0 && (off[0] != 0 || fv_off[0] != 0)) throw Error(ORBFE_EINVAL, "off[0] and fv_off[0] must be 0");
        std::vector<uint8_t> seen;
        for (int32_t f = 0; f < n_frames; ++f) {
            const int64_t n = off[f + 1] - off[f], nn = fv_off[f + 1] - fv_off[f];
            if (n < 0 || nn < 0) throw Error(ORBFE_EINVAL, at_frame(f, "offsets must not decrease"));
            if (n > ORBFE_BOW_MAX_FRAME || nn > ORBFE_BOW_MAX_FRAME)
                throw Error(ORBFE_EINVAL, at_frame(f, "more features or nodes than the limit of ") +
                                              std::to_string(ORBFE_BOW_MAX_FRAME) + " per frame");
            if (n > 0 && (!desc32 || !angle)) throw Error(ORBFE_EINVAL, "null argument");
            if (nn > 0 && (!fv_node || !fv_end)) throw Error(ORBFE_EINVAL, "null argument");
            check_frame_runs(f, off, fv_off, fv_node, fv_end, fv_idx, seen);
        }
        int64_t longest = 0;
        for (int32_t p = 0; p < n_pairs; ++p) {
            check_pair_frames(pairs, p, n_frames);
            for (int s = 0; s < 2; ++s) {
                const int32_t f = pairs[2 * p + s];
                longest = std::max(longest, off[f + 1] - off[f]);
            }
        }
        if (longest > out_stride) throw Error(ORBFE_EINVAL, "out_stride is shorter than a frame of the pairs");
        if (longest > 0 && (!out->match12 || !out->match21 || !out->bin12)) throw Error(ORBFE_EINVAL, "null argument");
        const int64_t n = off[n_frames], nn = fv_off[n_frames];
        Matcher& m = matcher();
        std::lock_guard<std::mutex> lk(m.mu);
        hipStream_t s = m.t.get();
        const size_t np = (size_t)n_pairs, os = (size_t)out_stride;
        m.d_desc.ensure((size_t)n * 32);
        m.d_angle.ensure(n);
        m.d_off.ensure(2 * ((size_t)n_frames + 1));
        m.d_fv.ensure(2 * (size_t)nn + (size_t)n + 2 * np);
        m.d_out.ensure(2 * np * os + 33 * np + 1);
        m.d_bin.ensure(np * os);
        BmFrames fr{};
        fr.off = m.d_off.p;
        fr.fv_off = m.d_off.p + n_frames + 1;
        fr.out_stride = out_stride;
        fr.desc = m.d_desc.p;
        fr.angle = m.d_angle.p;
        fr.angle_stride = 1;
        int32_t* d_node = m.d_fv.p;
        int32_t* d_end = d_node + nn;
        int32_t* d_idx = d_end + nn;
        int32_t* d_pairs = d_idx + n;
        fr.fv_node = d_node;
        fr.fv_end = d_end;
        fr.fv_idx = d_idx;
        fr.n_frames = n_frames;
        const uint8_t* el[2] = {elig1, elig2};
        for (int k = 0; k < 2; ++k)
            if (el[k] && n > 0) {
                m.d_elig[k].ensure(n);
                HIPCK(hipMemcpyAsync(m.d_elig[k].p, el[k], (size_t)n, hipMemcpyHostToDevice, s));
                fr.elig[k] = m.d_elig[k].p;
            }
        if (n > 0) {
            HIPCK(hipMemcpyAsync(m.d_desc.p, desc32, (size_t)n * 32, hipMemcpyHostToDevice, s));
            HIPCK(hipMemcpyAsync(m.d_angle.p, angle, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
            if (fv_idx) HIPCK(hipMemcpyAsync(d_idx, fv_idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        if (nn > 0) {
            HIPCK(hipMemcpyAsync(d_node, fv_node, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, s));
            HIPCK(hipMemcpyAsync(d_end, fv_end, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        HIPCK(hipMemcpyAsync(m.d_off.p, off, ((size_t)n_frames + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(m.d_off.p + n_frames + 1, fv_off, ((size_t)n_frames + 1) * sizeof(int64_t),
                             hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(d_pairs, pairs, 2 * np * sizeof(int32_t), hipMemcpyHostToDevice, s));
        BmOut d{};
        d.match12 = m.d_out.p;
        d.match21 = d.match12 + np * os;
        d.hist = d.match21 + np * os;
        d.n_raw = d.hist + 32 * np;
        d.status = d.n_raw + np;
        d.bin12 = m.d_bin.p;
        HIPCK(hipMemsetAsync(d.status, 0, sizeof(int32_t), s));
        m.t.begin(s);
        launch_match(fr, d_pairs, n_pairs, th, inclusive, nnratio, d, s);
        m.t.end(s);
        // the blocks come back whole into staging; only the entries the kernel wrote, [0, n1) and [0, n2) of each
        // pair's block, reach the caller's arrays
        m.h_match.resize(2 * np * os);
        m.h_bin.resize(np * os);
        if (np * os) {
            HIPCK(hipMemcpyAsync(m.h_match.data(), d.match12, 2 * np * os * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCK(hipMemcpyAsync(m.h_bin.data(), d.bin12, np * os, hipMemcpyDeviceToHost, s));
        }
        HIPCK(hipMemcpyAsync(out->hist, d.hist, 32 * np * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->n_raw, d.n_raw, np * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out->status) HIPCK(hipMemcpyAsync(out->status, d.status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        m.t.last_ms = m.t.elapsed_ms();
        for (size_t p = 0; p < np; ++p) {
            const size_t l1 = (size_t)(off[pairs[2 * p] + 1] - off[pairs[2 * p]]);
            const size_t l2 = (size_t)(off[pairs[2 * p + 1] + 1] - off[pairs[2 * p + 1]]);
            if (l1) {
                std::memcpy(out->match12 + p * os, &m.h_match[p * os], l1 * sizeof(int32_t));
                std::memcpy(out->bin12 + p * os, &m.h_bin[p * os], l1);
            }
            if (l2) std::memcpy(out->match21 + p * os, &m.h_match[(np + p) * os], l2 * sizeof(int32_t));
        }
    });
}

int orbfe_bow_match_last_ms(float* ms) {
    return guarded([&] {
        if (!ms) throw Error(ORBFE_EINVAL, "null argument");
        Matcher& m = matcher();
        std::lock_guard<std::mutex> lk(m.mu);
        *ms = m.t.last_ms;
    });
}

}  // extern "C"
