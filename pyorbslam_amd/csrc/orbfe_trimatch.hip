// orbfe_trimatch.hip — the epipolar-gated descriptor match of ORBMatcher.search_for_triangulation
// (ORBMatcher.py:584-711) for many keyframe pairs in one launch on gfx950.
//
// The reference walks the two keyframes' DBoW2 feature vectors with a walk of its own (every round draws one
// item from BOTH vectors; equal keys visit the node pair, otherwise one further item of the smaller side is
// discarded, and an exhausted vector at that point lets StopIteration escape).  Inside a visited node pair every
// feature of frame 1 without a map point (in run order) takes, among the features of frame 2's run that have no
// map point and are not yet matched, the one with the smallest Hamming distance <= th that also passes two
// float64 gates: the distance to the epipole (only when both features are monocular) and the distance to the
// epipolar line.  On equal distances the LAST candidate in run order wins (the reference skips only on
// dist > bestDist) and there is no second-best ratio.  A matched feature of frame 2 is blocked for the later
// features of frame 1.
//
// The walk runs on the host (orbfe_tri_match below) and reaches the device as a list of visited (run 1, run 2)
// pairs per keyframe pair.  k_tri_match: one workgroup per keyframe pair, one wave per visited node pair at a
// time (taken from a counter in LDS).  Inside a node the wave walks frame 1's run sequentially with that feature
// wave-uniform (staged 64 at a time, one per lane, read back with v_readlane), while the 64 lanes hold 64
// features of frame 2's run (the first 64 stay in registers: descriptor, angle, coordinates, the two
// thresholds of their octave; longer runs re-read the further chunks per feature of frame 1).  A lane's key is
// dist << 16 | (0xFFFF - position in the run), all ones when it holds no candidate that passes the gates; the
// wave-wide minimum, kept running across chunks, is the smallest distance and among equals the last position.
// Blocked flags are one byte per feature of frame 2 in LDS, preset from its map point and, under only_stereo,
// its mono flag.  The gates are IEEE double operations in the reference's order (-ffp-contract=off, correctly
// rounded division); the reference squares with `** 2`, which can differ from v * v by one ulp, so a gate whose
// left side lies within thr * 2^-48 of its threshold marks the pair ORBFE_TRI_MARGINAL for the caller to redo.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_host_util.h"

using namespace orbfe;

namespace orbfe {

constexpr int kTmWaves = 8;  // waves per workgroup: visited node pairs in flight per keyframe pair
constexpr unsigned kTmNone = 0xFFFFFFFFu;
constexpr double kTmMargin = 0x1p-48;
constexpr double kTmMinNormal = 0x1p-1022;

// Ragged frames: frame f is features [off[f], off[f + 1]); its run ends are entries [fv_off[f], fv_off[f + 1]) of
// fv_end, its fv_idx block starts at off[f], its level tables at lvl_off[f].
struct TmFrames {
    const int64_t *off, *fv_off, *lvl_off;
    const uint8_t* desc;
    const float* angle;
    const double* xy;
    const int32_t* octave;
    const uint8_t* flags;
    const int32_t *fv_end, *fv_idx;
    const double *thr_epi, *thr_ex;
    int64_t out_stride;
};

// The pairs: frame indices, F12 (9 doubles, row-major), the epipole (2 doubles) and the visited (run 1, run 2)
// pairs [vis_off[p], vis_off[p + 1]) of vis.
struct TmPairs {
    const int32_t* pairs;
    const double *F12, *epipole;
    const int64_t* vis_off;
    const int32_t* vis;
};

struct TmOut {
    int32_t* match12;
    int8_t* bin12;
    int32_t *hist, *n_raw, *status;
};

__device__ __forceinline__ unsigned tm_min(unsigned m) {
#pragma unroll
    for (int o = 32; o; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o, 64));
    return m;
}

// lhs is within thr * 2^-48 of thr: how the reference's `** 2` rounds could decide the comparison
__device__ __forceinline__ bool tm_marginal(double lhs, double thr) { return fabs(lhs - thr) <= thr * kTmMargin; }

// One candidate against one feature of frame 1: true when both gates pass.  mono: both features are monocular.
__device__ __forceinline__ bool tm_gates(bool mono, double ex, double ey, double a, double b, double c, double den,
                                         double x2, double y2, double t_ex, double t_epi, int& marginal) {
    if (mono) {
        const double dx = ex - x2, dy = ey - y2;
        const double e = dx * dx + dy * dy;
        if (tm_marginal(e, t_ex)) marginal = 1;
        if (e < t_ex) return false;
    }
    if (den == 0.0) return false;
    if (den < kTmMinNormal) marginal = 1;
    const double num = a * x2 + b * y2 + c;
    const double q = num * num / den;
    if (tm_marginal(q, t_epi)) marginal = 1;
    return q < t_epi;
}

__global__ __launch_bounds__(64 * kTmWaves) void k_tri_match(TmFrames fr, TmPairs pr, int th, int only_stereo,
                                                             TmOut out) {
    __shared__ uint8_t s_blk[ORBFE_BOW_MAX_FRAME];  // frame 2's features: ineligible or matched in this pair
    __shared__ int s_hist[32];
    __shared__ int s_raw, s_next, s_status;
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int f1 = pr.pairs[2 * (int64_t)p], f2 = pr.pairs[2 * (int64_t)p + 1];
    const int64_t base1 = fr.off[f1], base2 = fr.off[f2];
    const int n1 = (int)(fr.off[f1 + 1] - base1), n2 = (int)(fr.off[f2 + 1] - base2);
    const uint4* desc1 = reinterpret_cast<const uint4*>(fr.desc + base1 * 32);
    const uint4* desc2 = reinterpret_cast<const uint4*>(fr.desc + base2 * 32);
    const float *ang1p = fr.angle + base1, *ang2p = fr.angle + base2;
    const double *xy1 = fr.xy + 2 * base1, *xy2 = fr.xy + 2 * base2;
    const uint8_t *fl1 = fr.flags + base1, *fl2 = fr.flags + base2;
    const int32_t* oct2 = fr.octave + base2;
    const int32_t *idx1 = fr.fv_idx + base1, *idx2 = fr.fv_idx + base2;
    const int32_t *end1 = fr.fv_end + fr.fv_off[f1], *end2 = fr.fv_end + fr.fv_off[f2];
    const double *tepi2 = fr.thr_epi + fr.lvl_off[f2], *tex2 = fr.thr_ex + fr.lvl_off[f2];
    const uint8_t need = only_stereo ? (ORBFE_TRI_ELIGIBLE | ORBFE_TRI_STEREO) : ORBFE_TRI_ELIGIBLE;
    int32_t* m12 = out.match12 + (int64_t)p * fr.out_stride;
    int8_t* b12 = out.bin12 + (int64_t)p * fr.out_stride;
    for (int i = tid; i < n1; i += 64 * kTmWaves) {
        m12[i] = -1;
        b12[i] = -1;
    }
    for (int i = tid; i < n2; i += 64 * kTmWaves) s_blk[i] = (fl2[i] & need) == need ? 0 : 1;
    if (tid < 32) s_hist[tid] = 0;
    if (tid == 0) s_raw = s_next = s_status = 0;
    // the fills above and a match written below may be stores of different waves to one address
    __threadfence();
    __syncthreads();
    const double* F = pr.F12 + 9 * (int64_t)p;
    const double F00 = F[0], F01 = F[1], F02 = F[2], F10 = F[3], F11 = F[4], F12 = F[5], F20 = F[6], F21 = F[7],
                 F22 = F[8];
    const double ex = pr.epipole[2 * (int64_t)p], ey = pr.epipole[2 * (int64_t)p + 1];
    const int32_t* vis = pr.vis + 2 * pr.vis_off[p];
    const int n_vis = (int)(pr.vis_off[p + 1] - pr.vis_off[p]);
    volatile uint8_t* blk = s_blk;
    int raw = 0, marginal = 0;
    int my_i1 = -1, my_mono1 = 0;
    uint4 ma = make_uint4(0, 0, 0, 0), mb = ma;
    float my_ang1 = 0.f;
    double my_x1 = 0.0, my_y1 = 0.0;
    // waves take visited node pairs from a shared counter: runs differ in length, a fixed stride leaves waves idle
    for (;;) {
        int v = 0;
        if (lane == 0) v = atomicAdd(&s_next, 1);
        v = __builtin_amdgcn_readfirstlane(v);
        if (v >= n_vis) break;
        const int r1 = vis[2 * v], r2 = vis[2 * v + 1];
        const int a1 = r1 ? end1[r1 - 1] : 0, e1 = end1[r1];
        const int a2 = r2 ? end2[r2 - 1] : 0, e2 = end2[r2];
        const int len2 = e2 - a2;
        // the run's first 64 features of frame 2 stay in registers for the whole node
        int i2_0 = -1, mono2_0 = 0;
        uint4 ea = make_uint4(0, 0, 0, 0), eb = ea;
        float ang2_0 = 0.f;
        double x2_0 = 0.0, y2_0 = 0.0, tex_0 = 0.0, tepi_0 = 0.0;
        if (lane < len2) {
            i2_0 = idx2[a2 + lane];
            ea = desc2[2 * i2_0];
            eb = desc2[2 * i2_0 + 1];
            ang2_0 = ang2p[i2_0];
            x2_0 = xy2[2 * i2_0];
            y2_0 = xy2[2 * i2_0 + 1];
            const int o = oct2[i2_0];
            tex_0 = tex2[o];
            tepi_0 = tepi2[o];
            mono2_0 = !(fl2[i2_0] & ORBFE_TRI_STEREO);
        }
        // frame 1's run, 64 features at a time: lane j stages feature j of the chunk (-1 when it is ineligible) in
        // one round of loads, and the walk below takes them lane by lane, so it waits for no global load
        for (int k = a1; k < e1; ++k) {
            const int j = __builtin_amdgcn_readfirstlane((k - a1) & 63);
            if (j == 0) {
                my_i1 = -1;
                if (k + lane < e1) {
                    const int i = idx1[k + lane];
                    if ((fl1[i] & need) == need) my_i1 = i;
                }
                if (my_i1 >= 0) {
                    ma = desc1[2 * my_i1];
                    mb = desc1[2 * my_i1 + 1];
                    my_ang1 = ang1p[my_i1];
                    my_x1 = xy1[2 * my_i1];
                    my_y1 = xy1[2 * my_i1 + 1];
                    my_mono1 = !(fl1[my_i1] & ORBFE_TRI_STEREO);
                }
            }
            const int i1 = __builtin_amdgcn_readlane(my_i1, j);
            if (i1 < 0) continue;
            const uint4 qa = make_uint4(lane_value(ma.x, j), lane_value(ma.y, j), lane_value(ma.z, j), lane_value(ma.w, j));
            const uint4 qb = make_uint4(lane_value(mb.x, j), lane_value(mb.y, j), lane_value(mb.z, j), lane_value(mb.w, j));
            const bool mono1 = __builtin_amdgcn_readlane(my_mono1, j) != 0;
            const double x1 = lane_value(my_x1, j), y1 = lane_value(my_y1, j);
            // the epipolar line of i1 in frame 2 (check_dist_epipolar_line, ORBMatcher.py:699-704), once per i1
            const double a = x1 * F00 + y1 * F10 + F20;
            const double b = x1 * F01 + y1 * F11 + F21;
            const double c = x1 * F02 + y1 * F12 + F22;
            const double den = a * a + b * b;
            unsigned best = kTmNone;
            for (int c0 = 0; c0 < len2; c0 += 64) {
                const int pos = c0 + lane;
                unsigned key = kTmNone;
                if (c0 == 0) {
                    if (i2_0 >= 0 && !blk[i2_0]) {
                        const unsigned d = hamming256(ea, eb, qa, qb);
                        if ((int)d <= th &&
                            tm_gates(mono1 && mono2_0, ex, ey, a, b, c, den, x2_0, y2_0, tex_0, tepi_0, marginal))
                            key = (d << 16) | (0xFFFFu - (unsigned)pos);
                    }
                } else if (pos < len2) {
                    const int i2 = idx2[a2 + pos];
                    if (!blk[i2]) {
                        const unsigned d = hamming256(desc2[2 * i2], desc2[2 * i2 + 1], qa, qb);
                        if ((int)d <= th) {
                            const int o = oct2[i2];
                            if (tm_gates(mono1 && !(fl2[i2] & ORBFE_TRI_STEREO), ex, ey, a, b, c, den, xy2[2 * i2],
                                         xy2[2 * i2 + 1], tex2[o], tepi2[o], marginal))
                                key = (d << 16) | (0xFFFFu - (unsigned)pos);
                        }
                    }
                }
                best = min(best, tm_min(key));
            }
            if (best != kTmNone) {
                const int bp = __builtin_amdgcn_readfirstlane((int)(0xFFFFu - (best & 0xFFFFu)));
                int i2;
                float a2f;
                if (bp < 64) {
                    i2 = __builtin_amdgcn_readlane(i2_0, bp);
                    a2f = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ang2_0), bp));
                } else {
                    i2 = idx2[a2 + bp];
                    a2f = ang2p[i2];
                }
                const float a1f = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_ang1), j));
                double rot = (double)a1f - (double)a2f;
                if (rot < 0.0) rot += 360.0;
                const double q = rint(rot * (1.0 / 30));
                int bin = (q >= 0.0 && q <= 30.0) ? (int)q : 31;  // 31: angles outside [0, 360], never a kept bin
                if (bin == 30) bin = 0;
                if (bin == 31) marginal = 1;
                if (lane == 0) {
                    m12[i1] = i2;
                    b12[i1] = (int8_t)bin;
                    blk[i2] = 1;
                    atomicAdd(&s_hist[bin], 1);
                }
                ++raw;
            }
        }
    }
    if (lane == 0 && raw) atomicAdd(&s_raw, raw);
    if (marginal) atomicOr(&s_status, ORBFE_TRI_MARGINAL);
    __syncthreads();
    if (tid < 32) out.hist[(int64_t)p * 32 + tid] = s_hist[tid];
    if (tid == 0) {
        out.n_raw[p] = s_raw;
        out.status[p] = s_status;
    }
}

}  // namespace orbfe

namespace {

// scratch of orbfe_tri_match: process-wide, created on first use and never torn down (the HIP runtime may
// already be gone when static destructors run); callers on several threads take turns
struct TriMatcher {
    std::mutex mu;
    DevBuf<uint8_t> d_desc, d_flags;
    DevBuf<float> d_angle;
    DevBuf<double> d_f64;    // xy, thr_epi, thr_ex, F12, epipole
    DevBuf<int64_t> d_i64;   // off, fv_off, lvl_off, vis_off
    DevBuf<int32_t> d_i32;   // octave, fv_end, fv_idx, pairs, vis
    DevBuf<int32_t> d_out;   // match12, hist, n_raw, status
    DevBuf<int8_t> d_bin;
    std::vector<int32_t> h_match;  // host staging of match12
    std::vector<int8_t> h_bin;
    TimedStream t;
};
TriMatcher& tri_matcher() {
    static TriMatcher* m = new TriMatcher;
    return *m;
}

std::string at_pair(int32_t p, const char* what) { return "pair " + std::to_string(p) + ": " + what; }

// The reference's walk over two ascending node lists (ORBMatcher.py:604-677): the visited (run 1, run 2) pairs are
// appended to vis; false when the discard of the smaller side finds its list exhausted (StopIteration escapes).
bool tri_walk(const int32_t* node1, int64_t nn1, const int32_t* node2, int64_t nn2, std::vector<int32_t>& vis) {
    int64_t i = 0, j = 0;
    for (;;) {
        if (i >= nn1) return true;
        const int64_t r1 = i++;
        if (j >= nn2) return true;
        const int64_t r2 = j++;
        if (node1[r1] == node2[r2]) {
            vis.push_back((int32_t)r1);
            vis.push_back((int32_t)r2);
        } else if (node1[r1] < node2[r2]) {
            if (i >= nn1) return false;
            ++i;
        } else {
            if (j >= nn2) return false;
            ++j;
        }
    }
}

}  // namespace

extern "C" {

int orbfe_tri_match(const uint8_t* desc32, const float* angle, const double* xy, const int32_t* octave,
                    const uint8_t* flags, const int64_t* off, int32_t n_frames, const int64_t* fv_off,
                    const int32_t* fv_node, const int32_t* fv_end, const int32_t* fv_idx, const int64_t* lvl_off,
                    const double* thr_epi, const double* thr_ex, const int32_t* pairs, const double* F12,
                    const double* epipole, int32_t n_pairs, int32_t th, int32_t only_stereo,
                    const orbfe_tri_match_out* out, int64_t out_stride) {
    return guarded([&] {
        if (n_frames < 0 || n_pairs < 0 || out_stride < 0 || th < 0 || th > 256)
            throw Error(ORBFE_EINVAL, "bad argument");
        if (n_pairs == 0) return;
        if (!pairs || !F12 || !epipole || !out || !out->hist || !out->n_raw || !out->status || !out->stopped)
            throw Error(ORBFE_EINVAL, "null argument");
        if (n_frames > 0 && (!off || !fv_off || !lvl_off)) throw Error(ORBFE_EINVAL, "null argument");
        if (n_frames > 0 && (off[0] != 0 || fv_off[0] != 0 || lvl_off[0] != 0))
            throw Error(ORBFE_EINVAL, "off[0], fv_off[0] and lvl_off[0] must be 0");
        std::vector<uint8_t> seen;
        for (int32_t f = 0; f < n_frames; ++f) {
            const int64_t n = off[f + 1] - off[f], nn = fv_off[f + 1] - fv_off[f], nl = lvl_off[f + 1] - lvl_off[f];
            if (n < 0 || nn < 0 || nl < 0) throw Error(ORBFE_EINVAL, at_frame(f, "offsets must not decrease"));
            if (n > ORBFE_BOW_MAX_FRAME || nn > ORBFE_BOW_MAX_FRAME)
                throw Error(ORBFE_EINVAL, at_frame(f, "more features or nodes than the limit of ") +
                                              std::to_string(ORBFE_BOW_MAX_FRAME) + " per frame");
            if (n > 0 && (!desc32 || !angle || !xy || !octave || !flags)) throw Error(ORBFE_EINVAL, "null argument");
            if (nn > 0 && (!fv_node || !fv_end)) throw Error(ORBFE_EINVAL, "null argument");
            if (nl > 0 && (!thr_epi || !thr_ex)) throw Error(ORBFE_EINVAL, "null argument");
            if (nl > 0 && !(all_finite(thr_epi + lvl_off[f], nl) && all_finite(thr_ex + lvl_off[f], nl)))
                throw Error(ORBFE_EINVAL, at_frame(f, "a level threshold is not finite"));
            if (n > 0 && !all_finite(xy + 2 * off[f], 2 * n))
                throw Error(ORBFE_EINVAL, at_frame(f, "a keypoint coordinate is not finite"));
            for (int64_t i = 0; i < n; ++i) {
                const int32_t o = octave[off[f] + i];
                if (o < 0 || o >= nl) throw Error(ORBFE_EINVAL, at_frame(f, "an octave is outside the level table"));
            }
            check_frame_runs(f, off, fv_off, fv_node, fv_end, fv_idx, seen);
        }
        int64_t longest = 0;
        for (int32_t p = 0; p < n_pairs; ++p) {
            check_pair_frames(pairs, p, n_frames);
            longest = std::max(longest, off[pairs[2 * p] + 1] - off[pairs[2 * p]]);
            if (!all_finite(F12 + 9 * (int64_t)p, 9)) throw Error(ORBFE_EINVAL, at_pair(p, "F12 is not finite"));
            if (!all_finite(epipole + 2 * (int64_t)p, 2))
                throw Error(ORBFE_EINVAL, at_pair(p, "the epipole is not finite"));
        }
        if (longest > out_stride) throw Error(ORBFE_EINVAL, "out_stride is shorter than a frame of the pairs");
        if (longest > 0 && (!out->match12 || !out->bin12)) throw Error(ORBFE_EINVAL, "null argument");
        // the reference's walk, per pair; a pair whose walk stops gets no work
        const size_t np = (size_t)n_pairs, os = (size_t)out_stride;
        std::vector<int64_t> vis_off(np + 1, 0);
        std::vector<int32_t> vis;
        for (size_t p = 0; p < np; ++p) {
            const int32_t f1 = pairs[2 * p], f2 = pairs[2 * p + 1];
            const size_t before = vis.size();
            const bool ok = tri_walk(fv_node + fv_off[f1], fv_off[f1 + 1] - fv_off[f1], fv_node + fv_off[f2],
                                     fv_off[f2 + 1] - fv_off[f2], vis);
            if (!ok) vis.resize(before);
            out->stopped[p] = ok ? 0 : 1;
            vis_off[p + 1] = (int64_t)(vis.size() / 2);
        }
        const int64_t n = off[n_frames], nn = fv_off[n_frames], nl = lvl_off[n_frames];
        const size_t nv = vis.size() / 2;
        TriMatcher& m = tri_matcher();
        std::lock_guard<std::mutex> lk(m.mu);
        hipStream_t s = m.t.get();
        const size_t nf1 = (size_t)n_frames + 1;
        m.d_desc.ensure((size_t)n * 32);
        m.d_flags.ensure(n);
        m.d_angle.ensure(n);
        m.d_f64.ensure(2 * (size_t)n + 2 * (size_t)nl + 11 * np);
        m.d_i64.ensure(3 * nf1 + np + 1);
        m.d_i32.ensure(2 * (size_t)n + (size_t)nn + 2 * np + 2 * nv);
        m.d_out.ensure(np * os + 34 * np);
        m.d_bin.ensure(np * os);
        double* d_xy = m.d_f64.p;
        double* d_tepi = d_xy + 2 * n;
        double* d_tex = d_tepi + nl;
        double* d_F = d_tex + nl;
        double* d_epi = d_F + 9 * np;
        int64_t* d_off = m.d_i64.p;
        int64_t* d_fvoff = d_off + nf1;
        int64_t* d_lvloff = d_fvoff + nf1;
        int64_t* d_visoff = d_lvloff + nf1;
        int32_t* d_oct = m.d_i32.p;
        int32_t* d_idx = d_oct + n;
        int32_t* d_end = d_idx + n;
        int32_t* d_pairs = d_end + nn;
        int32_t* d_vis = d_pairs + 2 * np;
        auto up = [&](void* dst, const void* src, size_t bytes) {
            if (bytes) HIPCK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        };
        up(m.d_desc.p, desc32, (size_t)n * 32);
        up(m.d_flags.p, flags, (size_t)n);
        up(m.d_angle.p, angle, (size_t)n * sizeof(float));
        up(d_xy, xy, 2 * (size_t)n * sizeof(double));
        up(d_tepi, thr_epi, (size_t)nl * sizeof(double));
        up(d_tex, thr_ex, (size_t)nl * sizeof(double));
        up(d_F, F12, 9 * np * sizeof(double));
        up(d_epi, epipole, 2 * np * sizeof(double));
        up(d_off, off, nf1 * sizeof(int64_t));
        up(d_fvoff, fv_off, nf1 * sizeof(int64_t));
        up(d_lvloff, lvl_off, nf1 * sizeof(int64_t));
        up(d_visoff, vis_off.data(), (np + 1) * sizeof(int64_t));
        up(d_oct, octave, (size_t)n * sizeof(int32_t));
        if (fv_idx) up(d_idx, fv_idx, (size_t)n * sizeof(int32_t));
        up(d_end, fv_end, (size_t)nn * sizeof(int32_t));
        up(d_pairs, pairs, 2 * np * sizeof(int32_t));
        up(d_vis, vis.data(), 2 * nv * sizeof(int32_t));
        TmFrames fr{};
        fr.off = d_off;
        fr.fv_off = d_fvoff;
        fr.lvl_off = d_lvloff;
        fr.desc = m.d_desc.p;
        fr.angle = m.d_angle.p;
        fr.xy = d_xy;
        fr.octave = d_oct;
        fr.flags = m.d_flags.p;
        fr.fv_end = d_end;
        fr.fv_idx = d_idx;
        fr.thr_epi = d_tepi;
        fr.thr_ex = d_tex;
        fr.out_stride = out_stride;
        const TmPairs pr{d_pairs, d_F, d_epi, d_visoff, d_vis};
        TmOut d{};
        d.match12 = m.d_out.p;
        d.hist = d.match12 + np * os;
        d.n_raw = d.hist + 32 * np;
        d.status = d.n_raw + np;
        d.bin12 = m.d_bin.p;
        m.t.begin(s);
        hipLaunchKernelGGL(k_tri_match, dim3((unsigned)n_pairs), dim3(64 * kTmWaves), 0, s, fr, pr, (int)th,
                           (int)(only_stereo != 0), d);
        HIPCK(hipGetLastError());
        m.t.end(s);
        // the blocks come back whole into staging; only the entries the kernel wrote, [0, n1) of each pair's block,
        // reach the caller's arrays
        m.h_match.resize(np * os);
        m.h_bin.resize(np * os);
        if (np * os) {
            HIPCK(hipMemcpyAsync(m.h_match.data(), d.match12, np * os * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCK(hipMemcpyAsync(m.h_bin.data(), d.bin12, np * os, hipMemcpyDeviceToHost, s));
        }
        HIPCK(hipMemcpyAsync(out->hist, d.hist, 32 * np * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->n_raw, d.n_raw, np * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(out->status, d.status, np * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        m.t.last_ms = m.t.elapsed_ms();
        for (size_t p = 0; p < np; ++p) {
            const size_t l1 = (size_t)(off[pairs[2 * p] + 1] - off[pairs[2 * p]]);
            if (l1) {
                std::memcpy(out->match12 + p * os, &m.h_match[p * os], l1 * sizeof(int32_t));
                std::memcpy(out->bin12 + p * os, &m.h_bin[p * os], l1);
            }
        }
    });
}

int orbfe_tri_match_last_ms(float* ms) {
    return guarded([&] {
        if (!ms) throw Error(ORBFE_EINVAL, "null argument");
        TriMatcher& m = tri_matcher();
        std::lock_guard<std::mutex> lk(m.mu);
        *ms = m.t.last_ms;
    });
}

}  // extern "C"
