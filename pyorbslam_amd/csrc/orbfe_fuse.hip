// orbfe_fuse.hip — the search half of the reference's three projection searches, for every (keyframe, map point) of a
// call in one launch on gfx950: ORBMatcher.fuse_pkf_mp (ORBMatcher.py:498-567) as k_fuse_search, and LoopClosing's two
// Sim3 searches, ORBMatcher.fuse_kf_scw_mp (:395-480) and ORBMatcher.search_by_projection_ckf_scw_mp (:850-922), as
// k_scw_search; and the two directions of ORBMatcher.search_by_sim3 (:713-848) for many keyframe pairs as
// k_sim3_search; and relocalisation's ORBMatcher.search_by_projection_f_kf_f (:924-1008) into many frames as
// k_fkf_search; and tracking's local-map search, Frame.is_in_frustum (Frame.py:328-371) followed by
// ORBMatcher.search_by_projection_f_p (:215-283), as k_local_search; and tracking's motion-model search,
// ORBMatcher.search_by_projection_f_f (:291-393), for many (current frame, last frame) pairs as k_ff_search.  All six
// kernels are instantiations of one body, proj_search<kMode>.
//
// The reference projects each map point into a keyframe, gates it (depth sign, image bounds, scale-invariance
// distances, viewing angle), predicts its pyramid level, searches the keyframe's grid in a window of radius
// th * scale[level] (KeyFrame.get_features_in_area, KeyFrame.py:432-460), keeps the candidates whose octave is the
// level or one below, and takes the candidate of the smallest Hamming distance; among equal distances the EARLIEST
// in visiting order (column ix outer, row iy inner, the cell's list as stored) wins, because it replaces only on
// dist < bestDist.  None of this reads what a fusion changes, so it runs here for all items at once and the caller
// applies the matches afterwards in the reference's order.
//
// What the four variants do not share:
//   k_fuse_search  also projects the right coordinate ur = u - bf / z and filters the candidates by a chi-square on
//                  the reprojection error (three terms against 7.8 for a stereo feature, two against 5.99 for a mono
//                  one).
//   k_scw_search   has neither (slot 4 of the keyframe block, bf, is not read; u_right and inv_sigma2 are null); the
//                  pose is the one a Sim3 gives (the caller divides the scale out on the host, with the reference's
//                  expressions); and it has one more input: a byte per feature that takes the feature out of the
//                  candidates (the ckf search skips a feature whose vpMatched slot is taken).  A blocked entry is
//                  skipped first: it decides nothing, so it marks nothing either.
//
//   k_sim3_search  is k_scw_search without the blocked byte and without the viewing gate (the normal is not read), and
//                  it reads nothing of the target's block before the bounds: the camera coordinates come in two
//                  stages with a rounding in between, c1 = Rw p + tw and c = sR c1 + t, from the search's own
//                  scalars; the intrinsics are the search's too (the reference projects both directions with
//                  pKF1's); and the distance that is gated and that predicts the level is |c| in the target camera,
//                  so the Sim3's scale moves the level.  Its launch is ragged: a search is a target, a pose and a
//                  list of rows of the shared point table, and a 1-D grid runs over a host-built table of (search,
//                  first item) chunks, so no workgroup straddles two searches and an empty search launches nothing.
//
//   k_fkf_search   searches a Frame, not a KeyFrame (Frame.get_features_in_area, Frame.py:373-416), with
//                  k_sim3_search's ragged launch (a search is a target frame and a list of rows of the point table;
//                  there are no search scalars, the pose and the intrinsics are the target block's) and
//                  k_scw_search's blocked byte.  It has no depth gate: a point behind the camera whose u, v land
//                  inside the bounds is searched, and only |z| within its bound of 0 (or 1 / z, u or v not finite)
//                  marks.  u is (fx * xc) * invz + cx, the reference's order.  The image bounds are inclusive at both
//                  ends.  The distance is |p - Ow| as in k_scw_search; there is no viewing gate and the normal is not
//                  read.  Both ends of the cell window truncate toward zero (int()), so a bound in (-1, 1) is cell 0
//                  and only the integers of magnitude >= 1 can flip one.  A candidate's octave lies in
//                  [level - 1, level + 1]: three octaves, the others keep two.
//
//   k_local_search is k_fkf_search's Frame target, ragged launch and blocked byte with what tracking's search adds:
//                  the depth gate pc.z < 0 (pc.z == 0 marks: the reference's NaN comparisons can let such a point
//                  through); ur = u - bf / z as in k_fuse_search; the viewing gate on the cosine itself,
//                  (PO . n) / dist < limit with one limit per search; the radius from the cosine (2.5 above 0.998,
//                  else 4, times th only where the caller's th != 1, times scale[level]); two octaves; a stereo gate
//                  per candidate (a feature whose right coordinate is > 0 is left out when |ur - uR| > r); and the
//                  second smallest key besides the smallest.  It also gives what is_in_frustum decides: in_view and
//                  the level, which stand whatever becomes of the window.
//
//   k_ff_search    is k_local_search's Frame target, ragged launch, blocked byte, depth gate, ur and per-candidate
//                  stereo gate, without any gate on the point itself: no distance gate, no viewing gate and no level
//                  prediction (slots 3-8 of a point's scalars are not read).  The level is the item's own (item_level,
//                  the octave of the last frame's keypoint), th is the search's (one double per search, where
//                  k_local_search has its cosine limit), and a per-search mode chooses the candidates' octaves:
//                  [level - 1, level + 1], [level, inf) when the camera moved forward, [0, level] when backward.  Only
//                  the smallest key comes back.
//
// The depth gate: fuse_pkf_mp and fuse_kf_scw_mp skip z < 0, the ckf search z <= 0.  At z == 0 the first two run on to
// 1 / 0, u and v become inf or NaN and fail the image test, so all three skip the point and one code path serves them.
//
// proj_search: a workgroup is (keyframe, chunk of kPsChunk points).  Phase 1: thread t does point t's geometry in
// IEEE double (-ffp-contract=off, correctly rounded division and square root) and leaves u, v (and ur), their error
// bounds, the radius, the level and the clamped cell window in LDS.  Phase 2: groups of kPsGroup lanes take the
// chunk's points in turn; for one column ix the window's cells are one contiguous range of the grid's CSR, whose
// entries the lanes take kPsGroup at a time.  A lane's key is dist << 16 | position in the keyframe's CSR (all ones
// without a candidate); the __shfl_xor minimum over the group is the smallest distance and among equals the
// earliest visited.
//
// The reference's arithmetic is not this one: float32 poses and positions make it project, take the norm and the
// dot product in float32, it squares through pow, and its log is another library's.  Every value a decision
// compares therefore carries an absolute bound on how far the reference's value can lie from it, built from the
// magnitudes of the summed terms and scaled by `eps` (the caller's unit of rounding: 2^-23 for float32 inputs,
// 2^-48 for float64).  A decision whose two sides lie within the bound marks the item ORBFE_FUSE_MARGINAL; the
// outputs are then this arithmetic's and the caller redoes the item with the reference's expressions.  The
// derivation is in DESIGN.md.
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

constexpr int kPsChunk = ORBFE_FUSE_CHUNK;  // points per workgroup, one thread each in phase 1
constexpr int kPsGroup = 16;                // lanes that share one point's candidates in phase 2
constexpr unsigned kPsNone = 0xFFFFFFFFu;
constexpr int kPsKfF64 = ORBFE_FUSE_KF_F64;
constexpr int kPsPtF64 = ORBFE_FUSE_PT_F64;
constexpr int kPsSim3F64 = ORBFE_SIM3_F64;

struct PsKfs {
    const double* f64;   // kPsKfF64 per keyframe
    const int32_t* i32;  // cols, rows, levels per keyframe
    const int64_t *off, *cell_at, *idx_at, *lvl_off;
    const double *xy, *scale;
    const double *u_right, *inv_sigma2;  // k_fuse_search only
    const int32_t *octave, *cell_off, *cell_idx;
    const uint8_t* desc;
    const uint8_t* blocked;  // k_scw_search and k_fkf_search only, and there null when nothing is blocked
};

struct PsPts {
    const double* f64;  // kPsPtF64 per point
    const uint8_t* desc;
    int64_t n;
};

struct PsOut {
    int32_t *best_idx, *best_dist;
    uint8_t* status;
    int64_t stride;  // k_sim3_search, k_fkf_search, k_local_search: not read, the outputs are flat over the items
    // k_local_search only
    int32_t *second_idx, *second_dist, *level;
    uint8_t* in_view;
};

// k_sim3_search and k_fkf_search: the searches, their items and the launch's chunk table
struct PsSim3 {
    const double* f64;       // kPsSim3F64 per search; k_fkf_search: null, a search has no scalars of its own;
                             // k_local_search: one per search, the viewing cosine's limit
    const int32_t* kf;       // target keyframe per search
    const int64_t* off;      // search s owns items [off[s], off[s + 1])
    const int32_t* item_pt;  // point table row per item
    const int64_t* chunk;    // (search, first item) per workgroup
};

// k_ff_search only: what a search and an item have besides PsSim3 (whose f64 holds one double per search, its th)
struct PsFf {
    const int32_t* mode;        // per search: 0 [level - 1, level + 1], 1 forward [level, inf), 2 backward [0, level]
    const int32_t* item_level;  // per item, beside item_pt: the octave of the last frame's keypoint
};

enum PsMode { kPsFuse, kPsScw, kPsSim3, kPsFkf, kPsLocal, kPsFf };

// every margin test is strict: a bound of zero means every summed term was zero, and then the reference's value
// is this one exactly
__device__ __forceinline__ bool near_int(double a, double e) { return fabs(a - rint(a)) < e; }

template <PsMode kMode>
__device__ __forceinline__ void proj_search(const PsKfs& kf, const PsPts& pt, double th, double eps,
                                            const PsOut& out, [[maybe_unused]] const PsSim3& sx,
                                            [[maybe_unused]] int th_on = 0,
                                            [[maybe_unused]] const PsFf& ff = PsFf{}) {
    constexpr bool kFuse = kMode == kPsFuse, kScw = kMode == kPsScw, kSim3 = kMode == kPsSim3;
    constexpr bool kLocal = kMode == kPsLocal, kFf = kMode == kPsFf;
    constexpr bool kGate = kLocal || kFf;  // the depth gate's mark at zero and the per-candidate stereo gate
    // a Frame target: the reference's (fx * xc) * invz, inclusive bounds, a window truncated at both ends
    constexpr bool kFkf = kMode == kPsFkf || kGate;
    constexpr bool kDepthFree = kMode == kPsFkf;  // no depth gate
    constexpr bool kRagged = kSim3 || kFkf;  // a 1-D grid over the chunk table, outputs flat over the items
    constexpr bool kBlocked = kScw || kFkf;
    constexpr bool kRight = kFuse || kGate;  // projects ur = u - bf / z
    __shared__ double s_u[kPsChunk], s_v[kPsChunk], s_eu[kPsChunk], s_ev[kPsChunk], s_r[kPsChunk];
    __shared__ double s_ur[kPsChunk], s_eur[kPsChunk];  // referenced, and so allocated, where kRight only
    __shared__ int16_t s_x0[kPsChunk], s_x1[kPsChunk], s_y0[kPsChunk], s_y1[kPsChunk], s_lvl[kPsChunk];
    __shared__ uint8_t s_st[kPsChunk];
    const int tid = threadIdx.x;
    // the workgroup's keyframe, its first item and the end of its item range: (keyframe, chunk of the shared
    // points) of a 2-D grid, or in the ragged kernels the chunk table's (search, first item) and the search's target
    [[maybe_unused]] int srch = 0;
    int k;
    int64_t first, n_end;
    if constexpr (kRagged) {
        srch = (int)sx.chunk[2 * (int64_t)blockIdx.x];
        first = sx.chunk[2 * (int64_t)blockIdx.x + 1];
        n_end = sx.off[srch + 1];
        k = sx.kf[srch];
    } else {
        k = blockIdx.y;
        first = (int64_t)blockIdx.x * kPsChunk;
        n_end = pt.n;
    }
    const double* K = kf.f64 + (int64_t)k * kPsKfF64;
    const int cols = kf.i32[3 * k], rows = kf.i32[3 * k + 1], levels = kf.i32[3 * k + 2];
    const double* scale = kf.scale + kf.lvl_off[k];
    // ---- phase 1: one point per thread
    {
        int lvl = -1, x0 = 0, x1 = -1, y0 = 0, y1 = -1;
        unsigned st = 0;
        double u = 0.0, v = 0.0, Eu = 0.0, Ev = 0.0, r = 0.0;
        [[maybe_unused]] double ur = 0.0, Eur = 0.0;
        const int64_t i = first + tid;
        if (i < n_end) {
            const double* P;
            if constexpr (kRagged)
                P = pt.f64 + (int64_t)sx.item_pt[i] * kPsPtF64;
            else
                P = pt.f64 + i * kPsPtF64;
            // k_sim3_search: the intrinsics are the search's (pKF1's in both directions), not the target's
            [[maybe_unused]] const double* S = nullptr;
            if constexpr (kSim3) S = sx.f64 + (int64_t)srch * kPsSim3F64;
            const double* I = kSim3 ? S : K;
            const double fx = I[0], fy = I[1], cx = I[2], cy = I[3];
            [[maybe_unused]] const double bf = kRight ? K[4] : 0.0;  // the others do not read the slot
            const double minX = K[20], maxX = K[21], minY = K[22], maxY = K[23], winv = K[24], hinv = K[25],
                         lsf = K[26];
            const double p0 = P[0], p1 = P[1], p2 = P[2];
            double xc, yc, zc, Ex, Ey, Ez;
            if constexpr (kSim3) {
                // two stages with a rounding in between, as the reference: c1 = Rw p + tw, then c = sR c1 + t
                const double *Rw = S + 4, *tw = S + 13, *sR = S + 16, *t = S + 25;
                const double c0 = ((Rw[0] * p0 + Rw[1] * p1) + Rw[2] * p2) + tw[0];
                const double c1 = ((Rw[3] * p0 + Rw[4] * p1) + Rw[5] * p2) + tw[1];
                const double c2 = ((Rw[6] * p0 + Rw[7] * p1) + Rw[8] * p2) + tw[2];
                const double E0 = 4.0 * eps * (((fabs(Rw[0] * p0) + fabs(Rw[1] * p1)) + fabs(Rw[2] * p2)) + fabs(tw[0]));
                const double E1 = 4.0 * eps * (((fabs(Rw[3] * p0) + fabs(Rw[4] * p1)) + fabs(Rw[5] * p2)) + fabs(tw[1]));
                const double E2 = 4.0 * eps * (((fabs(Rw[6] * p0) + fabs(Rw[7] * p1)) + fabs(Rw[8] * p2)) + fabs(tw[2]));
                xc = ((sR[0] * c0 + sR[1] * c1) + sR[2] * c2) + t[0];
                yc = ((sR[3] * c0 + sR[4] * c1) + sR[5] * c2) + t[1];
                zc = ((sR[6] * c0 + sR[7] * c1) + sR[8] * c2) + t[2];
                Ex = ((fabs(sR[0]) * E0 + fabs(sR[1]) * E1) + fabs(sR[2]) * E2) +
                     4.0 * eps * (((fabs(sR[0] * c0) + fabs(sR[1] * c1)) + fabs(sR[2] * c2)) + fabs(t[0]));
                Ey = ((fabs(sR[3]) * E0 + fabs(sR[4]) * E1) + fabs(sR[5]) * E2) +
                     4.0 * eps * (((fabs(sR[3] * c0) + fabs(sR[4] * c1)) + fabs(sR[5] * c2)) + fabs(t[1]));
                Ez = ((fabs(sR[6]) * E0 + fabs(sR[7]) * E1) + fabs(sR[8]) * E2) +
                     4.0 * eps * (((fabs(sR[6] * c0) + fabs(sR[7] * c1)) + fabs(sR[8] * c2)) + fabs(t[2]));
            } else {
                xc = ((K[5] * p0 + K[6] * p1) + K[7] * p2) + K[14];
                yc = ((K[8] * p0 + K[9] * p1) + K[10] * p2) + K[15];
                zc = ((K[11] * p0 + K[12] * p1) + K[13] * p2) + K[16];
                Ex = 4.0 * eps * (((fabs(K[5] * p0) + fabs(K[6] * p1)) + fabs(K[7] * p2)) + fabs(K[14]));
                Ey = 4.0 * eps * (((fabs(K[8] * p0) + fabs(K[9] * p1)) + fabs(K[10] * p2)) + fabs(K[15]));
                Ez = 4.0 * eps * (((fabs(K[11] * p0) + fabs(K[12] * p1)) + fabs(K[13] * p2)) + fabs(K[16]));
            }
            do {
                if constexpr (kSim3) {
                    // the camera coordinates are themselves rounded products of finite inputs: an overflow in
                    // either stage decides nothing
                    if (!isfinite(((xc + yc) + zc) + ((Ex + Ey) + Ez))) {
                        st = ORBFE_FUSE_MARGINAL;
                        break;
                    }
                }
                if constexpr (kDepthFree) {
                    // no depth gate: the sign of zc decides nothing, but within its bound of 0 nothing after it is
                    // known, and at zc == 0 the reference divides by zero; the caller's redo follows it there
                    if (zc == 0.0 || fabs(zc) < Ez) {
                        st = ORBFE_FUSE_MARGINAL;
                        break;
                    }
                } else if (zc < 0.0) {
                    if (-zc < Ez) st = ORBFE_FUSE_MARGINAL;
                    break;
                }
                // zc == 0 runs on: 1 / 0 is inf, u and v end as inf or NaN and fail the image test below (the ckf
                // search leaves at its z <= 0; neither way reaches a window)
                const double iz = 1.0 / zc;
                // k_fkf_search multiplies in the reference's order there, (fx * xc) * iz: xn, yn are then fx * xc and
                // fy * yc, and fxx, fyy again the products the principal point is added to
                const double xn = kFkf ? fx * xc : xc * iz, yn = kFkf ? fy * yc : yc * iz;
                const double fxx = kFkf ? xn * iz : fx * xn, fyy = kFkf ? yn * iz : fy * yn;
                u = fxx + cx;
                v = fyy + cy;
                [[maybe_unused]] double bz = 0.0;
                if constexpr (kRight) {
                    bz = bf * iz;
                    ur = u - bz;
                }
                // Frame's bounds are inclusive at both ends
                const bool in = kFkf ? !(u < minX || u > maxX || v < minY || v > maxY)
                                     : minX <= u && u < maxX && minY <= v && v < maxY;
                if constexpr (!kDepthFree) {
                    if (zc < Ez) st = ORBFE_FUSE_MARGINAL;
                    // k_local_search: the reference's NaN comparisons may let the point through its bounds
                    if constexpr (kGate)
                        if (zc == 0.0) st = ORBFE_FUSE_MARGINAL;
                    if (zc == 0.0) break;  // not in the image (in is false), whatever xc and yc are
                }
                const double rz = Ez / (kFkf ? fabs(zc) : zc);
                if (!(rz <= 0.25)) st = ORBFE_FUSE_MARGINAL;
                const double aiz = kFkf ? fabs(iz) : iz;
                const double Eiz = aiz * (2.0 * rz + 2.0 * eps);
                const double Ax = kFkf ? fabs(fx) * Ex : fabs(xc) * Eiz + Ex * (iz + Eiz),
                             Ay = kFkf ? fabs(fy) * Ey : fabs(yc) * Eiz + Ey * (iz + Eiz);
                const double Exn = Ax + eps * (fabs(xn) + Ax), Eyn = Ay + eps * (fabs(yn) + Ay);
                const double Mu = fabs(fxx) + fabs(cx), Mv = fabs(fyy) + fabs(cy);
                if constexpr (kFkf) {
                    const double Bx = fabs(xn) * Eiz + Exn * (aiz + Eiz), By = fabs(yn) * Eiz + Eyn * (aiz + Eiz);
                    Eu = (Bx + eps * (fabs(fxx) + Bx)) + 4.0 * eps * Mu;
                    Ev = (By + eps * (fabs(fyy) + By)) + 4.0 * eps * Mv;
                } else {
                    Eu = fabs(fx) * Exn + 4.0 * eps * Mu;
                    Ev = fabs(fy) * Eyn + 4.0 * eps * Mv;
                }
                double sum;  // finite when everything phase 2 reads is
                if constexpr (!kRight) {
                    sum = ((u + v) + Eu) + Ev;
                } else {
                    Eur = (Eu + fabs(bf) * Eiz) + 4.0 * eps * (fabs(bz) + Mu);
                    sum = ((((u + v) + ur) + Eu) + Ev) + Eur;
                }
                if (!isfinite(sum)) {
                    st = ORBFE_FUSE_MARGINAL;
                    break;
                }
                if (fabs(u - minX) < Eu + eps * fabs(minX) || fabs(u - maxX) < Eu + eps * fabs(maxX) ||
                    fabs(v - minY) < Ev + eps * fabs(minY) || fabs(v - maxY) < Ev + eps * fabs(maxY))
                    st = ORBFE_FUSE_MARGINAL;
                if (!in) break;
                if constexpr (kFf) {
                    // no gate on the point and no prediction: the level is the item's own, th the search's.  The
                    // window below is the Frame window further down, statement for statement: sharing it through a
                    // nested block or a lambda changes the register allocation of the other five kernels
                    const int level = ff.item_level[i];
                    r = sx.f64[srch] * scale[level];
                    const double ax = ((u - minX) - r) * winv, bx = ((u - minX) + r) * winv;
                    const double ay = ((v - minY) - r) * hinv, by = ((v - minY) + r) * hinv;
                    if (!isfinite((ax + bx) + (ay + by))) {
                        st = ORBFE_FUSE_MARGINAL;
                        break;
                    }
                    const double Ewx = fabs(winv) * (Eu + 4.0 * eps * ((fabs(u) + fabs(minX)) + fabs(r)));
                    const double Ewy = fabs(hinv) * (Ev + 4.0 * eps * ((fabs(v) + fabs(minY)) + fabs(r)));
                    if ((fabs(ax) > 0.5 && near_int(ax, Ewx)) || (fabs(bx) > 0.5 && near_int(bx, Ewx)) ||
                        (fabs(ay) > 0.5 && near_int(ay, Ewy)) || (fabs(by) > 0.5 && near_int(by, Ewy)))
                        st = ORBFE_FUSE_MARGINAL;
                    const double tax = trunc(ax), tbx = trunc(bx), tay = trunc(ay), tby = trunc(by);
                    if (tax >= (double)cols || tbx < 0.0 || tay >= (double)rows || tby < 0.0) break;
                    x0 = tax < 0.0 ? 0 : (int)tax;
                    x1 = tbx > (double)(cols - 1) ? cols - 1 : (int)tbx;
                    y0 = tay < 0.0 ? 0 : (int)tay;
                    y1 = tby > (double)(rows - 1) ? rows - 1 : (int)tby;
                    lvl = level;
                    break;
                }
                [[maybe_unused]] double po0 = 0.0, po1 = 0.0, po2 = 0.0;
                double dist, Ed;
                if constexpr (kSim3) {
                    // the norm of the target camera's coordinates, so the Sim3's scale moves the level.  Its
                    // operands are rounded sums of unknown cancellation: the norm moves by at most the length of
                    // what moves them
                    dist = sqrt((xc * xc + yc * yc) + zc * zc);
                    Ed = ((Ex + Ey) + Ez) + 6.0 * eps * dist;
                } else {
                    po0 = p0 - K[17];
                    po1 = p1 - K[18];
                    po2 = p2 - K[19];
                    dist = sqrt((po0 * po0 + po1 * po1) + po2 * po2);
                    Ed = 6.0 * eps * dist;
                }
                const double minD = P[6], maxD = P[7];
                if (!isfinite(dist)) {
                    st = ORBFE_FUSE_MARGINAL;
                    break;
                }
                if (fabs(dist - minD) < Ed + eps * fabs(minD) || fabs(dist - maxD) < Ed + eps * fabs(maxD))
                    st = ORBFE_FUSE_MARGINAL;
                if (dist < minD || dist > maxD) break;
                [[maybe_unused]] double vc = 0.0;
                if constexpr (kLocal) {
                    // the cosine itself is compared, with the search's limit and with 0.998 for the radius
                    const double t0 = po0 * P[3], t1 = po1 * P[4], t2 = po2 * P[5];
                    const double dot = (t0 + t1) + t2;
                    vc = dot / dist;
                    const double lim = sx.f64[srch];
                    const double Evc = 5.0 * eps * ((fabs(t0) + fabs(t1)) + fabs(t2)) / dist + 8.0 * eps * fabs(vc);
                    if (!isfinite(vc + Evc)) {
                        st = ORBFE_FUSE_MARGINAL;
                        break;
                    }
                    if (fabs(vc - lim) < Evc + eps * fabs(lim) || fabs(vc - 0.998) < Evc + eps * 0.998)
                        st = ORBFE_FUSE_MARGINAL;
                    if (vc < lim) break;
                } else if constexpr (!kSim3 && !kFkf) {  // the others have no viewing gate and do not read the normal
                    const double t0 = po0 * P[3], t1 = po1 * P[4], t2 = po2 * P[5];
                    const double dot = (t0 + t1) + t2;
                    const double half = 0.5 * dist;
                    if (fabs(dot - half) < 5.0 * eps * ((fabs(t0) + fabs(t1)) + fabs(t2)) + Ed)
                        st = ORBFE_FUSE_MARGINAL;
                    if (dot < half) break;
                }
                const double q = log(P[8] / dist) / lsf;
                if (!isfinite(q)) {
                    st = ORBFE_FUSE_MARGINAL;
                    break;
                }
                if constexpr (kSim3) {
                    // dist is off by up to rd of itself, and |log(1 - rd)| <= 1.5 rd for rd <= 0.25
                    const double rd = Ed / dist;
                    if (!(rd <= 0.25)) st = ORBFE_FUSE_MARGINAL;
                    if (near_int(q, (1.5 * rd + 4.0 * eps) / fabs(lsf) + 4.0 * eps * fabs(q))) st = ORBFE_FUSE_MARGINAL;
                } else {
                    if (near_int(q, 10.0 * eps / fabs(lsf) + 4.0 * eps * fabs(q))) st = ORBFE_FUSE_MARGINAL;
                }
                const double cq = ceil(q);
                const int level = cq < 0.0 ? 0 : (cq > (double)(levels - 1) ? levels - 1 : (int)cq);
                if constexpr (kLocal) {
                    // in view from here on, whatever becomes of the window
                    lvl = level;
                    double r0 = vc > 0.998 ? 2.5 : 4.0;
                    if (th_on) r0 *= th;  // th == 1 multiplies nothing, as in the reference
                    r = r0 * scale[level];
                } else {
                    r = th * scale[level];
                }
                const double ax = ((u - minX) - r) * winv, bx = ((u - minX) + r) * winv;
                const double ay = ((v - minY) - r) * hinv, by = ((v - minY) + r) * hinv;
                if (!isfinite((ax + bx) + (ay + by))) {
                    st = ORBFE_FUSE_MARGINAL;
                    break;
                }
                const double Ewx = fabs(winv) * (Eu + 4.0 * eps * ((fabs(u) + fabs(minX)) + fabs(r)));
                const double Ewy = fabs(hinv) * (Ev + 4.0 * eps * ((fabs(v) + fabs(minY)) + fabs(r)));
                if constexpr (kFkf) {
                    // int() truncates toward zero at both ends: (-1, 1) is cell 0, so only an integer of magnitude
                    // >= 1 separates two outcomes (max(0, .) hides the negative ones of a lower end, harmlessly
                    // marked here)
                    if ((fabs(ax) > 0.5 && near_int(ax, Ewx)) || (fabs(bx) > 0.5 && near_int(bx, Ewx)) ||
                        (fabs(ay) > 0.5 && near_int(ay, Ewy)) || (fabs(by) > 0.5 && near_int(by, Ewy)))
                        st = ORBFE_FUSE_MARGINAL;
                    const double tax = trunc(ax), tbx = trunc(bx), tay = trunc(ay), tby = trunc(by);
                    // the four early returns of Frame.get_features_in_area
                    if (tax >= (double)cols || tbx < 0.0 || tay >= (double)rows || tby < 0.0) break;
                    x0 = tax < 0.0 ? 0 : (int)tax;
                    x1 = tbx > (double)(cols - 1) ? cols - 1 : (int)tbx;
                    y0 = tay < 0.0 ? 0 : (int)tay;
                    y1 = tby > (double)(rows - 1) ? rows - 1 : (int)tby;
                    lvl = level;
                    break;
                }
                if (near_int(ax, Ewx) || near_int(bx, Ewx) || near_int(ay, Ewy) || near_int(by, Ewy))
                    st = ORBFE_FUSE_MARGINAL;
                const double fax = floor(ax), cbx = ceil(bx), fay = floor(ay), cby = ceil(by);
                // the four early returns of get_features_in_area
                if (fax >= (double)cols || cbx < 0.0 || fay >= (double)rows || cby < 0.0) break;
                x0 = fax < 0.0 ? 0 : (int)fax;
                x1 = cbx > (double)(cols - 1) ? cols - 1 : (int)cbx;
                y0 = fay < 0.0 ? 0 : (int)fay;
                y1 = cby > (double)(rows - 1) ? rows - 1 : (int)cby;
                lvl = level;
            } while (false);
        }
        s_u[tid] = u;
        s_v[tid] = v;
        s_eu[tid] = Eu;
        s_ev[tid] = Ev;
        if constexpr (kRight) {
            s_ur[tid] = ur;
            s_eur[tid] = Eur;
        }
        s_r[tid] = r;
        s_x0[tid] = (int16_t)x0;
        s_x1[tid] = (int16_t)x1;
        s_y0[tid] = (int16_t)y0;
        s_y1[tid] = (int16_t)y1;
        s_lvl[tid] = (int16_t)lvl;
        s_st[tid] = (uint8_t)st;
    }
    __syncthreads();
    // ---- phase 2: kPsGroup lanes per point
    const int g = tid / kPsGroup, l = tid % kPsGroup;
    const int64_t base = kf.off[k];
    const double* xy = kf.xy + 2 * base;
    const int32_t* oct = kf.octave + base;
    const uint4* desc = reinterpret_cast<const uint4*>(kf.desc + base * 32);
    const int32_t* coff = kf.cell_off + kf.cell_at[k];
    const int32_t* cidx = kf.cell_idx + kf.idx_at[k];
    [[maybe_unused]] const double *uright = nullptr, *is2 = nullptr;
    [[maybe_unused]] const uint8_t* blk = nullptr;
    if constexpr (kBlocked) {
        blk = kf.blocked ? kf.blocked + base : nullptr;
        if constexpr (kGate) uright = kf.u_right + base;
    } else if constexpr (kFuse) {
        uright = kf.u_right + base;
        is2 = kf.inv_sigma2 + kf.lvl_off[k];
    }
    for (int j = g; j < kPsChunk; j += kPsChunk / kPsGroup) {
        const int64_t i = first + j;
        if (i >= n_end) break;
        const int level = s_lvl[j];
        unsigned st = s_st[j];
        unsigned key = kPsNone;
        [[maybe_unused]] unsigned key2 = kPsNone;  // k_local_search: the second smallest key
        if (level >= 0) {
            const double u = s_u[j], v = s_v[j], Eu = s_eu[j], Ev = s_ev[j], r = s_r[j];
            [[maybe_unused]] double ur = 0.0, Eur = 0.0;
            if constexpr (kRight) {
                ur = s_ur[j];
                Eur = s_eur[j];
            }
            const int x0 = s_x0[j], x1 = s_x1[j], y0 = s_y0[j], y1 = s_y1[j];
            const uint4* pd;
            if constexpr (kRagged)
                pd = reinterpret_cast<const uint4*>(pt.desc + (int64_t)sx.item_pt[i] * 32);
            else
                pd = reinterpret_cast<const uint4*>(pt.desc + i * 32);
            const uint4 qa = pd[0], qb = pd[1];
            const double er_r = eps * fabs(r);
            [[maybe_unused]] int olo = 0, ohi = 0;  // k_ff_search: the search's octave range around the item's level
            if constexpr (kFf) {
                const int md = ff.mode[srch];
                olo = md == 1 ? level : (md == 2 ? 0 : level - 1);
                ohi = md == 1 ? 0x7FFFFFFF : (md == 2 ? level : level + 1);
            }
            for (int ix = x0; ix <= x1; ++ix) {
                const int a = coff[ix * rows + y0], b = coff[ix * rows + y1 + 1];
                for (int pos = a + l; pos < b; pos += kPsGroup) {
                    const int f = cidx[pos];
                    if constexpr (kBlocked)
                        if (blk && blk[f]) continue;
                    const double kx = xy[2 * f], ky = xy[2 * f + 1];
                    const double dx = kx - u, dy = ky - v;
                    const double Edx = Eu + 2.0 * eps * (fabs(kx) + fabs(u)), Edy = Ev + 2.0 * eps * (fabs(ky) + fabs(v));
                    if (fabs(fabs(dx) - r) < Edx + er_r || fabs(fabs(dy) - r) < Edy + er_r) st = ORBFE_FUSE_MARGINAL;
                    if (!(fabs(dx) < r && fabs(dy) < r)) continue;
                    const int o = oct[f];
                    if constexpr (kFf) {
                        if (o < olo || o > ohi) continue;
                    } else {
                        if (o < level - 1 || o > level + (kFkf && !kLocal ? 1 : 0)) continue;
                    }
                    if constexpr (kFuse) {
                        const double kr = uright[f];
                        const double ex = u - kx, ey = v - ky;
                        const double bxy = (2.0 * fabs(ex) * Edx + Edx * Edx) + (2.0 * fabs(ey) * Edy + Edy * Edy);
                        double e2, B, T;
                        if (kr >= 0.0) {
                            const double er = ur - kr;
                            const double Eer = Eur + 2.0 * eps * (fabs(kr) + fabs(ur));
                            e2 = (ex * ex + ey * ey) + er * er;
                            B = bxy + (2.0 * fabs(er) * Eer + Eer * Eer);
                            T = 7.8;
                        } else {
                            e2 = ex * ex + ey * ey;
                            B = bxy;
                            T = 5.99;
                        }
                        const double chi = e2 * is2[o];
                        const double Echi = fabs(is2[o]) * B + 6.0 * eps * fabs(chi);
                        if (!(fabs(chi - T) >= Echi + eps * T)) st = ORBFE_FUSE_MARGINAL;  // a NaN marks too
                        if (chi > T) continue;
                    }
                    if constexpr (kGate) {
                        // the per-candidate stereo gate: |ur - uR| > r leaves a feature with a right coordinate out
                        const double kr = uright[f];
                        if (kr > 0.0) {
                            const double er = fabs(ur - kr);
                            const double Eer = Eur + 2.0 * eps * (fabs(kr) + fabs(ur));
                            if (fabs(er - r) < Eer + er_r) st = ORBFE_FUSE_MARGINAL;
                            if (er > r) continue;
                        }
                    }
                    const unsigned d = hamming256(desc[2 * f], desc[2 * f + 1], qa, qb);
                    const unsigned c = (d << 16) | (unsigned)pos;
                    if constexpr (kLocal) {
                        // positions differ, so keys do: the lane holds the two smallest of what it has seen
                        key2 = min(key2, max(key, c));
                    }
                    key = min(key, c);
                }
            }
#pragma unroll
            for (int o = kPsGroup / 2; o; o >>= 1) {
                const unsigned ok = (unsigned)__shfl_xor((int)key, o, kPsGroup);
                if constexpr (kLocal) {
                    // the two smallest of two disjoint sets, each given by its two smallest
                    const unsigned ok2 = (unsigned)__shfl_xor((int)key2, o, kPsGroup);
                    key2 = min(max(key, ok), min(key2, ok2));
                }
                key = min(key, ok);
                st |= (unsigned)__shfl_xor((int)st, o, kPsGroup);
            }
        }
        if (l == 0) {
            const int64_t at = kRagged ? i : (int64_t)k * out.stride + i;
            out.best_idx[at] = key == kPsNone ? -1 : cidx[key & 0xFFFFu];
            out.best_dist[at] = key == kPsNone ? -1 : (int)(key >> 16);
            out.status[at] = (uint8_t)st;
            if constexpr (kLocal) {
                out.second_idx[at] = key2 == kPsNone ? -1 : cidx[key2 & 0xFFFFu];
                out.second_dist[at] = key2 == kPsNone ? -1 : (int)(key2 >> 16);
                out.level[at] = level;
                out.in_view[at] = level >= 0;
            }
        }
    }
}

__global__ __launch_bounds__(kPsChunk) void k_fuse_search(PsKfs kf, PsPts pt, double th, double eps, PsOut out) {
    proj_search<kPsFuse>(kf, pt, th, eps, out, PsSim3{});
}

__global__ __launch_bounds__(kPsChunk) void k_scw_search(PsKfs kf, PsPts pt, double th, double eps, PsOut out) {
    proj_search<kPsScw>(kf, pt, th, eps, out, PsSim3{});
}

// a 1-D grid over the chunk table: a workgroup is up to kPsChunk items of one search
__global__ __launch_bounds__(kPsChunk) void k_sim3_search(PsKfs kf, PsPts pt, double th, double eps, PsOut out,
                                                          PsSim3 sx) {
    proj_search<kPsSim3>(kf, pt, th, eps, out, sx);
}

// the same grid; sx.f64 is null: the pose and the intrinsics are the target frame's block
__global__ __launch_bounds__(kPsChunk) void k_fkf_search(PsKfs kf, PsPts pt, double th, double eps, PsOut out,
                                                         PsSim3 sx) {
    proj_search<kPsFkf>(kf, pt, th, eps, out, sx);
}

// the same grid; sx.f64 holds one double per search, the viewing cosine's limit; th multiplies the radius only
// where th_on is set
__global__ __launch_bounds__(kPsChunk) void k_local_search(PsKfs kf, PsPts pt, double th, double eps, PsOut out,
                                                           PsSim3 sx, int th_on) {
    proj_search<kPsLocal>(kf, pt, th, eps, out, sx, th_on);
}

// the same grid; sx.f64 holds one double per search, its th; ff the searches' octave modes and the items' levels
__global__ __launch_bounds__(kPsChunk) void k_ff_search(PsKfs kf, PsPts pt, double eps, PsOut out, PsSim3 sx,
                                                        PsFf ff) {
    proj_search<kPsFf>(kf, pt, 0.0, eps, out, sx, 0, ff);
}

}  // namespace orbfe

namespace {

// scratch of one entry: process-wide, created on first use and never torn down (the HIP runtime may already be gone
// when static destructors run); callers of that entry on several threads take turns.  Each entry has an instance of
// its own, so they do not wait for each other and each last_ms is its own entry's.
struct Searcher {
    std::mutex mu;
    DevBuf<uint8_t> d_u8;   // keyframe descriptors, point descriptors, blocked bytes, status
    DevBuf<double> d_f64;   // keyframe scalars, xy, u_right, scale, inv_sigma2, point scalars, search scalars
    DevBuf<int64_t> d_i64;  // off, cell_at, idx_at, lvl_off, srch_off, chunk table
    DevBuf<int32_t> d_i32;  // keyframe ints, octave, cell_off, cell_idx, srch_kf, item_pt, (item_level, srch_mode,)
                            // best_idx, best_dist
    std::vector<int32_t> h_i32;
    std::vector<uint8_t> h_st;
    std::vector<int64_t> h_chunk;  // k_sim3_search, k_fkf_search: (search, first item) per workgroup
    TimedStream t;
};
template <PsMode kMode>
Searcher& searcher() {
    static Searcher* m = new Searcher;
    return *m;
}

std::string at_kf(int32_t k, const std::string& what) { return "keyframe " + std::to_string(k) + ": " + what; }

// what orbfe_sim3_search and orbfe_fkf_search have besides the keyframes and the point table
struct Sim3In {
    const double* f64;  // orbfe_fkf_search: null; orbfe_local_search: the viewing cosine's limit per search;
                        // orbfe_ff_search: th per search
    const int32_t* kf;
    const int64_t* off;
    int32_t n;
    const int32_t* item_pt;
    int th_on = 0;  // orbfe_local_search only
    // orbfe_ff_search only
    const int32_t* mode = nullptr;
    const int32_t* item_level = nullptr;
};

// All six entries: validate, stage, launch, download.  kPsLocal is kPsFkf with u_right, slot 4 and the normal read,
// one scalar per search and four more outputs.  kPsFf is kPsLocal without those outputs, with th as the search's
// scalar (the argument th is not looked at), a mode per search and a level per item, and slots 3-8 of a point's
// scalars free to hold anything.  Otherwise, not kPsFuse: u_right and inv_sigma2 are not looked at and
// slot 4 of a keyframe's scalars may hold anything.  kPsScw, kPsFkf: blocked may be null (nothing is blocked);
// otherwise blocked is not looked at.  kPsSim3, kPsFkf: sx is the searches, slots 3-5 of a point's scalars may hold
// anything, out_stride is not looked at and the outputs are flat over the items; kPsSim3 alone has search scalars and
// lets slots 0-19 of a keyframe's scalars hold anything.  Out is the entry's orbfe_*_out.
template <PsMode kMode, class Out>
void search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy, const int32_t* octave,
            const double* u_right, const uint8_t* desc32, const uint8_t* blocked, const int64_t* cell_at,
            const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
            const double* scale, const double* inv_sigma2, int32_t n_kf, const double* pt_f64,
            const uint8_t* pt_desc32, int64_t n_pts, double th, double eps, const Out* out, int64_t out_stride,
            [[maybe_unused]] const Sim3In* sx = nullptr) {
    constexpr bool kFuse = kMode == kPsFuse, kScw = kMode != kPsFuse, kSim3 = kMode == kPsSim3;
    constexpr bool kLocal = kMode == kPsLocal, kFf = kMode == kPsFf;
    constexpr bool kRight = kFuse || kLocal || kFf;  // u_right and slot 4 (bf) are read
    constexpr bool kRagged = kSim3 || kMode == kPsFkf || kLocal || kFf;
    constexpr bool kBlocked = kMode == kPsScw || kMode == kPsFkf || kLocal || kFf;
    constexpr size_t kOutI32 = kLocal ? 5 : 2, kOutU8 = kLocal ? 2 : 1;  // output arrays per item
    if (n_kf < 0 || n_pts < 0 || out_stride < 0) throw Error(ORBFE_EINVAL, "bad argument");
    if (n_kf > 65535) throw Error(ORBFE_EINVAL, "more than 65535 keyframes in one call");
    if (!std::isfinite(th) || !std::isfinite(eps) || eps < 0.0)
        throw Error(ORBFE_EINVAL, "th and eps must be finite and eps not negative");
    int64_t n_items = 0;
    if constexpr (kRagged) {
        if (sx->n < 0) throw Error(ORBFE_EINVAL, "bad argument");
        if (sx->n == 0) return;
        if (!sx->off) throw Error(ORBFE_EINVAL, "null argument");
        if (sx->off[0] != 0) throw Error(ORBFE_EINVAL, "srch_off[0] must be 0");
        for (int32_t q = 0; q < sx->n; ++q)
            if (sx->off[q + 1] < sx->off[q])
                throw Error(ORBFE_EINVAL, "search " + std::to_string(q) + ": srch_off must not decrease");
        n_items = sx->off[sx->n];
        if (n_items == 0) return;
        if (((kSim3 || kLocal || kFf) && !sx->f64) || !sx->kf || !sx->item_pt ||
            (kFf && (!sx->mode || !sx->item_level)))
            throw Error(ORBFE_EINVAL, "null argument");
        for (int32_t q = 0; q < sx->n; ++q) {
            if (sx->kf[q] < 0 || sx->kf[q] >= n_kf)
                throw Error(ORBFE_EINVAL, "search " + std::to_string(q) + ": the target is outside the keyframes");
            if (kSim3 && !all_finite(sx->f64 + (int64_t)q * ORBFE_SIM3_F64, ORBFE_SIM3_F64))
                throw Error(ORBFE_EINVAL, "search " + std::to_string(q) + ": a scalar is not finite");
            if (kLocal && !std::isfinite(sx->f64[q]))
                throw Error(ORBFE_EINVAL, "search " + std::to_string(q) + ": the viewing cosine's limit is not finite");
            if (kFf && !std::isfinite(sx->f64[q]))
                throw Error(ORBFE_EINVAL, "search " + std::to_string(q) + ": th is not finite");
            if (kFf && (sx->mode[q] < 0 || sx->mode[q] > 2))
                throw Error(ORBFE_EINVAL, "search " + std::to_string(q) + ": the mode is outside 0..2");
        }
        for (int64_t i = 0; i < n_items; ++i)
            if (sx->item_pt[i] < 0 || sx->item_pt[i] >= n_pts)
                throw Error(ORBFE_EINVAL, "an item is outside the point table");
    } else {
        if (n_kf == 0 || n_pts == 0) return;
    }
    if (!kf_f64 || !kf_i32 || !off || !cell_at || !idx_at || !lvl_off || !cell_off || !scale ||
        (!kScw && !inv_sigma2) || !pt_f64 || !pt_desc32 || !out || !out->best_idx || !out->best_dist || !out->status)
        throw Error(ORBFE_EINVAL, "null argument");
    if constexpr (kLocal)
        if (!out->in_view || !out->level || !out->second_idx || !out->second_dist)
            throw Error(ORBFE_EINVAL, "null argument");
    if (!kRagged && out_stride < n_pts) throw Error(ORBFE_EINVAL, "out_stride is below the point count");
    if (off[0] != 0 || cell_at[0] != 0 || idx_at[0] != 0 || lvl_off[0] != 0)
        throw Error(ORBFE_EINVAL, "off[0], cell_at[0], idx_at[0] and lvl_off[0] must be 0");
    for (int32_t k = 0; k < n_kf; ++k)
        if (off[k + 1] < off[k] || cell_at[k + 1] < cell_at[k] || idx_at[k + 1] < idx_at[k] ||
            lvl_off[k + 1] < lvl_off[k])
            throw Error(ORBFE_EINVAL, at_kf(k, "offsets must not decrease"));
    for (int32_t k = 0; k < n_kf; ++k) {
        const int64_t n = off[k + 1] - off[k], nc = cell_at[k + 1] - cell_at[k], ni = idx_at[k + 1] - idx_at[k],
                      nl = lvl_off[k + 1] - lvl_off[k];
        if (n > ORBFE_BOW_MAX_FRAME || ni > ORBFE_BOW_MAX_FRAME)
            throw Error(ORBFE_EINVAL, at_kf(k, "more features or grid entries than the limit of " +
                                                   std::to_string(ORBFE_BOW_MAX_FRAME) + " per keyframe"));
        // slot 4 is bf, which only k_fuse_search reads; k_sim3_search reads none of the slots before the bounds
        const double* Kk = kf_f64 + (int64_t)k * ORBFE_FUSE_KF_F64;
        if (!((kSim3 || (all_finite(Kk, 4) && (!kRight || std::isfinite(Kk[4])) && all_finite(Kk + 5, 15))) &&
              all_finite(Kk + 20, ORBFE_FUSE_KF_F64 - 20)))
            throw Error(ORBFE_EINVAL, at_kf(k, "a scalar is not finite"));
        const int64_t cols = kf_i32[3 * k], rows = kf_i32[3 * k + 1], levels = kf_i32[3 * k + 2];
        if (levels <= 0) throw Error(ORBFE_EINVAL, at_kf(k, "the level count must be positive"));
        if (nl != levels) throw Error(ORBFE_EINVAL, at_kf(k, "the level table does not have one entry per level"));
        if (cols <= 0 || rows <= 0 || cols > 4096 || rows > 4096)
            throw Error(ORBFE_EINVAL, at_kf(k, "grid columns and rows must lie in [1, 4096]"));
        if (nc != cols * rows + 1) throw Error(ORBFE_EINVAL, at_kf(k, "the grid needs columns * rows + 1 cell offsets"));
        if (!(all_finite(scale + lvl_off[k], nl) && (kScw || all_finite(inv_sigma2 + lvl_off[k], nl))))
            throw Error(ORBFE_EINVAL, at_kf(k, "a level table entry is not finite"));
        if (n > 0 && (!xy || !octave || (kRight && !u_right) || !desc32)) throw Error(ORBFE_EINVAL, "null argument");
        if (n > 0 && !(all_finite(xy + 2 * off[k], 2 * n) && (!kRight || all_finite(u_right + off[k], n))))
            throw Error(ORBFE_EINVAL, at_kf(k, "a keypoint coordinate is not finite"));
        for (int64_t i = 0; i < n; ++i) {
            const int32_t o = octave[off[k] + i];
            if (o < 0 || o >= levels) throw Error(ORBFE_EINVAL, at_kf(k, "an octave is outside the level table"));
        }
        const int32_t* co = cell_off + cell_at[k];
        if (co[0] != 0) throw Error(ORBFE_EINVAL, at_kf(k, "the first cell offset must be 0"));
        for (int64_t c = 0; c < nc - 1; ++c)
            if (co[c + 1] < co[c]) throw Error(ORBFE_EINVAL, at_kf(k, "cell offsets must not decrease"));
        if (co[nc - 1] != ni) throw Error(ORBFE_EINVAL, at_kf(k, "the last cell offset is not the grid entry count"));
        if (ni > 0 && !cell_idx) throw Error(ORBFE_EINVAL, "null argument");
        for (int64_t e = 0; e < ni; ++e) {
            const int32_t f = cell_idx[idx_at[k] + e];
            if (f < 0 || f >= n) throw Error(ORBFE_EINVAL, at_kf(k, "a grid entry is outside the features"));
        }
    }
    if constexpr (kFf) {
        // levels are positive here; an item's level indexes its target's scale table
        for (int32_t q = 0; q < sx->n; ++q) {
            const int32_t levels = kf_i32[3 * sx->kf[q] + 2];
            for (int64_t i = sx->off[q]; i < sx->off[q + 1]; ++i)
                if (sx->item_level[i] < 0 || sx->item_level[i] >= levels)
                    throw Error(ORBFE_EINVAL,
                                "search " + std::to_string(q) + ": an item's level is outside the target's");
        }
        for (int64_t i = 0; i < n_pts; ++i)  // only the position is read
            if (!all_finite(pt_f64 + i * ORBFE_FUSE_PT_F64, 3))
                throw Error(ORBFE_EINVAL, "a point scalar is not finite");
    } else if constexpr (kRagged && !kLocal) {
        for (int64_t i = 0; i < n_pts; ++i)  // slots 3-5, the normal, are not read
            if (!(all_finite(pt_f64 + i * ORBFE_FUSE_PT_F64, 3) && all_finite(pt_f64 + i * ORBFE_FUSE_PT_F64 + 6, 3)))
                throw Error(ORBFE_EINVAL, "a point scalar is not finite");
    } else {
        if (!all_finite(pt_f64, n_pts * ORBFE_FUSE_PT_F64)) throw Error(ORBFE_EINVAL, "a point scalar is not finite");
    }
    // the outputs: a row of out_stride per keyframe, or flat over the items
    const size_t nk = (size_t)n_kf, np = (size_t)n_pts, os = (size_t)out_stride;
    const size_t n_out = kRagged ? (size_t)n_items : nk * os;
    [[maybe_unused]] size_t ns = 0, n_chunk = 0;
    const size_t n = (size_t)off[n_kf], nc = (size_t)cell_at[n_kf], ni = (size_t)idx_at[n_kf],
                 nl = (size_t)lvl_off[n_kf];
    // what only one variant stages has no room in the other's buffers
    const size_t n_ur = kRight ? n : 0, n_is2 = kScw ? 0 : nl, n_blk = kBlocked ? pad_to(n, 16) : 0;
    const bool has_blocked = kBlocked && blocked != nullptr && n > 0;
    Searcher& m = searcher<kMode>();
    std::lock_guard<std::mutex> lk(m.mu);
    if constexpr (kRagged) {
        // no workgroup straddles two searches, and an empty search gets none
        ns = (size_t)sx->n;
        m.h_chunk.clear();
        for (int32_t q = 0; q < sx->n; ++q)
            for (int64_t i = sx->off[q]; i < sx->off[q + 1]; i += kPsChunk) {
                m.h_chunk.push_back(q);
                m.h_chunk.push_back(i);
            }
        n_chunk = m.h_chunk.size() / 2;
        if (n_chunk > 0x7FFFFFFFu) throw Error(ORBFE_EINVAL, "more items than one launch takes");
    }
    hipStream_t s = m.t.get();
    // descriptors are read as uint4: both blocks start on 16 bytes
    m.d_u8.ensure(pad_to(n * 32, 16) + pad_to(np * 32, 16) + n_blk + kOutU8 * n_out);
    m.d_f64.ensure(nk * ORBFE_FUSE_KF_F64 + 2 * n + n_ur + nl + n_is2 + np * ORBFE_FUSE_PT_F64 +
                   (kSim3 ? ns * ORBFE_SIM3_F64 : (kLocal || kFf) ? ns : 0));
    m.d_i64.ensure(4 * (nk + 1) + (kRagged ? ns + 1 + 2 * n_chunk : 0));
    m.d_i32.ensure(3 * nk + n + nc + ni + (kRagged ? ns + n_out : 0) + (kFf ? n_out + ns : 0) + kOutI32 * n_out);
    uint8_t* d_desc = m.d_u8.p;
    uint8_t* d_pdesc = d_desc + pad_to(n * 32, 16);
    uint8_t* d_blk = d_pdesc + pad_to(np * 32, 16);
    uint8_t* d_st = d_blk + n_blk;
    double* d_kf = m.d_f64.p;
    double* d_xy = d_kf + nk * ORBFE_FUSE_KF_F64;
    double* d_ur = d_xy + 2 * n;
    double* d_scale = d_ur + n_ur;
    double* d_is2 = d_scale + nl;
    double* d_pt = d_is2 + n_is2;
    [[maybe_unused]] double* d_sx = d_pt + np * ORBFE_FUSE_PT_F64;
    int64_t* d_off = m.d_i64.p;
    int64_t* d_cat = d_off + nk + 1;
    int64_t* d_iat = d_cat + nk + 1;
    int64_t* d_lvl = d_iat + nk + 1;
    [[maybe_unused]] int64_t* d_soff = d_lvl + nk + 1;
    [[maybe_unused]] int64_t* d_chunk = d_soff + ns + 1;
    int32_t* d_ki = m.d_i32.p;
    int32_t* d_oct = d_ki + 3 * nk;
    int32_t* d_coff = d_oct + n;
    int32_t* d_cidx = d_coff + nc;
    [[maybe_unused]] int32_t* d_skf = d_cidx + ni;
    [[maybe_unused]] int32_t* d_item = d_skf + ns;
    [[maybe_unused]] int32_t* d_ilvl = d_item + n_out;  // k_ff_search only, as d_mode
    [[maybe_unused]] int32_t* d_mode = d_ilvl + n_out;
    int32_t* d_bi = kFf ? d_mode + ns : (kRagged ? d_item + n_out : d_cidx + ni);
    int32_t* d_bd = d_bi + n_out;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        if (bytes) HIPCK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    };
    up(d_desc, desc32, n * 32);
    up(d_pdesc, pt_desc32, np * 32);
    if (has_blocked) up(d_blk, blocked, n);
    up(d_kf, kf_f64, nk * ORBFE_FUSE_KF_F64 * sizeof(double));
    up(d_xy, xy, 2 * n * sizeof(double));
    up(d_ur, u_right, n_ur * sizeof(double));
    up(d_scale, scale, nl * sizeof(double));
    up(d_is2, inv_sigma2, n_is2 * sizeof(double));
    up(d_pt, pt_f64, np * ORBFE_FUSE_PT_F64 * sizeof(double));
    up(d_off, off, (nk + 1) * sizeof(int64_t));
    up(d_cat, cell_at, (nk + 1) * sizeof(int64_t));
    up(d_iat, idx_at, (nk + 1) * sizeof(int64_t));
    up(d_lvl, lvl_off, (nk + 1) * sizeof(int64_t));
    up(d_ki, kf_i32, 3 * nk * sizeof(int32_t));
    up(d_oct, octave, n * sizeof(int32_t));
    up(d_coff, cell_off, nc * sizeof(int32_t));
    up(d_cidx, cell_idx, ni * sizeof(int32_t));
    [[maybe_unused]] PsSim3 dsx{};
    if constexpr (kRagged) {
        if constexpr (kSim3) up(d_sx, sx->f64, ns * ORBFE_SIM3_F64 * sizeof(double));
        if constexpr (kLocal || kFf) up(d_sx, sx->f64, ns * sizeof(double));
        if constexpr (kFf) {
            up(d_ilvl, sx->item_level, n_out * sizeof(int32_t));
            up(d_mode, sx->mode, ns * sizeof(int32_t));
        }
        up(d_soff, sx->off, (ns + 1) * sizeof(int64_t));
        up(d_chunk, m.h_chunk.data(), 2 * n_chunk * sizeof(int64_t));
        up(d_skf, sx->kf, ns * sizeof(int32_t));
        up(d_item, sx->item_pt, n_out * sizeof(int32_t));
        dsx = PsSim3{kSim3 || kLocal || kFf ? d_sx : nullptr, d_skf, d_soff, d_item, d_chunk};
    }
    PsKfs kf{};
    kf.f64 = d_kf;
    kf.i32 = d_ki;
    kf.off = d_off;
    kf.cell_at = d_cat;
    kf.idx_at = d_iat;
    kf.lvl_off = d_lvl;
    kf.xy = d_xy;
    kf.scale = d_scale;
    kf.u_right = kRight ? d_ur : nullptr;
    kf.inv_sigma2 = kScw ? nullptr : d_is2;
    kf.octave = d_oct;
    kf.cell_off = d_coff;
    kf.cell_idx = d_cidx;
    kf.desc = d_desc;
    kf.blocked = has_blocked ? d_blk : nullptr;
    const PsPts pt{d_pt, d_pdesc, n_pts};
    // k_local_search: second_idx, second_dist and level follow best_dist, in_view follows status
    const PsOut d{d_bi, d_bd, d_st, out_stride, kLocal ? d_bd + n_out : nullptr, kLocal ? d_bd + 2 * n_out : nullptr,
                  kLocal ? d_bd + 3 * n_out : nullptr, kLocal ? d_st + n_out : nullptr};
    m.t.begin(s);
    if constexpr (kFf) {
        hipLaunchKernelGGL(k_ff_search, dim3((unsigned)n_chunk), dim3(kPsChunk), 0, s, kf, pt, eps, d, dsx,
                           PsFf{d_mode, d_ilvl});
    } else if constexpr (kLocal) {
        hipLaunchKernelGGL(k_local_search, dim3((unsigned)n_chunk), dim3(kPsChunk), 0, s, kf, pt, th, eps, d, dsx,
                           sx->th_on);
    } else if constexpr (kRagged) {
        constexpr auto kernel = kSim3 ? k_sim3_search : k_fkf_search;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_chunk), dim3(kPsChunk), 0, s, kf, pt, th, eps, d, dsx);
    } else {
        const unsigned chunks = (unsigned)((np + kPsChunk - 1) / kPsChunk);
        constexpr auto kernel = kFuse ? k_fuse_search : k_scw_search;
        hipLaunchKernelGGL(kernel, dim3(chunks, (unsigned)n_kf), dim3(kPsChunk), 0, s, kf, pt, th, eps, d);
    }
    HIPCK(hipGetLastError());
    m.t.end(s);
    // the rows come back whole into staging; only the entries the kernel wrote, [0, n_pts) of each row, reach
    // the caller's arrays
    m.h_i32.resize(kOutI32 * n_out);
    m.h_st.resize(kOutU8 * n_out);
    HIPCK(hipMemcpyAsync(m.h_i32.data(), d_bi, kOutI32 * n_out * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(m.h_st.data(), d_st, kOutU8 * n_out, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    m.t.last_ms = m.t.elapsed_ms();
    if constexpr (kRagged) {  // every item was written
        std::memcpy(out->best_idx, m.h_i32.data(), n_out * sizeof(int32_t));
        std::memcpy(out->best_dist, m.h_i32.data() + n_out, n_out * sizeof(int32_t));
        std::memcpy(out->status, m.h_st.data(), n_out);
        if constexpr (kLocal) {
            std::memcpy(out->second_idx, m.h_i32.data() + 2 * n_out, n_out * sizeof(int32_t));
            std::memcpy(out->second_dist, m.h_i32.data() + 3 * n_out, n_out * sizeof(int32_t));
            std::memcpy(out->level, m.h_i32.data() + 4 * n_out, n_out * sizeof(int32_t));
            std::memcpy(out->in_view, m.h_st.data() + n_out, n_out);
        }
        return;
    }
    for (size_t k = 0; k < nk; ++k) {
        std::memcpy(out->best_idx + k * os, &m.h_i32[k * os], np * sizeof(int32_t));
        std::memcpy(out->best_dist + k * os, &m.h_i32[nk * os + k * os], np * sizeof(int32_t));
        std::memcpy(out->status + k * os, &m.h_st[k * os], np);
    }
}

template <PsMode kMode>
void last_ms(float* ms) {
    if (!ms) throw Error(ORBFE_EINVAL, "null argument");
    Searcher& m = searcher<kMode>();
    std::lock_guard<std::mutex> lk(m.mu);
    *ms = m.t.last_ms;
}

}  // namespace

extern "C" {

int orbfe_fuse_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                      const int32_t* octave, const double* u_right, const uint8_t* desc32, const int64_t* cell_at,
                      const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
                      const double* scale, const double* inv_sigma2, int32_t n_kf, const double* pt_f64,
                      const uint8_t* pt_desc32, int64_t n_pts, double th, double eps, const orbfe_fuse_out* out,
                      int64_t out_stride) {
    return guarded([&] {
        search<kPsFuse>(kf_f64, kf_i32, off, xy, octave, u_right, desc32, nullptr, cell_at, cell_off, idx_at, cell_idx,
                      lvl_off, scale, inv_sigma2, n_kf, pt_f64, pt_desc32, n_pts, th, eps, out, out_stride);
    });
}

int orbfe_fuse_search_last_ms(float* ms) {
    return guarded([&] { last_ms<kPsFuse>(ms); });
}

int orbfe_scw_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                     const int32_t* octave, const uint8_t* desc32, const uint8_t* blocked, const int64_t* cell_at,
                     const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
                     const double* scale, int32_t n_kf, const double* pt_f64, const uint8_t* pt_desc32, int64_t n_pts,
                     double th, double eps, const orbfe_scw_out* out, int64_t out_stride) {
    return guarded([&] {
        search<kPsScw>(kf_f64, kf_i32, off, xy, octave, nullptr, desc32, blocked, cell_at, cell_off, idx_at, cell_idx,
                     lvl_off, scale, nullptr, n_kf, pt_f64, pt_desc32, n_pts, th, eps, out, out_stride);
    });
}

int orbfe_scw_search_last_ms(float* ms) {
    return guarded([&] { last_ms<kPsScw>(ms); });
}

int orbfe_sim3_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                      const int32_t* octave, const uint8_t* desc32, const int64_t* cell_at, const int32_t* cell_off,
                      const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off, const double* scale,
                      int32_t n_kf, const double* pt_f64, const uint8_t* pt_desc32, int64_t n_pts,
                      const double* srch_f64, const int32_t* srch_kf, const int64_t* srch_off, int32_t n_srch,
                      const int32_t* item_pt, double th, double eps, const orbfe_sim3_out* out) {
    return guarded([&] {
        const Sim3In sx{srch_f64, srch_kf, srch_off, n_srch, item_pt};
        search<kPsSim3>(kf_f64, kf_i32, off, xy, octave, nullptr, desc32, nullptr, cell_at, cell_off, idx_at, cell_idx,
                        lvl_off, scale, nullptr, n_kf, pt_f64, pt_desc32, n_pts, th, eps, out, 0, &sx);
    });
}

int orbfe_sim3_search_last_ms(float* ms) {
    return guarded([&] { last_ms<kPsSim3>(ms); });
}

int orbfe_fkf_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                     const int32_t* octave, const uint8_t* desc32, const uint8_t* blocked, const int64_t* cell_at,
                     const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx, const int64_t* lvl_off,
                     const double* scale, int32_t n_kf, const double* pt_f64, const uint8_t* pt_desc32, int64_t n_pts,
                     const int32_t* srch_kf, const int64_t* srch_off, int32_t n_srch, const int32_t* item_pt,
                     double th, double eps, const orbfe_fkf_out* out) {
    return guarded([&] {
        const Sim3In sx{nullptr, srch_kf, srch_off, n_srch, item_pt};
        search<kPsFkf>(kf_f64, kf_i32, off, xy, octave, nullptr, desc32, blocked, cell_at, cell_off, idx_at, cell_idx,
                       lvl_off, scale, nullptr, n_kf, pt_f64, pt_desc32, n_pts, th, eps, out, 0, &sx);
    });
}

int orbfe_fkf_search_last_ms(float* ms) {
    return guarded([&] { last_ms<kPsFkf>(ms); });
}

int orbfe_local_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                       const int32_t* octave, const double* u_right, const uint8_t* desc32, const uint8_t* blocked,
                       const int64_t* cell_at, const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx,
                       const int64_t* lvl_off, const double* scale, int32_t n_kf, const double* pt_f64,
                       const uint8_t* pt_desc32, int64_t n_pts, const double* srch_limit, const int32_t* srch_kf,
                       const int64_t* srch_off, int32_t n_srch, const int32_t* item_pt, double th, int32_t th_on,
                       double eps, const orbfe_local_out* out) {
    return guarded([&] {
        const Sim3In sx{srch_limit, srch_kf, srch_off, n_srch, item_pt, th_on != 0};
        search<kPsLocal>(kf_f64, kf_i32, off, xy, octave, u_right, desc32, blocked, cell_at, cell_off, idx_at,
                         cell_idx, lvl_off, scale, nullptr, n_kf, pt_f64, pt_desc32, n_pts, th, eps, out, 0, &sx);
    });
}

int orbfe_local_search_last_ms(float* ms) {
    return guarded([&] { last_ms<kPsLocal>(ms); });
}

int orbfe_ff_search(const double* kf_f64, const int32_t* kf_i32, const int64_t* off, const double* xy,
                    const int32_t* octave, const double* u_right, const uint8_t* desc32, const uint8_t* blocked,
                    const int64_t* cell_at, const int32_t* cell_off, const int64_t* idx_at, const int32_t* cell_idx,
                    const int64_t* lvl_off, const double* scale, int32_t n_kf, const double* pt_f64,
                    const uint8_t* pt_desc32, int64_t n_pts, const double* srch_th, const int32_t* srch_mode,
                    const int32_t* srch_kf, const int64_t* srch_off, int32_t n_srch, const int32_t* item_pt,
                    const int32_t* item_level, double eps, const orbfe_ff_out* out) {
    return guarded([&] {
        const Sim3In sx{srch_th, srch_kf, srch_off, n_srch, item_pt, 0, srch_mode, item_level};
        search<kPsFf>(kf_f64, kf_i32, off, xy, octave, u_right, desc32, blocked, cell_at, cell_off, idx_at, cell_idx,
                      lvl_off, scale, nullptr, n_kf, pt_f64, pt_desc32, n_pts, 0.0, eps, out, 0, &sx);
    });
}

int orbfe_ff_search_last_ms(float* ms) {
    return guarded([&] { last_ms<kPsFf>(ms); });
}

}  // extern "C"
