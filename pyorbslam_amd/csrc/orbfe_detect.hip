// orbfe_detect.hip — k_detect: per-cell FAST-9/16 + 3x3 NMS + iniTh/minTh fallback + ordered compaction
// (ComputeKeyPointsOctTree cell loop, ORBextractor.cpp:768-828).  Integer / packed-f16 work: no MFMA.
#include <hip/hip_runtime.h>

#include "orbfe_device.h"
#include "orbfe_kernels.h"

namespace orbfe {

// ------------------------------------------------------------------------------- k_detect
// One wavefront per (cell, image).  FAST "M" of a pixel:
//   M = max(v - min_arc max9, max_arc min9 - v) over the 16 arcs of 9 contiguous circle pixels;
//   the pixel is a segment-test corner at threshold t iff M > t, and OpenCV's cornerScore is M - 1.
// Work is done on horizontal pixel pairs (x, x + 1), x even, in packed f16: pixel values live in LDS as
// u16 0x3C00 | p, normal f16 numbers in [1, 2) ordered exactly like p, so v_pk_maximum3/minimum3_f16
// are exact and differences of the raw u16 bits are differences of p.
//  1. ROI -> LDS (u16, pitch RP, ROI column c at index c + 1 so even window columns are dword
//     aligned): 16 lanes per row each read one dword from the 4-byte aligned start of column -1, take
//     the next dword from the neighbour lane (DPP), re-align with v_alignbyte and widen with v_perm; the
//     next cell's loads are in flight during this cell's compute.
//  2. Pre-test, every pair: P = max(v - min_k max(c_k, c_k+1), max_k min(c_k, c_k+1) - v) over the
//     circularly adjacent cardinal pairs (circle points 0, 4, 8, 12) bounds M from above, because every
//     arc of 9 contains such a pair (computed as max(v - max(min(c0, c2), min(c1, c3)), ...): every
//     cycle edge joins an even and an odd cardinal).  Pairs with P <= tq = min(iniTh, minTh) in both pixels have M <= tq:
//     neither corners nor relevant NMS neighbours at either threshold; they keep M = 0.  The others are
//     queued in row-major order (ballot + mbcnt).  (Queueing single pixels halves the M work per pixel
//     but not per cell: a cell's queue is a few 64-entry steps either way, measured slower.)
//  3. Exact M of the queued pairs -> a u8 M map with a zero border (half the LDS of a u16 map: detect is
//     occupancy-bound, one 64-thread workgroup per wave); pairs with a pixel above max(tq, 1) are
//     compacted in place into the same queue (row-major) for NMS.
//  4. NMS over that queue, two pixels per lane.  For t >= 1, "score > every 8-neighbour's score at t" (neighbours outside the
//     window or not corners at t score 0) is equivalent to M > t and M > max(8-neighbour M): a neighbour
//     with M <= t is below M anyway.  So the local-max test is threshold independent: one pass decides
//     iniTh and minTh together, and the iniTh -> minTh fallback (ORBextractor.cpp:811-815) only picks
//     which survivor list is kept.  Kept pixels are written in the queue's row-major order, i.e.
//     cv::FAST's output order.
typedef _Float16 fd_h2 __attribute__((ext_vector_type(2)));
typedef short fd_s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ fd_h2 fd_h(uint32_t v) { return __builtin_bit_cast(fd_h2, v); }
__device__ __forceinline__ fd_s2 fd_s(fd_h2 v) { return __builtin_bit_cast(fd_s2, v); }
__device__ __forceinline__ fd_h2 fd_max(fd_h2 a, fd_h2 b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ fd_h2 fd_min(fd_h2 a, fd_h2 b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ fd_h2 fd_max3(fd_h2 a, fd_h2 b, fd_h2 c) { return fd_max(fd_max(a, b), c); }
__device__ __forceinline__ fd_h2 fd_min3(fd_h2 a, fd_h2 b, fd_h2 c) { return fd_min(fd_min(a, b), c); }
template <int DX>
__device__ __forceinline__ fd_h2 fd_pair(const uint32_t* q) {  // u16 pair at column offset DX
    if constexpr ((DX & 1) == 0) return fd_h(q[DX / 2]);
    else return fd_h(__builtin_amdgcn_alignbyte(q[(DX + 1) / 2], q[(DX - 1) / 2], 2));
}

// Upper bounds of the two adjacent pixel pairs at dwords R and R + 1 (pixels x .. x + 3), sharing the
// cardinal rows: 6 dwords of the centre row, 2 above, 2 below.
template <int S>
__device__ __forceinline__ void fast_bound_quad(const uint32_t* R, fd_s2& bA, fd_s2& bB) {
    const uint32_t m2 = R[-2], m1 = R[-1], z0 = R[0], p1 = R[1], p2 = R[2], p3 = R[3];
    const uint32_t u0 = R[-3 * S], u1 = R[-3 * S + 1], d0 = R[3 * S], d1 = R[3 * S + 1];
    auto bound = [](uint32_t v, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
        const fd_h2 h0 = fd_h(c0), h1 = fd_h(c1), h2 = fd_h(c2), h3 = fd_h(c3);
        // min over the 4 cycle edges (i, i + 1) of max(h_i, h_i+1): every edge joins an even and an odd
        // cardinal, so it is max(min(h0, h2), min(h1, h3)) (3 ops instead of 6); dually for b
        const fd_h2 a = fd_max(fd_min(h0, h2), fd_min(h1, h3));
        const fd_h2 b = fd_min(fd_max(h0, h2), fd_max(h1, h3));
        const fd_s2 vs = __builtin_bit_cast(fd_s2, v);
        return __builtin_elementwise_max(vs - fd_s(a), fd_s(b) - vs);
    };
    // cardinals in circle order: 0 = (0, +3), 4 = (+3, 0), 8 = (0, -3), 12 = (-3, 0)
    bA = bound(z0, d0, __builtin_amdgcn_alignbyte(p2, p1, 2), u0, __builtin_amdgcn_alignbyte(m1, m2, 2));
    bB = bound(p1, d1, __builtin_amdgcn_alignbyte(p3, p2, 2), u1, __builtin_amdgcn_alignbyte(z0, m1, 2));
}

// Exact M of the pixel pair at dword R (row stride S dwords), as biased u16 x2.
template <int S>
__device__ __forceinline__ uint32_t fast_m_pair(const uint32_t* R) {
    const fd_h2 p[16] = {fd_pair<0>(R + 3 * S),  fd_pair<1>(R + 3 * S),  fd_pair<2>(R + 2 * S),  fd_pair<3>(R + S),
                         fd_pair<3>(R),          fd_pair<3>(R - S),      fd_pair<2>(R - 2 * S),  fd_pair<1>(R - 3 * S),
                         fd_pair<0>(R - 3 * S),  fd_pair<-1>(R - 3 * S), fd_pair<-2>(R - 2 * S), fd_pair<-3>(R - S),
                         fd_pair<-3>(R),         fd_pair<-3>(R + S),     fd_pair<-2>(R + 2 * S), fd_pair<-1>(R + 3 * S)};
    fd_h2 mx3[16], mn3[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mx3[k] = fd_max3(p[k], p[(k + 1) & 15], p[(k + 2) & 15]);
        mn3[k] = fd_min3(p[k], p[(k + 1) & 15], p[(k + 2) & 15]);
    }
    fd_h2 lo = fd_max3(mx3[0], mx3[3], mx3[6]), hi = fd_min3(mn3[0], mn3[3], mn3[6]);
#pragma unroll
    for (int k = 1; k < 15; k += 2) {
        lo = fd_min3(lo, fd_max3(mx3[k], mx3[(k + 3) & 15], mx3[(k + 6) & 15]),
                     fd_max3(mx3[k + 1], mx3[(k + 4) & 15], mx3[(k + 7) & 15]));
        hi = fd_max3(hi, fd_min3(mn3[k], mn3[(k + 3) & 15], mn3[(k + 6) & 15]),
                     fd_min3(mn3[k + 1], mn3[(k + 4) & 15], mn3[(k + 7) & 15]));
    }
    lo = fd_min(lo, fd_max3(mx3[15], mx3[2], mx3[5]));
    hi = fd_max(hi, fd_min3(mn3[15], mn3[2], mn3[5]));
    const fd_s2 v = __builtin_bit_cast(fd_s2, R[0]);
    const fd_s2 m = __builtin_elementwise_max(__builtin_elementwise_max(v - fd_s(lo), fd_s(hi) - v), fd_s2{0, 0});
    return __builtin_bit_cast(uint32_t, m) | 0x3C003C00u;
}

__device__ __forceinline__ int imax3(int a, int b, int c) { return max(max(a, b), c); }

// o +/- (this lane's bit of the lane mask m): one v_addc / v_subb with the mask as the carry (the compiler's
// form of o + (int)inverse_ballot(m) is a v_cndmask and an add)
__device__ __forceinline__ int fd_plus_bit(int o, uint64_t m) {
    int r;
    uint64_t co;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(co) : "v"(o), "s"(m));
    return r;
}
__device__ __forceinline__ int fd_minus_bit(int o, uint64_t m) {
    int r;
    uint64_t co;
    asm("v_subb_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(co) : "v"(o), "s"(m));
    return r;
}

// cells per k_detect wavefront: 4 (the next cell's ROI loads overlap this one), or 1 for batches too small to
// give the chip >= 8 waves per CU that way (a frame pair: 610 waves of 4 cells, 2 440 of one)
constexpr int kFdCells = 4;
constexpr int kFdSmallCells = 1;  // cells per wave for small batches

template <bool B>
struct fd_flag {  // a compile-time switch passed to a generic lambda
    static constexpr bool value = B;
};

// u16 elements of k_detect's ROI area: the ROI itself, and after the M stage the minTh survivors of a cell
// (u32 records, at most slot_cap = Geo::fd_alt); a multiple of 8 so the M map after it is 16-byte aligned
__host__ __device__ inline int detect_roi_elems(const Geo& g, int rp) {
    const int n = rp * g.max_rh > 2 * g.fd_alt ? rp * g.max_rh : 2 * g.fd_alt;
    return (n + 7) & ~7;
}

// RP: ROI pitch in u16 (48, 64 or 96; >= widest ROI + 3).  NS: staged row slots (4 rows each, >= max_rh / 4).
// CPW: cells per wave.  ST: the debug counters of orbfe_debug_detect_stats / orbfe_debug_detect_lanes.
// 5 waves per SIMD (<= 96 VGPRs; 4 for the wider / taller ROI shapes, which need the registers) and
// <= 8 KiB of LDS for KITTI / EuRoC cells: detect is bound by how many
// cells are in flight per CU (16 -> 10 resident waves costs +32 %, measured by padding the launch's LDS).
template <int RP, int NS, int CPW, bool ST = false>
__global__ __launch_bounds__(64, (RP == 48 && NS <= 12) ? 5 : 4) void k_detect(Geo g, const CellGeo* __restrict__ cells, const uint8_t* __restrict__ in,
                                               int64_t in_pitch, const uint8_t* __restrict__ ws,
                                               int* __restrict__ cell_count, uint32_t* __restrict__ slots,
                                               int* __restrict__ stats) {
    constexpr int S = RP / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // ROI (max_rh rows x RP u16); after the M stage the same bytes stage the minTh survivors (u32 records)
    uint16_t* roi = (uint16_t*)lds;
    // u8 M map, (max_wh + 2) rows of MP = RP bytes: px (x, y) at (y + 1) * MP + x + 2, i.e. at the pair's queue
    // entry + MP
    constexpr int MP = RP;
    uint8_t* mm = (uint8_t*)(roi + detect_roi_elems(g, RP));
    // pair queue: entry = y * RP + x + 2 (x even; fd_pq entries), the ROI u16 index of the dword that holds
    // the top-left corner of the pair's circles (ROI row y = window row y - 3, pair at ROI index
    // entry + 3 RP + 2), so the M stage's ROI reads are the entry plus non-negative immediate offsets and its map
    // address the entry plus MP; the M stage compacts the queue in place into the NMS queue
    uint16_t* pq = (uint16_t*)(mm + MP * (g.max_wh + 2));
    int bx, img;
    xcd_block(bx, img);  // neighbouring cells' ROIs overlap by 6 rows / columns: keep them in one L2
    const int lane = threadIdx.x;
    const int c_first = bx * CPW, c_last = min(c_first + CPW, g.ncells);
    // ROI staging, 8 lanes per row (dwords 2d, 2d + 1), 8 rows per step (NS / 2 steps): lane d loads two
    // dwords of the row from the 4-byte aligned start of column -1 and takes dword 2d + 2 from its
    // neighbour lane (DPP row_shl:1) to re-align 8 bytes with v_alignbyte (rows are <= 59 px, so 16
    // dwords cover every row; what lane 7 receives from the next row's lane only lands in columns >= 60).
    // The loads of the next cell are issued before this cell's compute (prefetch into NS registers).
    constexpr int NS2 = NS / 2;
    const int d = lane & 7, r0 = lane >> 3;
    uint2 raw[NS2];
    // Every slot loads unconditionally, through a resource bounded to the level (a row past it reads 0): rows
    // past the ROI and dwords past its width land only in LDS the commit below never writes or in columns
    // past the ROI, and the per-slot range tests, zero fills and branches are gone (one v_add per slot)
    auto issue = [&](int c) {
        const CellGeo cg = load_cell(cells, c);
        int stride;
        const uint8_t* lvl = level_ptr(g, cg.level, in, in_pitch, ws, img, &stride);
        const __amdgpu_buffer_rsrc_t rs = bounded_rsrc(lvl, (uint32_t)(stride * g.lv[cg.level].h));
        const uint32_t lvl_lo = (uint32_t)(uintptr_t)lvl;
        const uint32_t off0 = (uint32_t)((cg.y0 + r0) * stride + cg.x0 - 1);
        // rows r0 + 8 k share the alignment of row r0 (8 k * stride is a multiple of 4)
        const uint32_t al0 = off0 - ((lvl_lo + off0) & 3u) + 8u * d;
#pragma unroll
        for (int k = 0; k < NS2; ++k)
            raw[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs, al0 + (uint32_t)(8 * k * stride), 0, 0));
    };
    if (c_first < c_last) issue(c_first);
    for (int c = c_first; c < c_last; ++c) {
        const CellGeo cg = load_cell(cells, c);
        const int rw = cg.x1 - cg.x0, rh = cg.y1 - cg.y0;
        const int ww = rw - 6, wh = rh - 6;  // detection window = ROI rows/cols 3 .. n-4
        {
            int stride;
            const uint8_t* lvl = level_ptr(g, cg.level, in, in_pitch, ws, img, &stride);
            const uint32_t lvl_lo = (uint32_t)(uintptr_t)lvl;
            const uint32_t off0 = (uint32_t)((cg.y0 + r0) * stride + cg.x0 - 1);
            const int n8 = (rw + 8) >> 3;  // 8-column groups of columns -1 .. rw-1 (8 * n8 <= RP)
#pragma unroll
            for (int k = 0; k < NS2; ++k) {
                // every lane takes part in the DPP (uniform control flow); lanes 15 of a DPP row get 0 (bound_ctrl:
                // the same 0 as an `old` operand, without the v_mov that would materialise it)
                const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)raw[k].x, 0x101, 0xF, 0xF, true);
                const int r = r0 + 8 * k;
                if (r < rh && d < n8) {
                    const int sh = (int)((lvl_lo + off0 + (uint32_t)(8 * k * stride)) & 3u);
                    const uint32_t w0 = __builtin_amdgcn_alignbyte(raw[k].y, raw[k].x, sh);
                    const uint32_t w1 = __builtin_amdgcn_alignbyte(nb, raw[k].y, sh);
                    uint4 u;
                    u.x = __builtin_amdgcn_perm(0x3C3C3C3Cu, w0, 0x04010400u);
                    u.y = __builtin_amdgcn_perm(0x3C3C3C3Cu, w0, 0x04030402u);
                    u.z = __builtin_amdgcn_perm(0x3C3C3C3Cu, w1, 0x04010400u);
                    u.w = __builtin_amdgcn_perm(0x3C3C3C3Cu, w1, 0x04030402u);
                    *(uint4*)(roi + r * RP + 8 * d) = u;
                }
            }
            // the M map with its zero border
            uint4* m128 = (uint4*)mm;
            for (int i = lane; i < (MP / 16) * (wh + 2); i += 64) m128[i] = uint4{0u, 0u, 0u, 0u};
        }
        if (c + 1 < c_last) issue(c + 1);  // in flight during this cell's compute
        __syncthreads();
        auto process = [&]() {
            if (ww <= 0 || wh <= 0) {
                if (lane == 0) cell_count[(int64_t)img * g.ncells + c] = 0;
                return;
            }
        const int tq = min(g.ini_th, g.min_th);
        // ---- 2. pre-test, two adjacent pairs (pixels x .. x + 3) per lane and step, quads in row-major
        //         order (lane -> quad i0 + lane); the pair queue stays row-major (two ballots per step)
        const int qrow = (ww + 3) >> 2, nquad = qrow * wh;
        // n / qrow for n <= 64 without an integer division: (n + 0.5) / qrow is >= 0.5 / qrow >= 1/28 away
        // from an integer, far more than the reciprocal's error
        const float rq = __builtin_amdgcn_rcpf((float)qrow);
        auto div_q = [&](int n) { return (int)__builtin_fmaf((float)n, rq, 0.5f * rq); };
        const int step_y = div_q(64), step_x = 64 - step_y * qrow;
        // Two queues when minTh < iniTh (ORBextractor.cpp:795-815: FAST at iniTh, then minTh only for a
        // cell where iniTh found nothing): B = pairs whose bound exceeds minTh (from the front of pq), and
        // its subset A = bound above iniTh (from the back, growing down).  Exact M, NMS and output run on A
        // first; B is processed only for a cell that A leaves empty.  A pixel outside every A pair has
        // M <= bound <= iniTh, so it can neither be an iniTh corner nor beat one in the NMS: the iniTh pass
        // needs M of the A pairs only.  Should the two queues meet (a cell where more than half of the pairs
        // pass at minTh), the cell takes the one-pass path below instead (both thresholds over B).
        const bool two = g.min_th < g.ini_th;
        const int tA = two ? g.ini_th : 0x7fff;  // above every bound
        const int cap = g.fd_pq;
        int npq = 0, npa = 0;
        {
            // two 64-quad steps per iteration: both steps' ROI reads are issued before either waits
            // (one LDS round trip per 128 quads); lanes past the window read a clamped row and vote 0
            int qy = div_q(lane), qx = lane - qy * qrow;
            auto advance = [&](int& y, int& x) {
                y += step_y;
                x += step_x;
                if (x >= qrow) {
                    x -= qrow;
                    ++y;
                }
            };
            // the pass conditions as lane masks (v_cmp straight into SGPR pairs, combined on the SALU): a
            // bool per lane would cost a v_cndmask + v_cmp round trip per ballot.  Only the last quad of a
            // row can hold pixels past the window (x4 == xl); rem = ww - xl of its 4 are inside.
            const int xl = 4 * (qrow - 1), rem = ww - xl;
            auto gt = [](int a, int b) { return (uint64_t)__builtin_amdgcn_sicmp(a, b, 38); };  // ICMP_SGT
            auto bound_at = [&](const uint32_t* R, uint64_t in, uint64_t last, uint64_t& ca, uint64_t& cb, uint64_t& aa,
                                uint64_t& ab) {
                fd_s2 ba, bb;
                fast_bound_quad<S>(R, ba, bb);
                const uint64_t va = rem > 1 ? ~0ull : ~last, vb2 = rem > 2 ? ~0ull : ~last,
                               vb3 = rem > 3 ? ~0ull : ~last;
                ca = in & (gt(ba.x, tq) | (gt(ba.y, tq) & va));
                cb = in & vb2 & (gt(bb.x, tq) | (gt(bb.y, tq) & vb3));
                aa = ca & (gt(ba.x, tA) | (gt(ba.y, tA) & va));
                ab = cb & (gt(bb.x, tA) | (gt(bb.y, tA) & vb3));
            };
            auto bound = [&](int i, int y, int x4, uint64_t& ca, uint64_t& cb, uint64_t& aa, uint64_t& ab) {
                bound_at((const uint32_t*)(roi + (min(y, wh - 1) + 3) * RP + x4 + 4),
                         __builtin_amdgcn_sicmp(i, nquad, 40), __builtin_amdgcn_sicmp(x4, xl, 32), ca, cb, aa, ab);
            };
            // entries in lane order, a lane's first before its second: the lane's first goes after every entry
            // of the lanes below it (one mbcnt chain over both masks, seeded with the queue length), its second
            // one further when it has a first
            auto below2 = [](uint64_t m0, uint64_t m1, int base) {
                return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1,
                       __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, base))));
            };
            auto emit = [&](int n, uint64_t b0, uint64_t b1, uint64_t a0, uint64_t a1) {
                const bool ca = __builtin_amdgcn_inverse_ballot_w64(b0), cb = __builtin_amdgcn_inverse_ballot_w64(b1);
                const uint16_t e = (uint16_t)n;
                const int o = below2(b0, b1, npq);
                if (ca) pq[o] = e;
                if (cb) pq[fd_plus_bit(o, b0)] = (uint16_t)(e + 2);
                npq += __popcll(b0) + __popcll(b1);
                // a half without an A pair (more than half of them) leaves npa and the collide rule as they are:
                // the A emission (two inverse ballots, an mbcnt chain, two address chains and stores) runs under
                // one scalar test
                {   // one threshold: tA is out of reach, the A masks are empty
                    const int na = __popcll(a0) + __popcll(a1);
                    if (ST && lane == 0 && two && na == 0) atomicAdd(&stats[6], 1);
                    // both counts only grow: once the queues would meet they stay met (collide below), and A
                    // stops writing so that B stays intact for the one-pass path
                    if (na != 0 && npq + npa + na <= cap) {
                        const bool aa = __builtin_amdgcn_inverse_ballot_w64(a0), ab = __builtin_amdgcn_inverse_ballot_w64(a1);
                        const int oa = cap - 1 - below2(a0, a1, npa);
                        if (aa) pq[oa] = e;
                        if (ab) pq[fd_minus_bit(oa, a0)] = (uint16_t)(e + 2);
                    }
                    npa += na;
                }
            };
            if (qrow <= 8) {
                // rows of 8 lanes (every KITTI / EuRoC cell but EuRoC level 7's): lane 8 r + qx takes quad qx
                // of row y0 + r (lanes qx >= qrow idle), so the lane order is the row-major queue order and
                // the ROI address and the entry are per-lane constants plus a uniform row offset.  Lanes of
                // rows past the window read (and vote 0 on) rows below it: still inside the LDS allocation
                // (ROI rows, then the M map).
                const int r = lane >> 3, qx = lane & 7;
                const uint64_t colok = __builtin_amdgcn_sicmp(qx, qrow, 40), last = __builtin_amdgcn_sicmp(4 * qx, xl, 32);
                const uint32_t* R0 = (const uint32_t*)(roi + (r + 3) * RP + 4 * qx + 4);
                for (int y0 = 0; y0 < wh; y0 += 16) {
                    uint64_t ca0, cb0, ca1, cb1, aa0, ab0, aa1, ab1;
                    bound_at(R0 + y0 * S, colok & __builtin_amdgcn_sicmp(r, wh - y0, 40), last, ca0, cb0, aa0, ab0);
                    bound_at(R0 + (y0 + 8) * S, colok & __builtin_amdgcn_sicmp(r, wh - y0 - 8, 40), last, ca1, cb1, aa1,
                             ab1);
                    emit((y0 + r) * RP + 4 * qx + 2, ca0, cb0, aa0, ab0);
                    emit((y0 + r + 8) * RP + 4 * qx + 2, ca1, cb1, aa1, ab1);
                }
            } else {
                for (int i0 = 0; i0 < nquad; i0 += 128) {
                    int qy2 = qy, qx2 = qx;
                    advance(qy2, qx2);
                    uint64_t ca0, cb0, ca1, cb1, aa0, ab0, aa1, ab1;
                    bound(i0 + lane, qy, 4 * qx, ca0, cb0, aa0, ab0);
                    bound(i0 + 64 + lane, qy2, 4 * qx2, ca1, cb1, aa1, ab1);
                    emit(qy * RP + 4 * qx + 2, ca0, cb0, aa0, ab0);
                    emit(qy2 * RP + 4 * qx2 + 2, ca1, cb1, aa1, ab1);
                    qy = qy2;
                    qx = qx2;
                    advance(qy, qx);
                }
            }
        }
        __syncthreads();
        // ---- 3. exact M of a queue's pairs -> M map; the pairs with a pixel above tl are compacted in place
        //         (entry i at qb[dir * i]: dir -1 for A at the back of pq) into the NMS queue; returns its length
        //         The stage takes the entries [first, n) and appends to the nn entries the queue already holds
        //         (nn <= first).  With a carry (the A queue only), the kb lanes that the last step leaves idle take
        //         the B entries pq[0 .. kb): they store their M too and compact the pairs with a pixel above
        //         max(minTh, 1) in place into pq[0 .. nnb), outside the stage's own compaction (a pair of both
        //         queues would otherwise enter A's NMS queue twice); kb <= those idle lanes, so only the last step
        //         carries.
        auto m_stage = [&](auto carry, uint16_t* qb, int dir, int first, int n, int nn, int tl, int kb, int& nnb) {
            constexpr bool CY = decltype(carry)::value;
            const int ne = CY ? n + kb : n;  // entries that have a lane
            auto slot = [&](int i) { return CY && i >= n ? pq + (i - n) : qb + dir * i; };
            // the queue entry of the next step is read one step ahead (its LDS round trip overlaps this step)
            uint32_t e_next = first + lane < ne ? *slot(first + lane) : 2u;  // idle lanes: pixel (0, 0)
            for (int k0 = first; k0 < n; k0 += 64) {
                // every lane computes (a lane past ne repeats an earlier entry of its own, harmlessly); the map
                // store and the compaction take the lanes of this step's entries (lane masks, as the pre-test)
                const uint32_t e = e_next;
                if (k0 + 64 + lane < ne) e_next = *slot(k0 + 64 + lane);
                const uint64_t inr = __builtin_amdgcn_sicmp(k0 + lane, n, 40);  // ICMP_SLT
                const uint64_t ine = CY ? (uint64_t)__builtin_amdgcn_sicmp(k0 + lane, ne, 40) : inr;
                const uint32_t m = fast_m_pair<S>((const uint32_t*)(roi + e) + 3 * S + 1);
                // the u8 map keeps M itself (low byte of each biased half); odd width: the last pair's second
                // pixel lies outside the window, its map entry is cleared after this stage
                if (__builtin_amdgcn_inverse_ballot_w64(ine))
                    *(uint16_t*)(mm + e + MP) = (uint16_t)__builtin_amdgcn_perm(0u, m, 0x0c0c0200u);
                // slots below k0 + 64 are written; every read of the queue (this step's entries, the next
                // step's prefetch) was issued before
                auto above = [&](int t) {
                    return (uint64_t)__builtin_amdgcn_sicmp((int)(m & 0x3FFu), t, 38) |
                           (uint64_t)__builtin_amdgcn_sicmp((int)((m >> 16) & 0x3FFu), t, 38);
                };
                const uint64_t bh = inr & above(tl);
                if (__builtin_amdgcn_inverse_ballot_w64(bh)) qb[dir * (nn + lanes_below(bh))] = (uint16_t)e;
                nn += __popcll(bh);
                if (CY && (ine & ~inr) != 0) {  // the carried lanes: their entries pq[0 .. kb) are all read
                    const uint64_t bc = ine & ~inr & above(max(g.min_th, 1));
                    if (__builtin_amdgcn_inverse_ballot_w64(bc)) pq[nnb + lanes_below(bc)] = (uint16_t)e;
                    nnb += __popcll(bc);
                }
            }
            // odd width: column ww (right of the window) got the outside pixel's M from the last pairs; NMS
            // reads it as a neighbour (and as that pixel's own score) and needs 0 there
            if ((ww & 1) && lane < wh) mm[(lane + 1) * MP + ww + 2] = 0;
            __syncthreads();
            return nn;
        };
        // ---- 4. NMS (local max) over an NMS queue + ordered compaction.  For t >= 1, "score > every
        //         8-neighbour's score at t" is M > t and M > max(neighbour M) (a neighbour with M <= t is
        //         below anyway).  Kept pixels: pairs row-major, pixel x before x + 1 = cv::FAST's order.
        //         thb1 >= 1: also test the second threshold and stage its survivors in `alt` (one-pass path).
        uint32_t* out = slots + (int64_t)img * g.slot_total + cg.slot_off;
        uint32_t* alt = (uint32_t*)roi;  // >= 2 * slot_cap u16 (detect_roi_elems)
        auto nms_stage = [&](const uint16_t* qb, int dir, int nn, int thb0, int thb1, int& t0, int& t1) {
            t0 = t1 = 0;
            for (int k0 = 0; k0 < nn; k0 += 64) {
                // every lane computes on an entry in range; lane masks select the kept pixels
                const uint64_t inr = __builtin_amdgcn_sicmp(k0 + lane, nn, 40);  // ICMP_SLT
                const int e = qb[dir * min(k0 + lane, nn - 1)];
                const uint8_t* q = mm + e + MP;  // pixel A = (x, y); B = (x + 1, y)
                const int t_0 = q[-MP - 1], t_1 = q[-MP], t_2 = q[-MP + 1], t_3 = q[-MP + 2];
                const int m_0 = q[-1], owna = q[0], ownb = q[1], m_3 = q[2];
                const int b_0 = q[MP - 1], b_1 = q[MP], b_2 = q[MP + 1], b_3 = q[MP + 2];
                const int c1 = max(t_1, b_1), c2 = max(t_2, b_2);  // the pair's columns without its own row
                const int na = max(imax3(t_0, m_0, b_0), imax3(c1, c2, ownb));
                const int nb = max(imax3(t_3, m_3, b_3), imax3(c1, c2, owna));
                // (x + 3, y + 3) = (e % RP + 1, e / RP + 3)
                const uint32_t xy = (uint32_t)(cg.x0 + (int)((uint32_t)e % RP) + 1) +
                                    __umul24((uint32_t)(cg.y0 + (int)((uint32_t)e / RP) + 3), (uint32_t)cg.kw);
                const uint32_t reca = xy | ((uint32_t)(owna - 1) << 24);
                const uint32_t recb = (xy + 1u) | ((uint32_t)(ownb - 1) << 24);
                auto keep = [&](int th, uint64_t& ba, uint64_t& bb, int& t, uint32_t* dst) {
                    ba = inr & (uint64_t)__builtin_amdgcn_sicmp(owna, max(na, th), 38);
                    bb = inr & (uint64_t)__builtin_amdgcn_sicmp(ownb, max(nb, th), 38);
                    const bool ka = __builtin_amdgcn_inverse_ballot_w64(ba), kb = __builtin_amdgcn_inverse_ballot_w64(bb);
                    const int o = t + lanes_below(ba) + lanes_below(bb);
                    // slot_cap holds by the strict NMS (no two kept pixels are 8-neighbours); never write past it
                    if (ka && o < cg.slot_cap) dst[o] = reca;
                    if (kb) {
                        const int ob = fd_plus_bit(o, ba);
                        if (ob < cg.slot_cap) dst[ob] = recb;
                    }
                    t += __popcll(ba) + __popcll(bb);
                };
                uint64_t ba, bb;
                keep(thb0, ba, bb, t0, out);
                if (thb1 > 0) keep(thb1, ba, bb, t1, alt);
            }
        };
        const bool collide = npq + npa > cap;
        // orbfe_debug_detect_stats: cells that took the one-pass path despite two thresholds (the queues met)
        if (ST && lane == 0 && two && collide) atomicAdd(&stats[1], 1);
        int total = 0;
        if (two && !collide) {
            int t0, t1;
            // A's last M step has 64 ceil(npa / 64) - npa idle lanes (on average nine tenths of the step): they take
            // the first kb entries of B.  Such an entry outside A has M <= bound <= iniTh in both pixels, so its map
            // entry (0 until now) changes neither A's compaction nor the iniTh NMS; an entry of both queues stores
            // the same M twice.  The fallback then starts behind the carried entries, on their nnb0 <= kb survivors
            // (the front of pq and the A region at its back are disjoint: npq + npa <= cap).
            const int kb = min(((npa + 63) & ~63) - npa, npq);
            int nnb0 = 0, none = 0;
            const int nna = m_stage(fd_flag<true>{}, pq + cap - 1, -1, 0, npa, 0, max(tA, 1), kb, nnb0);
            if (ST && lane == 0 && kb > 0) {
                atomicAdd(&stats[3], 1);
                atomicAdd(&stats[4], kb);
            }
            nms_stage(pq + cap - 1, -1, nna, max(g.ini_th, 1), 0, t0, t1);
            total = t0;
            if (t0 == 0) {  // minTh fallback: the rest of B (the A pairs' M is recomputed, identically)
                if (ST && lane == 0) {
                    atomicAdd(&stats[2], 1);
                    atomicAdd(&stats[5], (npq - kb + 63) >> 6);
                }
                const int nnb = m_stage(fd_flag<false>{}, pq, 1, kb, npq, nnb0, max(g.min_th, 1), 0, none);
                nms_stage(pq, 1, nnb, max(g.min_th, 1), 0, t0, t1);
                total = t0;
            }
        } else {
            // one pass over B at tq = min(iniTh, minTh), both thresholds in the NMS: iniTh survivors go
            // straight out, minTh survivors are staged in the (dead) ROI area and copied out only if iniTh
            // kept nothing
            int none = 0;
            const int nnq = m_stage(fd_flag<false>{}, pq, 1, 0, npq, 0, max(tq, 1), 0, none);
            const bool fb = g.min_th != g.ini_th;
            int t0, t1;
            nms_stage(pq, 1, nnq, max(g.ini_th, 1), fb ? max(g.min_th, 1) : 0, t0, t1);
            total = t0;
            if (t0 == 0 && t1 > 0) {
                __syncthreads();
                for (int i = lane; i < min(t1, cg.slot_cap); i += 64) out[i] = alt[i];
                total = t1;
            }
        }
        if (lane == 0) cell_count[(int64_t)img * g.ncells + c] = min(total, cg.slot_cap);
        if (ST && lane == 0) atomicAdd(&stats[0], 1);
        };
        process();
        __syncthreads();  // the next cell overwrites the ROI and the M map
    }
}

int detect_rp(const Geo& g) { return g.max_rw + 3 <= 48 ? 48 : g.max_rw + 3 <= 64 ? 64 : 96; }

size_t detect_lds_bytes(const Geo& g) {
    // ROI, the M map (pitch RP bytes), the pair queue
    return 2 * (size_t)detect_roi_elems(g, detect_rp(g)) + (size_t)detect_rp(g) * (g.max_wh + 2) + 2 * (size_t)g.fd_pq;
}

// cells per wave for a batch: 4 unless that leaves fewer than 8 waves per CU
int detect_cpw(const Geo& g, int n_images) {
    // 8 pairs: 39 us with one cell per wave against 47 with four (tools/microbench.py, round 4)
    return n_images < kSmallBatchImages || (int64_t)n_images * ((g.ncells + kFdCells - 1) / kFdCells) < 8 * 256
               ? kFdSmallCells
               : kFdCells;
}

template <int RP, int NS>
static void launch_detect_rp(const Geo& g, const CellGeo* cells, const uint8_t* in, int64_t in_pitch, const uint8_t* ws,
                             int* cell_count, uint32_t* slots, int n_images, hipStream_t s, int cpw, int* stats) {
    const dim3 grid((g.ncells + cpw - 1) / cpw, n_images), blk(64);
    const size_t lds = detect_lds_bytes(g);
    auto k = stats ? (cpw == kFdSmallCells ? k_detect<RP, NS, kFdSmallCells, true> : k_detect<RP, NS, kFdCells, true>)  // debug counters
                   : (cpw == kFdSmallCells ? k_detect<RP, NS, kFdSmallCells> : k_detect<RP, NS, kFdCells>);
    hipLaunchKernelGGL(k, grid, blk, lds, s, g, cells, in, in_pitch, ws, cell_count, slots, stats);
}

hipError_t launch_detect(const Geo& g, const CellGeo* cells, const uint8_t* in, int64_t in_pitch, const uint8_t* ws,
                         int* cell_count, uint32_t* slots, int n_images, hipStream_t s, int cells_per_wave, int* stats) {
    const int cpw = cells_per_wave ? cells_per_wave : detect_cpw(g, n_images);
    if (cpw != kFdCells && cpw != kFdSmallCells) return hipErrorInvalidValue;
    // ROIs of at most 48 rows (KITTI, EuRoC) stage from 12 registers, taller ones (<= 64) from 16
    const bool tall = g.max_rh > 48;
    switch (detect_rp(g)) {
        case 48:
            if (tall) launch_detect_rp<48, 16>(g, cells, in, in_pitch, ws, cell_count, slots, n_images, s, cpw, stats);
            else launch_detect_rp<48, 12>(g, cells, in, in_pitch, ws, cell_count, slots, n_images, s, cpw, stats);
            break;
        case 64:
            if (tall) launch_detect_rp<64, 16>(g, cells, in, in_pitch, ws, cell_count, slots, n_images, s, cpw, stats);
            else launch_detect_rp<64, 12>(g, cells, in, in_pitch, ws, cell_count, slots, n_images, s, cpw, stats);
            break;
        default: launch_detect_rp<96, 16>(g, cells, in, in_pitch, ws, cell_count, slots, n_images, s, cpw, stats);
    }
    return hipGetLastError();
}

}  // namespace orbfe
