// orbfe_resize.hip — the pyramid: cv::resize INTER_LINEAR 8U, level by level (k_resize_rows) or every level in
// one launch for small batches (k_resize_cascade) (ComputePyramid, ORBextractor.cpp:1106-1132).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "orbfe_device.h"
#include "orbfe_internal.h"

namespace orbfe {

// the scalar tail of the vertical pass: FixedPtCast<int, uchar, 22> (round half up) of INTER_LINEAR, or for
// the INTER_AREA fast path saturate_cast<uchar>(sum * 0.25f), i.e. sum / 4 rounded half to even (t = sum << 20)
__device__ __forceinline__ uint32_t resize_tail(uint32_t t, int area) {
    if (!area) return (t + (1u << 21)) >> 22;
    const uint32_t q = t >> 22, r = t & 0x3FFFFFu;
    return q + (r > 0x200000u || (r == 0x200000u && (q & 1u)));
}

// ------------------------------------------------------------------------------- k_resize
// The per-level kernel (k_resize_rows) and the one-launch cascade (k_resize_cascade) share this scheme for a
// band of output rows of level l (l >= 1), full width:
//  * staging: the source rows the band reads (sy0(first) .. sy1(last) of level l-1) are one contiguous
//    byte range in memory for every level (stride W for the input, the 16-byte pitch for derived levels),
//    so they are copied to LDS as a flat run of aligned dwords, every load issued before the first wait;
//    LDS byte sh0 + r * stride + c holds source row ys_lo + r, column c (sh0 = the range's misalignment).
//  * the level's x coefficients become, per 4-pixel group, v_perm selectors into an 8-byte tap window
//    starting at the group's first sx plus the packed (a0, a1) weights.
//  * compute: per group and row, 2 x (3 LDS dwords, 2 v_alignbyte, 4 v_perm + 4 v_dot2_u32_u16) for the
//    horizontal taps, then OpenCV's vertical rounding; one aligned dword store per 4 output pixels.

// Horizontal taps of a group's 4th pixel from a window of its own (LevelGeo::wide): A3 = LDS byte address of
// its source pixel sx3, aa = its (a0, a1) weights.
// (W3 = A3 - o the window's aligned address, o = A3 & 3: k_resize_rows hoists them out of its row loop)
__device__ __forceinline__ uint32_t resize_tap3_al(uint32_t W3, uint32_t o, uint32_t aa) {
    typedef __attribute__((address_space(3))) const uint32_t lds_c32;
    lds_c32* w = (lds_c32*)(uintptr_t)W3;
    const uint32_t x = __builtin_amdgcn_alignbyte(w[1], w[0], o);
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(x, x, 0x0c010c00u)),
                                  __builtin_bit_cast(us2, aa), 0u, false);
}
__device__ __forceinline__ uint32_t resize_tap3(uint32_t A3, uint32_t aa) {
    const uint32_t o = A3 & 3u;
    return resize_tap3_al(A3 - o, o, aa);
}
constexpr int kRsSlots = 16;     // k_resize_cascade: staged dwords per thread per pass (it takes half)
constexpr int kRsRowSlots = 24;  // k_resize_rows: staged dwords per thread per pass (a short pass takes 8 or 16)

// k_resize_rows: one workgroup per band of LevelGeo::rs_rows output rows, the compute mapped so that a wave's
// row is uniform.  The block holds R_s row sets of W_g waves (64 W_g >= the level's groups): lane
// (w % W_g) * 64 + lane of a set owns one 4-pixel group for the whole band, its x selectors / weights in
// registers; set w / W_g takes a run of consecutive rows of the band.  A row's source-row LDS addresses and
// vertical weights come from scalar loads of the y table, the store is a buffer store with the row offset in
// soffset: per 4 pixels only the taps, the vertical rounding and the pack are VALU work.  Blocks of
// NT = 64 (W_g R_s + remainder wave) threads, 256 <= NT <= 512 (the host picks R_s).  AL4: the source row
// stride is a multiple of 4 (every derived level's pitch, the input when its width is), so a group's window
// has the same misalignment in every source row.
template <bool MULTI, bool AL4, int NT>
__global__ __launch_bounds__(512) void k_resize_rows(Geo g, int l, const uint8_t* __restrict__ in, int64_t in_pitch,
                                                     uint8_t* __restrict__ ws, const ResizeX* __restrict__ xt,
                                                     const ResizeY* __restrict__ yt, int wg, int remw, int wgl,
                                                     int* __restrict__ zero_word) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    // staged source rows; the staging's pointers carry their address spaces (generic ones compile to flat
    // loads, which the compiler must wait for with vmcnt and lgkmcnt together)
    typedef __attribute__((address_space(3))) uint32_t lds_w32;
    typedef __attribute__((address_space(1))) const uint32_t glb_u32;
    lds_w32* s_src = (lds_w32*)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)rs_lds;
    const LevelGeo& L = g.lv[l];
    const LevelGeo& P = g.lv[l - 1];
    int bx, img;
    xcd_block(bx, img);
    const int t = threadIdx.x;
    if (zero_word && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) *zero_word = 0;
    const int rows = L.rs_rows;  // kRsRows, fewer for very wide levels (LevelGeo::rs_rows)
    const int dy0 = bx * rows, nrow = min(rows, L.h - dy0);
    const int ngrp = (L.w + 3) >> 2;
    int sstride;
    const uint8_t* src = level_ptr(g, l - 1, in, in_pitch, ws, img, &sstride);
    const ResizeY* yb = yt + L.ytab_off + dy0;
    const int ys_lo = yb[0].sy0, ys_hi = yb[nrow - 1].sy1;
    const uintptr_t a0 = (uintptr_t)(src + (int64_t)ys_lo * sstride);
    const int sh0 = (int)(a0 & 3);
    glb_u32* gsrc = (glb_u32*)(a0 - sh0);
    const int ndw = ((ys_hi - ys_lo) * sstride + P.w + sh0 + 3) >> 2;
    typedef __attribute__((address_space(3))) const uint32_t lds_u32;
    const uint32_t src_lds = (uint32_t)(uintptr_t)s_src;
    // this thread's group: x selectors / weights straight from the table (issued with the staging loads)
    // remw = 1: the last wave takes the groups past the wg full 64-group chunks (rem < 64 of them) for all
    // rows of the band: lane j owns group wg * 64 + j % rem and rows j / rem, + 64 / rem, ... (a per-lane
    // row), instead of a mostly idle row-uniform wave per row.  A set has wgl <= 8 waves: when a level has
    // more chunks than that (rows wider than 2 048 px), a set's wave walks chunks c, c + wgl, ...
    const int wv = t >> 6, fullw = NT / 64 - remw, nset = fullw / wgl;
    const bool remwave = wv >= fullw;
    const int set = __builtin_amdgcn_readfirstlane(remwave ? 0 : wv / wgl);
    const int rem = ngrp - wg * 64, lane = t & 63;
    const int rstep = remwave ? 64 / rem : nset;  // rows between a lane's rows in the remainder wave
    const int row0 = remwave ? lane / rem : set;
    int ch = remwave ? wg : wv - set * wgl;       // this wave's first 64-group chunk
    const int ch_step = remwave ? 1 : wgl, ch_end = remwave ? wg + 1 : wg;
    int grp = 0;
    bool own = false;
    uint4 e{}, aa{};
    int sx0 = 0;
    uint32_t d3 = 0;  // LevelGeo::wide: the 4th pixel's source column past the group's first
    auto chunk = [&](int c) {
        grp = remwave ? wg * 64 + lane % rem : c * 64 + lane;
        own = remwave ? lane < rstep * rem : grp < ngrp;
        if (own) {
            const uint4* xg = (const uint4*)(xt + L.xtab_off);
            const uint4 q0 = xg[2 * grp], q1 = xg[2 * grp + 1];
            sx0 = (int)q0.x;
            d3 = q1.z - q0.x;
            auto sel = [&](uint32_t sx) { const uint32_t r = sx - q0.x; return r | ((r + 1) << 16) | 0x0c000c00u; };
            e = uint4{sel(q0.x), sel(q0.z), sel(q1.x), sel(q1.z)};
            aa = uint4{q0.y, q0.w, q1.y, q1.w};
        }
    };
    chunk(ch);
    // staging by every thread of the block: compile-time strides (NT), immediate LDS offsets, and every load of
    // a pass (up to kRsRowSlots dwords per thread; KITTI's bands take one pass, level 1 its 21 slots) issued
    // before the first wait.  The loads go through a wave-uniform buffer resource: one VGPR offset for all
    // slots, the slot and pass in the SGPR offset, no 64-bit address arithmetic; the range test is one compare
    // of the thread index against a wave-uniform limit per slot, shared by the load and the LDS store.  The
    // test must guard the load itself: the resource's bounds check does not include the SGPR offset, so an
    // unguarded slot past the run reads past the buffer.
    {
        const __amdgpu_buffer_rsrc_t rsrc = bounded_rsrc((const void*)(uintptr_t)gsrc, (uint32_t)(4 * ndw));
        // one pass: S slots per thread, every load before the first LDS store
        auto pass = [&](auto nslot, int base, int left) {
            constexpr int S = decltype(nslot)::value;
            uint32_t v[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                v[k] = 0u;
                if (t < left - NT * k)
                    v[k] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (uint32_t)(4 * t), (uint32_t)(4 * (base + NT * k)), 0);
            }
            // one LDS address per pass (immediate offsets per slot)
            lds_w32* sp = s_src + base + t;
#pragma unroll
            for (int k = 0; k < S; ++k)
                if (t < left - NT * k) sp[NT * k] = v[k];
        };
        for (int base = 0; base < ndw; base += NT * kRsRowSlots) {
            const int left = ndw - base;  // wave-uniform: a scalar branch picks the pass's slot count
            if (left <= NT * kRsRowSlots / 3)
                pass(std::integral_constant<int, kRsRowSlots / 3>{}, base, left);
            else if (left <= NT * (kRsRowSlots * 2 / 3))
                pass(std::integral_constant<int, kRsRowSlots * 2 / 3>{}, base, left);
            else
                pass(std::integral_constant<int, kRsRowSlots>{}, base, left);
        }
    }
    __syncthreads();
    uint8_t* dst = ws + (int64_t)img * g.ws_bytes + L.ws_off + (int64_t)dy0 * L.pitch;
    const __amdgpu_buffer_rsrc_t rd = uniform_rsrc(dst);
    for (;;) {
        if (!own) return;  // only a level's last chunk is partial
        const int dx = 4 * grp;
        const bool tail = dx + 3 >= L.xvec;  // FixedPtCast<int, uchar, 22> past the last SIMD block
        const uint32_t lsrc = src_lds + (uint32_t)sh0 + (uint32_t)sx0;
        // AL4: the window's misalignment and aligned base, the same in every source row of the band
        const uint32_t lo = lsrc & 3u, lal = lsrc - lo, lo3 = (lsrc + d3) & 3u, lal3 = lsrc + d3 - lo3;
        // TAIL: a wave with a lane in the scalar tail (a level's last groups), or the remainder wave, keeps the
        // taps unmasked for resize_tail and tests each lane per row; every other wave masks a source row's taps
        // once, where they are produced (reused taps would be masked twice), and packs without the test
        auto band = [&](auto tail_c) {
            constexpr bool TAIL = decltype(tail_c)::value;
            // psy: the previous row's second source row.  Full waves walk consecutive rows, and a row's first
            // source row is mostly the previous row's second: its taps are reused, not recomputed.  The two tap
            // sets alternate between ha and hb over a 2-row unrolled loop, so the reuse needs no register copies
            // (4-5 v_mov per row and 4-pixel group before)
            int psy = -1;
            auto row = [&](int rr, uint32_t (&h0)[4], uint32_t (&h1)[4], bool reuse) {
                const ResizeY y = yb[rr];  // full waves: uniform, scalar loads
                const uint32_t r0 = (uint32_t)((y.sy0 - ys_lo) * sstride), r1 = (uint32_t)((y.sy1 - ys_lo) * sstride);
                const uint32_t B0 = (uint32_t)y.b0 << 12, B1 = (uint32_t)y.b1 << 12;
                auto taps = [&](uint32_t roff, uint32_t (&h)[4]) {
                    const uint32_t A = lsrc + roff, o = AL4 ? lo : A & 3u;
                    lds_u32* w = (lds_u32*)(uintptr_t)(AL4 ? lal + roff : A - o);
                    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
                    const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, o), d1 = __builtin_amdgcn_alignbyte(w2, w1, o);
                    h[0] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.x)),
                                                  __builtin_bit_cast(us2, aa.x), 0u, false);
                    h[1] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.y)),
                                                  __builtin_bit_cast(us2, aa.y), 0u, false);
                    h[2] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.z)),
                                                  __builtin_bit_cast(us2, aa.z), 0u, false);
                    h[3] = L.wide ? (AL4 ? resize_tap3_al(lal3 + roff, lo3, aa.w) : resize_tap3(A + d3, aa.w))
                                  : __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.w)),
                                                           __builtin_bit_cast(us2, aa.w), 0u, false);
                    if (!TAIL) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) h[k] &= ~15u;
                    }
                };
                // h0 holds the taps of source row psy (the previous row's h1) when reuse applies
                if (!(reuse && y.sy0 == psy)) taps(r0, h0);
                taps(r1, h1);
                if (reuse) psy = y.sy1;
                uint32_t out;
                if (TAIL) {
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (__umulhi(h0[k] & ~15u, B0) + __umulhi(h1[k] & ~15u, B1) + 2) >> 2;
                    if (tail) {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (dx + k >= L.xvec) v[k] = resize_tail(h0[k] * (B0 >> 12) + h1[k] * (B1 >> 12), L.area);
                    }
                    out = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
                } else {
                    // the sums + 2 are below 2^10: two to a dword at 16-bit spacing, one shift for both, one v_perm
                    // for the four bytes (5 instructions for 7)
                    uint32_t s[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = __umulhi(h0[k], B0) + __umulhi(h1[k], B1);
                    const uint32_t p01 = ((s[1] << 16) + (s[0] + 0x20002u)) >> 2, p23 = ((s[3] << 16) + (s[2] + 0x20002u)) >> 2;
                    out = __builtin_amdgcn_perm(p23, p01, 0x06040200u);
                }
                // pixels past L.w land in the row's pitch padding
                __builtin_amdgcn_raw_buffer_store_b32(out, rd, (uint32_t)dx, (uint32_t)(rr * L.pitch), 0);
            };
            uint32_t ha[4] = {0u, 0u, 0u, 0u}, hb[4] = {0u, 0u, 0u, 0u};
            if (!(TAIL && remwave)) {  // set s: rows [s * per, (s + 1) * per), consecutive
                const int per = (nrow + nset - 1) / nset, rend = min(set * per + per, nrow);
                int rr = set * per;
                for (; rr + 1 < rend; rr += 2) {
                    row(rr, ha, hb, true);
                    row(rr + 1, hb, ha, true);
                }
                if (rr < rend) row(rr, ha, hb, true);
            } else {
                for (int rr = row0; rr < nrow; rr += rstep) row(rr, ha, hb, false);
            }
        };
        // wave-uniform (the ballot is over the lanes still here: the chunk's owners)
        if (__builtin_amdgcn_ballot_w64(tail || remwave) != 0)
            band(std::true_type{});
        else
            band(std::false_type{});
        if (!MULTI) return;  // one chunk per wave (every level up to 2 048 px)
        ch += ch_step;
        if (ch >= ch_end) return;
        chunk(ch);
    }
}

// k_resize_cascade: the whole pyramid (levels 1 .. L-1) in ONE launch for small batches, where the seven
// per-level launches are seven latency chains of a few microseconds each (8 pairs: 58 us of 233 per step).
// One 512-thread workgroup per (horizontal strip, image).  Strip s computes at every level the rows the
// next level's rows of the strip need (its own rows, plus a halo its neighbours also compute) and stores
// the rows it owns; ownership partitions every level (host: resize_strips), so each output row is written
// exactly once, with the arithmetic of k_resize_rows (same taps, same vertical rounding).  Level 0's source
// rows are staged from the input like k_resize_rows; every later level reads the previous level's strip
// from LDS, ping-ponging between two buffers (A: level 0 staging and even levels, B: odd levels).
// tab: per (strip, level) int16 {computed lo, hi, owned lo, hi}; offB / offX: byte offsets of buffer B and
// of the per-level x selector table in the dynamic LDS.  (kCasNT threads; no derived level has more than kCasGroups
// groups: orbfe_kernels.h)
__global__ __launch_bounds__(kCasNT) void k_resize_cascade(Geo g, const uint8_t* __restrict__ in, int64_t in_pitch,
                                                        uint8_t* __restrict__ ws, const ResizeX* __restrict__ xt,
                                                        const ResizeY* __restrict__ yt, const int16_t* __restrict__ tab,
                                                        int offB, int offX, int* __restrict__ zero_word,
                                                        long long* __restrict__ prof) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    typedef __attribute__((address_space(3))) const uint32_t lds_u32;
    typedef __attribute__((address_space(3))) uint32_t lds_w32;
    const int strip = blockIdx.x, img = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), nwv = blockDim.x >> 6;
    if (zero_word && strip == 0 && img == 0 && t == 0) *zero_word = 0;
    // orbfe_debug_cascade_profile: wall-clock marks of the first thread, 32 per (image, strip): 0 start,
    // 1 staging issued + stored, 2 + l level l's rows may start (after its first barrier), 12 + l level l done
    long long* pm = prof ? prof + ((int64_t)img * gridDim.x + strip) * 32 : nullptr;
    auto mark = [&](int id) {
        if (pm && t == 0) pm[id] = (long long)wall_clock64();
    };
    mark(0);
    const int L = g.nlevels;
    const int16_t* st = tab + (int64_t)strip * L * 4;
    const uint32_t baseA = (uint32_t)(uintptr_t)(lds_u32*)rs_lds;
    const uint32_t baseB = baseA + (uint32_t)offB;
    // per group: v_perm selectors, then (a0, a1) weights; its first source column — double-buffered by level
    // parity: level l + 1's entries are loaded into registers while level l computes.  Every LDS and global
    // access goes through an address-space-qualified pointer: a generic one (an array of LDS pointers indexed
    // by the level's parity) compiles to flat loads, which count in vmcnt too — the item loop then waited for
    // the previous item's global stores before each table read.
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) v4u lds_u4;
    typedef __attribute__((address_space(3))) int lds_i32;
    typedef __attribute__((address_space(1))) const v4u glb_u4;
    auto u4 = [](v4u v) { return uint4{v.x, v.y, v.z, v.w}; };
    typedef __attribute__((address_space(1))) const uint32_t glb_u32;
    auto s_xa_of = [&](int par) { return (lds_u4*)(uintptr_t)(baseA + (uint32_t)offX + (uint32_t)(par * 32 * g.rs_ngrp)); };
    auto s_sx_of = [&](int par) {
        return (lds_i32*)(uintptr_t)(baseA + (uint32_t)offX + (uint32_t)(64 * g.rs_ngrp + par * 4 * g.rs_ngrp));
    };
    // groups per thread held in registers: prefetch / commit stage the selectors of a level's first kCasGroups
    // groups and no more, the row loop walks every group of the level; the host launches no cascade for a
    // geometry with a derived level of more groups (resize_strips, launch_resize_cascade)
    constexpr int kPre = kCasGroups / kCasNT;
    uint4 pq0[kPre], pq1[kPre];
    auto prefetch = [&](int l) {
        if (l >= g.nlevels) return;
        glb_u4* xg = (glb_u4*)(xt + g.lv[l].xtab_off);
        const int ng = (g.lv[l].w + 3) >> 2;
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const int gi = t + kCasNT * k;
            if (gi < ng) {
                pq0[k] = u4(xg[2 * gi]);
                pq1[k] = u4(xg[2 * gi + 1]);
            }
        }
    };
    auto commit = [&](int l) {
        lds_u4* sxa = s_xa_of(l & 1);
        lds_i32* ssx = s_sx_of(l & 1);
        const int ng = (g.lv[l].w + 3) >> 2;
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
            const int gi = t + kCasNT * k;
            if (gi < ng) {
                const uint4 q0 = pq0[k], q1 = pq1[k];
                auto sel = [&](uint32_t sx) { const uint32_t r = sx - q0.x; return r | ((r + 1) << 16) | 0x0c000c00u; };
                sxa[2 * gi] = v4u{sel(q0.x), sel(q0.z), sel(q1.x), sel(q1.z)};
                sxa[2 * gi + 1] = v4u{q0.y, q0.w, q1.y, q1.w};
                ssx[gi] = (int)(q0.x | ((q1.z - q0.x) << 24));  // sx0, and the 4th pixel's offset (wide levels)
            }
        }
    };
    prefetch(1);
    // ---- level 0 rows the strip's level 1 needs, staged as a flat dword run (k_resize_rows' staging)
    uint32_t src_base = baseA, src_sh;
    int src_row0, src_stride;
    {
        const LevelGeo& L1 = g.lv[1];
        const ResizeY* yb = yt + L1.ytab_off;
        const int c0 = st[4], c1 = st[5];
        const int ys_lo = yb[c0].sy0, ys_hi = yb[c1 - 1].sy1;
        const uintptr_t a0 = (uintptr_t)(in + (int64_t)img * in_pitch + (int64_t)ys_lo * g.W);
        src_sh = (uint32_t)(a0 & 3);
        glb_u32* gsrc = (glb_u32*)(a0 - src_sh);
        const int ndw = ((ys_hi - ys_lo) * g.W + g.W + (int)src_sh + 3) >> 2;
        lds_w32* s_src = (lds_w32*)(uintptr_t)baseA;
        for (int base = 0; base < ndw; base += kCasNT * kRsSlots / 2) {
            uint32_t v[kRsSlots / 2];
#pragma unroll
            for (int k = 0; k < kRsSlots / 2; ++k) {
                const int i = base + t + kCasNT * k;
                v[k] = i < ndw ? gsrc[i] : 0u;
            }
#pragma unroll
            for (int k = 0; k < kRsSlots / 2; ++k) {
                const int i = base + t + kCasNT * k;
                if (i < ndw) s_src[i] = v[k];
            }
        }
        src_row0 = ys_lo;
        src_stride = g.W;
    }
    mark(1);
    for (int l = 1; l < L; ++l) {
        const LevelGeo& Lv = g.lv[l];
        const int c0 = st[4 * l], c1 = st[4 * l + 1], o0 = st[4 * l + 2], o1 = st[4 * l + 3];
        const int ngrp = (Lv.w + 3) >> 2, nch = (ngrp + 63) >> 6;
        // x selectors / weights of the level (k_resize's per-group form), loaded during the previous level
        commit(l);
        prefetch(l + 1);
        const lds_u4* s_xa = s_xa_of(l & 1);
        const lds_i32* s_sx0 = s_sx_of(l & 1);
        const ResizeY* yb = yt + Lv.ytab_off;
        const uint32_t dst_base = (l & 1) ? baseB : baseA;
        __syncthreads();  // selectors staged; the source rows complete (previous level / staging)
        mark(2 + l);
        uint8_t* gdst = ws + (int64_t)img * g.ws_bytes + Lv.ws_off;
        const int pitch = Lv.pitch;
        // the level's fields in registers (read from the kernel arguments once, not per item)
        const int lv_wide = __builtin_amdgcn_readfirstlane(Lv.wide), lv_xvec = __builtin_amdgcn_readfirstlane(Lv.xvec),
                  lv_area = __builtin_amdgcn_readfirstlane(Lv.area);
        // items (row, chunk), row-major; wave wv takes items wv, wv + nwv, ...: row / chunk advanced
        // incrementally (uniform), no division per item.  (Measured slower here: k_resize_rows' row sets — a
        // wave walks consecutive rows of one chunk, reusing the previous row's taps — 39 -> 43 us at 8 pairs,
        // and two items per step with both items' reads issued before either waits, 39 -> 49 us.)
        // items = rows: wave wv takes rows c0 + wv, + nwv, ...; per row its y entry and offsets once (scalar),
        // then every 64-group chunk of the row (a uniform loop).  Measured (tools/cascade_profile.py, traces
        // at 8 pairs): (row, chunk) items 39.7 us, rows 36.4; also tried and slower: row sets with the previous
        // row's taps reused (43), two items per step with all reads issued first (49), the y entries staged in
        // LDS instead of scalar loads (42).
        for (int r = c0 + wv; r < c1; r += nwv) {
            const ResizeY y = yb[r];
            const uint32_t r0 = (uint32_t)((y.sy0 - src_row0) * src_stride), r1 = (uint32_t)((y.sy1 - src_row0) * src_stride);
            const uint32_t B0 = (uint32_t)y.b0 << 12, B1 = (uint32_t)y.b1 << 12;
            const bool own = r >= o0 && r < o1;
            const uint32_t lrow = dst_base + (uint32_t)((r - c0) * pitch);
            uint8_t* grow = gdst + (int64_t)r * pitch;
            for (int ch = 0; ch < nch; ++ch) {
                const int grp = ch * 64 + lane;
                if (grp < ngrp) {
                    const uint4 e = u4(s_xa[2 * grp]), aa = u4(s_xa[2 * grp + 1]);
                    const int sxp = s_sx0[grp];
                    const uint32_t d3 = (uint32_t)sxp >> 24;
                    const uint32_t lsrc = src_base + src_sh + (uint32_t)(sxp & 0xFFFFFF);
                    auto taps = [&](uint32_t roff, uint32_t (&h)[4]) {
                        const uint32_t A = lsrc + roff, o = A & 3u;
                        lds_u32* w = (lds_u32*)(uintptr_t)(A - o);
                        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
                        const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, o), d1 = __builtin_amdgcn_alignbyte(w2, w1, o);
                        h[0] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.x)),
                                                      __builtin_bit_cast(us2, aa.x), 0u, false);
                        h[1] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.y)),
                                                      __builtin_bit_cast(us2, aa.y), 0u, false);
                        h[2] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.z)),
                                                      __builtin_bit_cast(us2, aa.z), 0u, false);
                        h[3] = lv_wide ? resize_tap3(A + d3, aa.w)
                                       : __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(d1, d0, e.w)),
                                                                __builtin_bit_cast(us2, aa.w), 0u, false);
                    };
                    uint32_t h0[4], h1[4];
                    taps(r0, h0);
                    taps(r1, h1);
                    const int dx = 4 * grp;
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (__umulhi(h0[k] & ~15u, B0) + __umulhi(h1[k] & ~15u, B1) + 2) >> 2;
                    if (dx + 3 >= lv_xvec) {  // FixedPtCast<int, uchar, 22> past the last SIMD block
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (dx + k >= lv_xvec) v[k] = resize_tail(h0[k] * (B0 >> 12) + h1[k] * (B1 >> 12), lv_area);
                    }
                    const uint32_t px = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
                    *(lds_w32*)(uintptr_t)(lrow + (uint32_t)dx) = px;
                    if (own) *(uint32_t*)(grow + dx) = px;  // pitch padding past w
                }
            }
        }
        src_base = dst_base;
        src_sh = 0;
        src_row0 = c0;
        src_stride = pitch;
        __syncthreads();  // this level's rows complete before the next level reads them / the selectors change
        mark(12 + l);
    }
}

// ------------------------------------------------------------------------------- launchers
template <bool AL4>
static auto resize_rows_kernel(int threads) {
    switch (threads) {
        case 256: return k_resize_rows<false, AL4, 256>;
        case 320: return k_resize_rows<false, AL4, 320>;
        case 384: return k_resize_rows<false, AL4, 384>;
        case 448: return k_resize_rows<false, AL4, 448>;
        default: return k_resize_rows<false, AL4, 512>;
    }
}

hipError_t launch_resize(const Geo& g, int l, const uint8_t* in, int64_t in_pitch, uint8_t* ws, const ResizeX* xt,
                         const ResizeY* yt, int n_images, hipStream_t s, bool remainder_wave, int* zero_word) {
    const LevelGeo& L = g.lv[l];  // LDS sized for this level (its bands' source rows)
    dim3 grid((L.h + L.rs_rows - 1) / L.rs_rows, n_images);
    // k_resize_rows against the round-2 item-mapped kernel (profiles/r03/resize_rows_ab_r3f.log): 414 -> 394 us
    // per 256 pairs standalone, +0.8 % on the 4-handle step.
    // a level whose groups leave a last chunk of fewer than 40 (of 64) takes it in one remainder wave
    // (remainder_wave = false: never, every chunk row-uniform); at most 8 waves per row set, each walking several
    // chunks on rows wider than 2 048 px, so the block stays within __launch_bounds__(512)
    const int ngrp = (L.w + 3) / 4, rem = ngrp % 64;
    const int wg0 = (ngrp + 63) / 64;
    const int remw = (remainder_wave && ngrp >= 64 && wg0 <= 8 && rem > 0 && rem < 40) ? 1 : 0;
    const int wg = remw ? ngrp / 64 : wg0;
    const int wgl = std::min(wg, 8 - remw);
    const int sets = std::max(1, (4 - remw + wgl - 1) / wgl);  // >= 256 threads per block
    const int threads = 64 * (wgl * sets + remw);
    if (threads < 256 || threads > 512) return hipErrorInvalidConfiguration;
    // MULTI: a wave walks several 64-group chunks (levels wider than 2 048 px; always 8 waves, one set); the
    // one-chunk form is instantiated apart (the loop around it cost 3 % on KITTI, tools/dbg/mb_ab.sh, round 4),
    // per block size (the staging's strides) and per alignment of the source row stride
    const bool al4 = (l >= 2 ? g.lv[l - 1].pitch : g.W) % 4 == 0;
    const auto k = wg > wgl ? (al4 ? k_resize_rows<true, true, 512> : k_resize_rows<true, false, 512>)
                            : (al4 ? resize_rows_kernel<true>(threads) : resize_rows_kernel<false>(threads));
    hipLaunchKernelGGL(k, grid, dim3(threads), (size_t)L.rs_nsrc * L.rs_sp + 16, s, g, l, in, in_pitch, ws, xt, yt, wg,
                       remw, wgl, zero_word);
    return hipGetLastError();
}

hipError_t prepare_resize_cascade(int lds_bytes) { return raise_lds((const void*)k_resize_cascade, lds_bytes); }

hipError_t launch_resize_cascade(const Geo& g, const uint8_t* in, int64_t in_pitch, uint8_t* ws, const ResizeX* xt,
                                 const ResizeY* yt, const int16_t* strips, int n_strips, int off_b, int off_x,
                                 int lds_bytes, int n_images, hipStream_t s, int* zero_word, long long* prof) {
    if (g.nlevels < 2 || n_images <= 0) return hipSuccess;
    if (lds_bytes > lds_limit((const void*)k_resize_cascade)) return hipErrorInvalidConfiguration;  // prepare_resize_cascade was not run
    for (int l = 1; l < g.nlevels; ++l)
        if ((g.lv[l].w + 3) / 4 > kCasGroups) return hipErrorInvalidConfiguration;  // more groups than a strip stages
    hipLaunchKernelGGL(k_resize_cascade, dim3(n_strips, n_images), dim3(kCasNT), (size_t)lds_bytes, s, g, in, in_pitch, ws,
                       xt, yt, strips, off_b, off_x, zero_word, prof);
    return hipGetLastError();
}

}  // namespace orbfe
