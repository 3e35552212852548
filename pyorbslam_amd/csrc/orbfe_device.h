// orbfe_device.h — device helpers that more than one stage of the extractor uses (orbfe_resize.hip,
// orbfe_detect.hip, orbfe_kernels.hip), and the 256-bit Hamming distance and wave-uniform lane reads the matcher
// kernels share.  A helper of one stage lives with that stage.
#pragma once

#include <hip/hip_runtime.h>

#include "orbfe_common.h"

namespace orbfe {

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// Buffer resource for a wave-uniform base pointer: loads take a 32-bit lane offset (no 64-bit address
// arithmetic per lane).  Dword 3 = 0x00020000, the gfx9 raw-buffer format word.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* p) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0, 0x7FFFFFFF, 0x00020000);
}

// Buffer resource over the wave-uniform p, bounded to nbytes bytes.  The halves go through uint32_t: the
// builtin returns int, and a sign-extended low half OR-ed into the 64-bit address corrupts its high bits
// whenever bit 31 of the address is set.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bounded_rsrc(const void* p, uint32_t nbytes) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane(nbytes), 0x00020000);
}

// Buffer resource over the dword-aligned address at or below the wave-uniform p, bounded to
// bias + nbytes bytes; *bias = p's misalignment, so byte i of p sits at resource offset bias + i and a
// dword-aligned load covering it starts at (bias + i) & ~3 (never below the resource base).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t aligned_rsrc(const void* p, uint32_t nbytes, uint32_t* bias) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    *bias = lo & 3u;
    const uint32_t nb = __builtin_amdgcn_readfirstlane(nbytes);  // wave-uniform: an SGPR resource, never waterfalled
    return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | (lo & ~3u)), 0, nb + (lo & 3u),
                                             0x00020000);
}

// Two wave-wide sums at once (wave-uniform results): DPP quad_perm / row_ror sums inside each 16-lane row, then the
// four row sums through v_readlane (no LDS-crossbar round trips).  The DPP steps of the two interleave, so neither
// waits out the other's VALU-write -> DPP-read hazard (the s_nop the compiler puts between dependent DPP adds).
__device__ __forceinline__ void wave_sum2(int& a, int& b) {
    a += __builtin_amdgcn_update_dpp(0, a, 0xB1, 0xF, 0xF, false);
    b += __builtin_amdgcn_update_dpp(0, b, 0xB1, 0xF, 0xF, false);
    a += __builtin_amdgcn_update_dpp(0, a, 0x4E, 0xF, 0xF, false);
    b += __builtin_amdgcn_update_dpp(0, b, 0x4E, 0xF, 0xF, false);
    a += __builtin_amdgcn_update_dpp(0, a, 0x124, 0xF, 0xF, false);
    b += __builtin_amdgcn_update_dpp(0, b, 0x124, 0xF, 0xF, false);
    a += __builtin_amdgcn_update_dpp(0, a, 0x128, 0xF, 0xF, false);
    b += __builtin_amdgcn_update_dpp(0, b, 0x128, 0xF, 0xF, false);
    a = __builtin_amdgcn_readlane(a, 0) + __builtin_amdgcn_readlane(a, 16) + __builtin_amdgcn_readlane(a, 32) +
        __builtin_amdgcn_readlane(a, 48);
    b = __builtin_amdgcn_readlane(b, 0) + __builtin_amdgcn_readlane(b, 16) + __builtin_amdgcn_readlane(b, 32) +
        __builtin_amdgcn_readlane(b, 48);
}

__device__ __forceinline__ int reflect101(int p, int n) {
    // one reflection suffices: every caller overshoots by less than n
    p = p < 0 ? -p : p;
    return p >= n ? 2 * n - 2 - p : p;
}

// cv::borderInterpolate(BORDER_REFLECT_101) for any overshoot: the reflection iterates (period 2 n - 2), a
// 1-pixel side maps everything to 0 — the 19-pixel padding of levels up to 19 px (copyMakeBorder,
// ORBextractor.cpp:1122-1128)
__device__ __forceinline__ int reflect101_iter(int p, int n) {
    if (n == 1) return 0;
    const int per = 2 * n - 2;
    p = (p < 0 ? -p : p) % per;
    return p >= n ? per - p : p;
}

__device__ __forceinline__ const uint8_t* level_ptr(const Geo& g, int l, const uint8_t* in, int64_t in_pitch,
                                                    const uint8_t* ws, int img, int* stride) {
    if (l == 0) {
        *stride = g.W;
        return in + (int64_t)img * in_pitch;
    }
    *stride = g.lv[l].pitch;
    return ws + (int64_t)img * g.ws_bytes + g.lv[l].ws_off;
}

// A FAST cell's geometry as dword scalar loads (s_load) and SALU unpacking: reading the int16 fields
// directly compiles to a per-lane global_load_ushort whose vmcnt wait also drains the next cell's ROI
// prefetch — a full memory round trip per cell on the critical path.
__device__ __forceinline__ CellGeo load_cell(const CellGeo* __restrict__ cells, int c) {
    static_assert(sizeof(CellGeo) == 20, "CellGeo layout: 5 dwords");
    const uint32_t* p = (const uint32_t*)(cells + c);
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
    CellGeo cg;
    cg.level = (int16_t)(w0 & 0xFFFFu);
    cg.kw = (int16_t)(w0 >> 16);
    cg.x0 = (int16_t)(w1 & 0xFFFFu);
    cg.y0 = (int16_t)(w1 >> 16);
    cg.x1 = (int16_t)(w2 & 0xFFFFu);
    cg.y1 = (int16_t)(w2 >> 16);
    cg.slot_off = (int)w3;
    cg.slot_cap = (int)w4;
    return cg;
}

// A packed level key's coordinates ((x + y * w) | score << 24, kKeyXYBits): y = mul_hi(xy, mag) >> sh is
// floor(xy / w) for every xy < 2^24 (mag = ceil(2^(31 + s) / w), sh = s - 1, s = ceil(log2 w): the error term
// xy * (mag * w - 2^(31 + s)) < 2^24 * w < 2^(31 + s)), then x = xy - y * w (both < 2^24: v_mad_u32_u24).
struct KeyDiv {
    uint32_t w, mag, sh;
};
__device__ __forceinline__ KeyDiv key_div(const LevelGeo& L) {
    return KeyDiv{(uint32_t)__builtin_amdgcn_readfirstlane(L.w), (uint32_t)__builtin_amdgcn_readfirstlane((int)L.kmag),
                  (uint32_t)__builtin_amdgcn_readfirstlane(L.ksh)};
}
__device__ __forceinline__ void key_xy(uint32_t k, KeyDiv kd, int& x, int& y) {
    const uint32_t xy = k & 0xFFFFFFu;
    const uint32_t q = __umulhi(xy, kd.mag) >> kd.sh;
    y = (int)q;
    x = (int)(xy - __umul24(q, kd.w));
}

// XCD-aware remap of a (gridDim.x, gridDim.y) grid.  Hardware block i (flattened, x fastest) runs on
// XCD i % 8; the remap hands each XCD a contiguous run of logical blocks, so neighbouring tiles / cells /
// bands — which share halo rows and partly used cache lines — meet in the same L2 instead of being
// fetched from HBM by several XCDs.  Wave-uniform results (SGPRs).
__device__ __forceinline__ void xcd_block(int& bx, int& by) {
    const int nb = gridDim.x * gridDim.y, hw = blockIdx.y * gridDim.x + blockIdx.x, per = nb >> 3;
    const int lb = hw < 8 * per ? (hw & 7) * per + (hw >> 3) : hw;
    by = __builtin_amdgcn_readfirstlane(lb / (int)gridDim.x);
    bx = __builtin_amdgcn_readfirstlane(lb - by * (int)gridDim.x);
}

// Block-wide exclusive scan of a[0..n) in LDS, in place; returns the total.  The first 256 threads own
// contiguous chunks, so prefixes follow array order; further threads (blocks of up to 1024) only take
// part in the barriers.  tmp: 257 ints of LDS.
__device__ inline int block_excl_scan(int* a, int n, int* tmp) {
    const int t = threadIdx.x;
    const int per = (n + 255) >> 8;
    const int b = t < 256 ? min(t * per, n) : n, e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; ++i) s += a[i];
    if (t < 256) tmp[t] = s;
    __syncthreads();
    if (t < 64) {
        const int v0 = tmp[4 * t], v1 = tmp[4 * t + 1], v2 = tmp[4 * t + 2], v3 = tmp[4 * t + 3];
        const int tot = v0 + v1 + v2 + v3;
        int inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o, 64);
            if (t >= o) inc += y;
        }
        const int ex = inc - tot;
        tmp[4 * t] = ex;
        tmp[4 * t + 1] = ex + v0;
        tmp[4 * t + 2] = ex + v0 + v1;
        tmp[4 * t + 3] = ex + v0 + v1 + v2;
        if (t == 63) tmp[256] = inc;
    }
    __syncthreads();
    int run = t < 256 ? tmp[t] : 0;
    for (int i = b; i < e; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    const int total = tmp[256];
    __syncthreads();
    return total;
}

__device__ __forceinline__ int lanes_below(uint64_t b) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0));
}

// Hamming distance of two 256-bit ORB descriptors, each as two uint4: (a0, a1) against (b0, b1)
__device__ __forceinline__ unsigned hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// lane j's value of v, j wave-uniform
__device__ __forceinline__ unsigned lane_value(unsigned v, int j) {
    return (unsigned)__builtin_amdgcn_readlane((int)v, j);
}
__device__ __forceinline__ double lane_value(double v, int j) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = lane_value((unsigned)b, j), hi = lane_value((unsigned)(b >> 32), j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

}  // namespace orbfe
