"""Geometries of tests/test_gpu_resize_cascade.py and a restatement, in Python and in the host's integer
arithmetic, of the rules that shape a k_resize_cascade launch: resize_strips (the rows a strip owns and computes at
every level, the two ping-pong buffers, the selector table, the LDS total), cascade_strips and prepare_pyramid's
search for a strip count that fits (orbfe_host.hip), and the level-0 run a strip stages (orbfe_resize.hip).
tests/test_resize_cascade_cases_cpu.py uses the restatement to show that the geometries reach what they are
chosen for."""
from __future__ import annotations

import functools

from oracle.oracle import OracleExtractor
from resize_rows_cases import LDS_LIMIT, noise, params, xvec, ytab

CAS_THREADS = 1024         # kCasNT
CAS_WAVES = CAS_THREADS // 64
CAS_GROUPS = 1024             # kCasGroups: the 4-pixel groups of a level whose x selectors the kernel stages
PASS_DWORDS = CAS_THREADS * 16 // 2  # kCasNT * kRsSlots / 2: staged dwords per pass of the block
CASCADE_IMAGES = 32        # kCascadeImages: enqueues of fewer images take the cascade
AUTO = -1                  # a case's S: the automatic strip count of one image


# ---- the host's rules ------------------------------------------------------------------------------------------
def case_params(nlevels: int, scale: float, simd: int, nfeatures: int = 300) -> dict:
    return dict(params(nlevels, simd), scaleFactor=float(scale), nfeatures=int(nfeatures))


@functools.lru_cache(maxsize=None)
def level_sizes(h: int, w: int, nlevels: int, scale: float) -> tuple:
    """((w_l, h_l)); resize_rows_cases.level_sizes at a scale factor of the case's choice."""
    return tuple(OracleExtractor(**case_params(nlevels, scale, 16)).level_sizes(w, h))


def pitch(wl: int) -> int:
    return (wl + 15) & ~15


def groups(wl: int) -> int:
    return (wl + 3) // 4


@functools.lru_cache(maxsize=None)
def _ytabs(h: int, w: int, nlevels: int, scale: float) -> tuple:
    sizes = level_sizes(h, w, nlevels, scale)
    return (None,) + tuple(tuple(a.tolist() for a in ytab(sizes[l - 1][1], sizes[l][1])) for l in range(1, nlevels))


@functools.lru_cache(maxsize=None)
def resize_strips(h: int, w: int, nlevels: int, scale: float, S: int):
    """resize_strips: None where the host returns null, else own[l][0 .. S], clo[l][k], chi[l][k] (l >= 1), the
    buffer sizes A and B, off_b, off_x and the LDS total."""
    sizes = level_sizes(h, w, nlevels, scale)
    L, top = nlevels, nlevels - 1
    if L < 2 or S < 1 or S > sizes[top][1]:
        return None
    if max(groups(sizes[l][0]) for l in range(1, L)) > CAS_GROUPS:
        return None
    yt = _ytabs(h, w, nlevels, scale)
    own = [[0] * (S + 1) for _ in range(L)]
    clo = [[0] * S for _ in range(L)]
    chi = [[0] * S for _ in range(L)]
    own[top] = [k * sizes[top][1] // S for k in range(S + 1)]
    for l in range(top - 1, 0, -1):
        own[l][S] = sizes[l][1]
        for k in range(1, S):
            own[l][k] = yt[l + 1][0][own[l + 1][k]]
    for k in range(S):
        clo[top][k], chi[top][k] = own[top][k], own[top][k + 1]
        if chi[top][k] <= clo[top][k]:
            return None
        for l in range(top - 1, 0, -1):
            clo[l][k] = min(own[l][k], yt[l + 1][0][clo[l + 1][k]])
            chi[l][k] = max(own[l][k + 1], yt[l + 1][1][chi[l + 1][k] - 1] + 1)
    A = B = 0
    for k in range(S):
        ys_lo, ys_hi = yt[1][0][clo[1][k]], yt[1][1][chi[1][k] - 1]
        A = max(A, (ys_hi - ys_lo + 1) * w + 8)
        for l in range(1, L):
            b = (chi[l][k] - clo[l][k]) * pitch(sizes[l][0])
            if l & 1:
                B = max(B, b)
            else:
                A = max(A, b)
    a16 = lambda v: (v + 16 + 15) & ~15
    rs_ngrp = max([4] + [(groups(sizes[l][0]) + 3) & ~3 for l in range(1, L)])
    off_b = a16(A)
    off_x = off_b + a16(B)
    lds = off_x + rs_ngrp * 72
    if lds > LDS_LIMIT:
        return None
    return dict(S=S, own=own, clo=clo, chi=chi, A=A, B=B, off_b=off_b, off_x=off_x, lds=lds, sizes=sizes, yt=yt)


def cascade_strips(htop: int, nlevels: int, cus: int, n: int) -> int:
    """cascade_strips: the first strip count tried for an enqueue of n images, -1 for the per-level launches."""
    if n >= CASCADE_IMAGES or nlevels < 2:
        return -1
    return max(4, min(cus // max(n, 1), max(4, htop // 3)))


def chosen_strips(h: int, w: int, nlevels: int, scale: float, cus: int, n: int) -> int:
    """prepare_pyramid's search (S += 4 until a count fits or passes the top level's rows): the strip count of
    the cascade an n-image enqueue takes, 0 when it takes the per-level launches."""
    htop = level_sizes(h, w, nlevels, scale)[-1][1]
    S = cascade_strips(htop, nlevels, cus, n)
    while S > 0:
        if resize_strips(h, w, nlevels, scale, S):
            return S
        if S > htop:
            break
        S += 4
    return 0


def forced_strips(h: int, w: int, nlevels: int, scale: float, S: int) -> int:
    """The strip count orbfe_microbench (stage 0, variant 100 + S) runs: S, or the next of S + 4, S + 8, ... that
    fits; 0 when it refuses."""
    htop = level_sizes(h, w, nlevels, scale)[-1][1]
    if S <= 0 or S > htop:
        return 0
    while not resize_strips(h, w, nlevels, scale, S):
        if S > htop:
            return 0
        S += 4
    return S


def staged_run(h: int, w: int, nlevels: int, scale: float, S: int, k: int, img: int = 0) -> dict:
    """The level-0 run strip k of image img stages (k_resize_cascade), for a batch tensor on a 4-byte boundary
    whose images stand w * h bytes apart."""
    cs = resize_strips(h, w, nlevels, scale, S)
    ys_lo, ys_hi = cs["yt"][1][0][cs["clo"][1][k]], cs["yt"][1][1][cs["chi"][1][k] - 1]
    src_sh = (img * w * h + ys_lo * w) % 4
    ndw = ((ys_hi - ys_lo) * w + w + src_sh + 3) >> 2
    return dict(ys_lo=ys_lo, ys_hi=ys_hi, src_sh=src_sh, ndw=ndw, passes=-(-ndw // PASS_DWORDS))


def level_kind(h: int, w: int, nlevels: int, scale: float, l: int) -> str:
    """'area' (the exact 2x step), 'wide' (a group's 4th pixel has a tap window of its own) or 'linear'."""
    import numpy as np
    (sw, sh), (dw, dh) = level_sizes(h, w, nlevels, scale)[l - 1:l + 1]
    if sw == 2 * dw and sh == 2 * dh:
        return "area"
    fx = ((np.arange(dw) + 0.5) * (1.0 / (dw / sw)) - 0.5).astype(np.float32)
    sx = np.clip(np.floor(fx).astype(np.int64), 0, sw - 1)
    sx = np.concatenate([sx, np.full(4, sw - 1)])
    g0 = sx[0:groups(dw) * 4:4]
    return "wide" if ((sx[3:3 + 4 * len(g0):4] - g0) > 6).any() else "linear"


def tail_groups(h: int, w: int, nlevels: int, scale: float, simd: int, l: int) -> list:
    """Groups of level l with a pixel in the scalar tail."""
    (sw, sh), (dw, dh) = level_sizes(h, w, nlevels, scale)[l - 1:l + 1]
    xv = xvec(sw, sh, dw, dh, simd)
    return [g for g in range(groups(dw)) if 4 * g + 3 >= xv]


# ---- the cases: (h, w, nlevels, scaleFactor, simd, S) on noise(h, w) -------------------------------------------
# What each list is there for is asserted in tests/test_resize_cascade_cases_cpu.py (CASES_FOR there).  Three
# things the restatement shows that the lists take into account:
#  * a strip owns a level's rows from the first source row of its next-level rows on, so the rows it computes
#    never begin before the rows it owns: a halo lies above a strip's last owned row only, never below its first;
#  * with steps above 1 no sy0 / sy1 is clipped at the image border (the last row's sy1 is the source's last row
#    at most), so the first and last strips are the ones whose ranges end at rows 0 and h - 1;
#  * a step of 1.9 keeps a group's 4th pixel within 6 source columns of its first, so it is not `wide`: wide
#    steps lie between about 2.0 (not the exact 2x of `area`) and 3.0, here 2.2 and 3.0; 1.9 stays as the largest
#    step of the ordinary tap window.
STAGING = [(96, 131, 3, 1.2, 16, 8),     # runs under 1 024 dwords (src_sh 0 and 2)
           (128, 256, 2, 1.2, 16, 1),    # 8 192 dwords: one pass, filled
           (145, 226, 2, 1.2, 16, 1),    # 8 193 dwords
           (230, 300, 2, 1.2, 16, 1)]    # 17 250 dwords: three passes
STRIPS = [(97, 129, 3, 1.2, 16, 67),     # one top row per strip; every src_sh on image 0
          (96, 307, 3, 1.2, 16, 5),      # strips of 16, 17 and 13 rows at a level; every src_sh
          (96, 310, 4, 1.2, 16, 3)]      # the middle strip computes rows past its own at every level below the top
GROUPS = [(96, 307, 3, 1.2, 16, 5),      # level 1: 256 px, 64 groups
          (96, 310, 4, 1.2, 16, 3),      # level 1: 258 px, 65 groups
          (150, 309, 3, 1.2, 16, 4),     # 258 px again, every src_sh in four strips
          (40, 40, 4, 2.0, 16, 4)]       # levels of 3 and 2 groups
STEPS = [(40, 40, 4, 2.0, 0, 1), (40, 40, 4, 2.0, 16, 4), (140, 140, 3, 2.0, 32, 3),  # area
         (200, 200, 3, 2.2, 16, 4), (300, 300, 3, 3.0, 16, 33), (300, 300, 3, 3.0, 0, 1),  # wide
         (200, 200, 3, 1.9, 32, 4),
         (96, 307, 3, 1.2, 0, 5), (96, 307, 3, 1.2, 32, 5),
         (128, 128, 12, 1.2, 16, 17), (128, 128, 12, 1.2, 16, AUTO)]  # a deep pyramid
WIDTH = [(120, 4915, 3, 1.2, 16, AUTO),  # level 1: 4 096 px, CAS_GROUPS groups
         (120, 4917, 3, 1.2, 16, AUTO),  # 4 098 px, one group more
         (140, 8200, 3, 2.0, 16, AUTO),  # area, 1 025 groups
         (100, 12000, 2, 3.0, 16, AUTO)]  # the longest source rows a cascade takes
SEARCH = [(300, 4800, 5, 1.2, 16, AUTO),  # the first count does not fit the LDS, a later one does
          (300, 4800, 6, 1.2, 16, AUTO),  # none fits
          (40, 40, 5, 2.0, 16, AUTO)]     # a top level of 2 rows: fewer than the smallest automatic count
ORDINARY = [(96, 307, 3, 1.2, 16, AUTO), (128, 128, 12, 1.2, 16, AUTO), (300, 300, 3, 3.0, 16, AUTO)]
PATHS = SEARCH + ORDINARY + WIDTH[:2]
ALL = sorted(set(STAGING + STRIPS + GROUPS + STEPS + WIDTH + SEARCH + ORDINARY))
BATCH = (97, 129, 3)    # W * H = 1 mod 4: every image of a batch at another misalignment
# sweep_cases.mixed_batch (seed0, first) of the two batches: natural / noise / lattice and noise / lattice / binary,
# every image with keypoints above level 0 and different from the image it replaces
BATCH_FIRST, BATCH_SECOND = (7000, 0), (8000, 1)
BATCH_STRIPS = (5, 67, 1)  # forced in turn, the input replaced before each; 67 = the rows of the top level
NOMINAL_CUS = 256       # the CPU tests' CU count (an MI355X); the GPU tests ask the device


def nfeatures(case) -> int:
    """300, and 2 000 for the very wide images (at their aspect the oracle's record buffer is too small for 300)."""
    return 2000 if case[1] > 4000 else 300


def case_id(case) -> str:
    h, w, nlevels, scale, simd, S = case
    return f"{w}x{h}-L{nlevels}-x{scale}-simd{simd}-S{'auto' if S == AUTO else S}"


@functools.lru_cache(maxsize=None)
def reference_pyramid(h: int, w: int, nlevels: int, scale: float, simd: int) -> tuple:
    """The oracle's pyramid of noise(h, w); shared among the tests, read-only."""
    ox = OracleExtractor(**case_params(nlevels, scale, simd, nfeatures((h, w))))
    ox.extract(noise(h, w))
    return tuple(ox.pyramid())
