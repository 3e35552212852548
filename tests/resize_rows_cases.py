"""Geometries of tests/test_gpu_resize_rows.py and a restatement, in Python, of the rules by which the host
shapes a k_resize_rows launch (launch_resize in orbfe_resize.hip, the band and y-table rules of orbfe_host.hip,
the end of the vertical pass's vector span).  tests/test_resize_rows_cases_cpu.py uses the restatement to show
that the geometries reach the kernel's paths they are chosen for."""
from __future__ import annotations

import functools

import numpy as np

from oracle.oracle import OracleExtractor

PARAMS = dict(nfeatures=300, scaleFactor=1.2, iniThFAST=20, minThFAST=7)
SIMD_MODES = (0, 32)       # the two modes of test_resize_simd_modes: no vector span at all, 32-lane steps
BAND_ROWS = 16             # kRsRows
LDS_LIMIT = 150 * 1024
PASS_SLOTS = 24            # kRsRowSlots: staged dwords per thread and pass

# (h, w, nlevels): see CASES_FOR in tests/test_resize_rows_cases_cpu.py for what each is there for
STRIDES = [(58, 300, 3), (58, 301, 3), (58, 302, 3), (58, 303, 3)]
TAILS = [(58, 300, 3), (58, 496, 3), (58, 308, 3), (58, 491, 3), (56, 2461, 3)]
BLOCKS = [(58, 300, 3), (56, 624, 3), (56, 840, 3), (56, 2100, 3), (56, 2200, 3), (56, 2461, 3)]
SLOTS = [(97, 1200, 2), (97, 1229, 2)]
HEIGHTS = [(58, 300, 3), (59, 300, 3), (56, 300, 3), (56, 496, 3), (97, 129, 3)]
BATCH = (97, 129, 3)  # tall enough for keypoints above level 0; W * H = 1 mod 4: images off the dword grid
ALL = sorted(set(STRIDES + TAILS + BLOCKS + SLOTS + HEIGHTS))


def params(nlevels: int, simd: int = 16) -> dict:
    return dict(PARAMS, nlevels=int(nlevels), resize_simd_lanes=int(simd))


def noise(h: int, w: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference_pyramid(h: int, w: int, nlevels: int, simd: int) -> tuple:
    """The oracle's pyramid of noise(h, w); shared among the tests, read-only."""
    ox = OracleExtractor(**params(nlevels, simd))
    ox.extract(noise(h, w))
    return tuple(ox.pyramid())


def level_sizes(h: int, w: int, nlevels: int) -> list:
    return OracleExtractor(**params(nlevels)).level_sizes(w, h)  # [(w_l, h_l)]


# ---- the host's rules ------------------------------------------------------------------------------------------
def xvec(sw: int, sh: int, dw: int, dh: int, simd: int) -> int:
    """End of the vertical pass's vector span (resize_tables): pixels from here on take the scalar tail."""
    if sw == 2 * dw and sh == 2 * dh:  # the INTER_AREA fast path
        lanes = simd // 2
        return dw // lanes * lanes if lanes else 0
    xv = 0
    if simd > 0:
        while xv <= dw - simd:
            xv += simd
        while xv < dw - simd // 2:
            xv += simd // 2
    return xv


def ytab(sh: int, dh: int) -> tuple:
    """(sy0, sy1) per output row (resize_tables; float32 where the host rounds to float)."""
    if sh == 2 * dh:
        d = np.arange(dh)
        return 2 * d, 2 * d + 1
    scale = 1.0 / (dh / sh)
    fy = ((np.arange(dh) + 0.5) * scale - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    return np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)


def launch_shape(wl: int, remainder_wave: bool = True) -> dict:
    """launch_resize's block of a level wl pixels wide."""
    ngrp = (wl + 3) // 4
    rem, wg0 = ngrp % 64, (ngrp + 63) // 64
    remw = 1 if (remainder_wave and ngrp >= 64 and wg0 <= 8 and 0 < rem < 40) else 0
    wg = ngrp // 64 if remw else wg0
    wgl = min(wg, 8 - remw)
    sets = max(1, (4 - remw + wgl - 1) // wgl)
    threads = 64 * (wgl * sets + remw)
    assert 256 <= threads <= 512
    return dict(ngrp=ngrp, remw=remw, wg=wg, wgl=wgl, sets=sets, threads=threads, multi=wg > wgl,
                last_chunk=ngrp - 64 * (wg0 - 1))


def bands(sizes: list, l: int, base_mod4: int = 0) -> list:
    """The bands of level l >= 1: per band its rows, the staged run's misalignment sh0 and dwords (k_resize_rows),
    for an image whose first byte stands base_mod4 past a dword boundary."""
    (sw, sh), (dw, dh) = sizes[l - 1], sizes[l]
    stride = sw if l == 1 else (sw + 15) & ~15
    sy0, sy1 = ytab(sh, dh)
    rows = BAND_ROWS
    while True:
        nsrc = max(int(sy1[min(d + rows, dh) - 1] - sy0[d] + 1) for d in range(0, dh, rows))
        if nsrc * stride + 16 <= LDS_LIMIT or rows == 1:
            break
        rows //= 2
    out = []
    for d in range(0, dh, rows):
        nrow = min(rows, dh - d)
        lo, hi = int(sy0[d]), int(sy1[d + nrow - 1])
        sh0 = ((base_mod4 if l == 1 else 0) + lo * stride) % 4
        out.append(dict(nrow=nrow, sh0=sh0, ndw=((hi - lo) * stride + sw + sh0 + 3) >> 2))
    return out


def set_rows(nrow: int, nset: int) -> list:
    """Rows of each row set of a band (consecutive runs of ceil(nrow / nset))."""
    per = (nrow + nset - 1) // nset
    return [max(0, min(s * per + per, nrow) - s * per) for s in range(nset)]


def tail_groups(sizes: list, l: int, simd: int) -> list:
    """Indices of the 4-pixel groups of level l with a pixel in the scalar tail."""
    (sw, sh), (dw, dh) = sizes[l - 1], sizes[l]
    xv = xvec(sw, sh, dw, dh, simd)
    return [g for g in range((dw + 3) // 4) if 4 * g + 3 >= xv]
