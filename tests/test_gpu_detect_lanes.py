"""k_detect's lane decisions on the two-queue path, every image of detect_lane_cases.py: the B entries that the idle
lanes of A's last M step carry (and where the minTh fallback then starts) and the A emission that is skipped for a
pre-test half without an A pair, at window heights on both sides of a half.  The candidates row for
row, the keypoints and the descriptors against the oracle, one cell per wave (a single extraction) and four cells per
wave (a 32-image batch of mixed cases with the shape forced); the counters of orbfe_debug_detect_lanes against the
numpy restatement.

tests/test_detect_lane_cases_cpu.py shows on the CPU that every case has the queue lengths and the outcome it is
named for."""
import ctypes as C
import itertools

import numpy as np
import pytest

import detect_lane_cases as K
from oracle import oracle as O
from pyorbslam_amd._lib import call, ptr
from pyorbslam_amd.pyORBExtractor import ORBextractor

pytestmark = pytest.mark.gpu

SIZES = sorted({c.size for c in K.CASES})
BATCH_PAIRS = 16
BF, FX = 40.0, 100.0


def _lanes(handle):
    st = (C.c_int64 * 7)()
    call("orbfe_debug_detect_lanes", handle, st, 7)
    return list(st)


def _candidates(ex, cap):
    buf = np.zeros((cap, 3), np.int32)
    n = C.c_int32()
    call("orbfe_debug_candidates", ex.handle, 0, ptr(buf), cap, C.byref(n))
    return [tuple(r) for r in buf[:n.value].tolist()]


def _assert_output(kps, desc, ref, what):
    okps, odesc = ref
    assert len(kps) == len(okps), f"{what}: {len(kps)} keypoints, the oracle keeps {len(okps)}"
    assert kps.tobytes() == okps.tobytes(), f"{what}: keypoints differ"
    assert np.array_equal(np.asarray(desc).reshape(-1, 32), odesc.reshape(-1, 32)), f"{what}: descriptors differ"


def _assert_counters(got, cases, what):
    exp = [sum(v) for v in zip(*(K.expected_counters(c) for c in cases))]
    names = ("cells", "one-pass cells", "fallback cells", "A steps that carried", "B entries carried", "B steps run",
             "A emissions skipped")
    print(what, dict(zip(names, got)))
    assert got == exp, f"{what}: {dict(zip(names, got))}, the restatement counts {dict(zip(names, exp))}"
    # B steps run = ceil((|B| - kB) / 64) over the fallback cells
    assert got[5] == sum(-(-(r["B"] - r["kb"]) // 64) for c in cases for r in K.counts(c) if r["fallback"]), what


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_single_extraction(size):
    """One cell per wave: every case of the geometry on one handle, in turn."""
    ex = ORBextractor(**K.PARAMS)
    for case in (c for c in K.CASES if c.size == size):
        kps, desc = ex.extract(K.image(case))
        exp = [tuple(r) for r in K.candidates(case).tolist()]
        got = _candidates(ex, len(exp) + 8)
        n = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        assert got == exp, f"{case.name}: {len(got)} candidates against {len(exp)}, first difference at row {n}"
        _assert_output(kps, desc, K.ref(case), case.name)
        _assert_counters(_lanes(ex.handle), [case], case.name)
        kps, desc = ex.extract(K.image(case))   # the counting re-run left the stage's output as it was
        _assert_output(kps, desc, K.ref(case), f"{case.name}: again")


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_batch_four_cells_per_wave(size):
    """The geometry's cases, repeated and mixed with a flat image, as the 32 images of one enqueue; then the detect
    stage again with four cells per wave forced (a wave's cells share its LDS: what one cell's queues leave behind
    must not reach the next) and the later stages re-run on its output."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd.batch import StereoFrontEnd
    cases = [c for c in K.CASES if c.size == size]
    w, h = size
    cyc = itertools.cycle(cases)
    slots = [next(cyc) for _ in range(2 * BATCH_PAIRS)]
    images = [K.image(c) for c in slots]
    refs = [K.ref(c) for c in slots]
    flat = np.full((h, w), K.BG, np.uint8)
    images[5], refs[5] = flat, (np.zeros(0, O.KP_DTYPE), np.zeros((0, 32), np.uint8))
    fe = StereoFrontEnd(w, h, max_pairs=BATCH_PAIRS, lanes=1, **K.PARAMS)
    fe.enqueue(torch.from_numpy(np.stack(images)).cuda(), BATCH_PAIRS, bf=BF, fx=FX)

    def check(what):
        assert fe.overflow() == 0, what
        for s, (c, ref) in enumerate(zip(slots, refs)):
            kps, desc = fe.fetch_image(s)
            _assert_output(kps, desc, ref, f"{what}, slot {s} ({'flat' if s == 5 else c.name})")

    check(f"{w} x {h}: batch")
    ms = C.c_float()
    for variant in (4, 5):      # four cells per wave, one cell per wave
        call("orbfe_microbench", fe.handle, 1, variant, 1, C.byref(ms))
        for later in (2, 3, 4):
            call("orbfe_microbench", fe.handle, later, 0, 1, C.byref(ms))
        check(f"{w} x {h}: detect variant {variant}")
    # the counters of the whole batch, in both launch shapes (the entry point compares them)
    D = K.model()
    fc = [D.lane_counts(*D.maps(flat), c, 1 << 20, K.INI, K.MIN) for c in K.grid(size)]
    assert all(r["A"] == r["B"] == 0 and r["fallback"] for r in fc)
    flat_counters = [len(fc), 0, len(fc), 0, 0, 0, sum(r["a_skipped"] for r in fc)]
    exp = [sum(v) for v in zip(flat_counters, *(K.expected_counters(c) for s, c in enumerate(slots) if s != 5))]
    got = _lanes(fe.handle)
    assert got == exp, (got, exp)
