"""k_detect's arithmetic, every image of detect_fast_cases.py: the 16 arcs of the exact M in every instantiation a
geometry can reach, both polarities and both pixels of a pair; the threshold comparisons and their ends (0, 1, 254,
255, minTh > iniTh, one threshold); the eight NMS neighbours of both pixels and their ties; the detection window's
borders, between cells and at the level's edge, at every remainder of the last quad; and the one-pass path with its
minTh list copied out and discarded.  The candidates row for row, the keypoints and the descriptors against the
oracle, one cell per wave (a single extraction) and in 32-image batches with both launch shapes forced.

tests/test_detect_fast_cases_cpu.py shows on the CPU that every case stands on the decision it is named for."""
import ctypes as C

import numpy as np
import pytest

import detect_fast_cases as K
from oracle import oracle as O
from pyorbslam_amd._lib import call
from pyorbslam_amd.pyORBExtractor import ORBextractor
from test_gpu_detect_lanes import BATCH_PAIRS, BF, FX, _assert_output, _candidates

pytestmark = pytest.mark.gpu

SIZES = sorted({c.size for c in K.CASES})
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
NONE = (np.zeros(0, O.KP_DTYPE), np.zeros((0, 32), np.uint8))


def _groups(size):
    """The geometry's cases by threshold pair: one extractor each."""
    out = {}
    for c in K.CASES:
        if c.size == size:
            out.setdefault(c.th, []).append(c)
    return out


def _one_pass_cells(handle):
    st = (C.c_int64 * 3)()
    call("orbfe_debug_detect_stats", handle, st)
    return st[0], st[1]


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_single_extraction(size):
    """One cell per wave: every case of the geometry in turn, on one handle per threshold pair."""
    for th, cases in _groups(size).items():
        ex = ORBextractor(**cases[0].params)
        for case in cases:
            kps, desc = ex.extract(case.img)
            exp = [tuple(r) for r in K.candidates(case).tolist()]
            try:
                got = _candidates(ex, len(exp) + 64)
            except Exception as e:     # more candidates than the buffer holds
                raise AssertionError(f"{case.name}: {len(exp)} candidates expected: {e}") from e
            n = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
            assert got == exp, (f"{case.name}: {len(got)} candidates against {len(exp)}, first difference at row {n}: "
                                f"{got[n:n + 1]} against {exp[n:n + 1]}")
            _assert_output(kps, desc, K.ref(case), case.name)
            if th[1] < th[0]:
                cells, one_pass = _one_pass_cells(ex.handle)
                assert (cells, one_pass) == (len(K.counts(case)), sum(r["collide"] for r in K.counts(case))), case.name
                if case.family == "E":
                    assert one_pass >= 1, case.name


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_batch_both_launch_shapes(size):
    """The geometry's cases as the 32 images of an enqueue (as many enqueues as they need, a flat image among them);
    then the detect stage again with four cells and with one cell per wave forced, and the later stages re-run on its
    output: every slot against the oracle."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd.batch import StereoFrontEnd
    w, h = size
    n_img = 2 * BATCH_PAIRS
    for th, cases in _groups(size).items():
        fe = StereoFrontEnd(w, h, max_pairs=BATCH_PAIRS, lanes=1, **cases[0].params)
        for i0 in range(0, len(cases), n_img - 1):
            part = cases[i0:i0 + n_img - 1]
            seq = part[:5] + [None] + part[5:]      # None: a flat image
            slots = [seq[i % len(seq)] for i in range(n_img)]
            flat = np.full((h, w), int(part[0].img[0, 0]), np.uint8)
            images = [flat if c is None else c.img for c in slots]
            refs = [NONE if c is None else K.ref(c) for c in slots]
            names = ["flat" if c is None else c.name for c in slots]
            fe.enqueue(torch.from_numpy(np.stack(images)).cuda(), BATCH_PAIRS, bf=BF, fx=FX)

            def check(what):
                assert fe.overflow() == 0, what
                for s, (name, ref) in enumerate(zip(names, refs)):
                    kps, desc = fe.fetch_image(s)
                    _assert_output(kps, desc, ref, f"{what}, slot {s} ({name})")

            check(f"{w} x {h} th {th}: batch")
            ms = C.c_float()
            for variant in (4, 5):      # four cells per wave, one cell per wave
                call("orbfe_microbench", fe.handle, 1, variant, 1, C.byref(ms))
                for later in (2, 3, 4):
                    call("orbfe_microbench", fe.handle, later, 0, 1, C.byref(ms))
                check(f"{w} x {h} th {th}: detect variant {variant}")
            if th[1] < th[0]:
                exp = sum(sum(r["collide"] for r in K.counts(c)) for c in slots if c is not None)
                assert _one_pass_cells(fe.handle)[1] == exp, (size, th)
