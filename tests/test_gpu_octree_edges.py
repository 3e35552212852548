"""k_octree_bins (both pass implementations, both workgroup shapes) and k_octree at DistributeOctTree's decision
points, row for row against the oracle, every image of octree_cases.py: how the full passes end, the careful
switch at equality, the break and the ties of the careful phase, divisions below the bin depth, the geometry of
the splits, what a node keeps, the two pass implementations at their boundary, the key table and a level above 0.

tests/test_octree_cases_cpu.py shows on the CPU that every case yields exactly the candidates it places and
stands on the decision it is named for."""
import ctypes as C
import itertools

import numpy as np
import pytest

import octree_cases as K
from oracle import oracle as O
from pyorbslam_amd._lib import call, ptr
from pyorbslam_amd.pyORBExtractor import ORBextractor

pytestmark = pytest.mark.gpu

GROUPS = sorted({c.name[0] for c in K.CASES})
BATCH_PAIRS = 16        # n_images = 32: the launcher's own rule takes the 256-thread shape
SHORT_PAIRS = 2
BF, FX = 40.0, 100.0


def _group(g):
    return [c for c in K.CASES if c.name[0] == g]


def _debug(ex, fn, level, cap):
    buf = np.zeros((cap, 3), np.int32)
    n = C.c_int32()
    call(fn, ex.handle, level, ptr(buf), cap, C.byref(n))
    return buf[:n.value].copy()


def _kernel(ex):
    k, b = C.c_int32(), C.c_int64()
    call("orbfe_get_octree_kernel", ex.handle, C.byref(k), C.byref(b))
    return k.value


def _assert_rows(got, exp, what):
    got, exp = [tuple(r) for r in np.asarray(got).tolist()], [tuple(r) for r in np.asarray(exp).tolist()]
    n = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    assert got == exp, f"{what}: {len(got)} rows against {len(exp)}, first difference at row {n}: " \
                       f"{got[n] if n < len(got) else None} != {exp[n] if n < len(exp) else None}"


def _assert_output(kps, desc, ref, what):
    okps, odesc = ref
    assert len(kps) == len(okps), f"{what}: {len(kps)} keypoints, the oracle keeps {len(okps)}"
    for i in range(len(okps)):
        assert kps[i:i + 1].tobytes() == okps[i:i + 1].tobytes(), f"{what}: keypoint {i}: {kps[i]} != {okps[i]}"
    assert np.array_equal(np.asarray(desc).reshape(-1, 32), odesc.reshape(-1, 32)), f"{what}: descriptors differ"


def _assert_case(ex, case, what):
    """One extraction through ex: the candidates, the selection in list order, the keypoints and descriptors."""
    kps, desc = ex.extract(K.image(case))
    i = K.info(case)
    for level in range(case.level):
        assert len(_debug(ex, "orbfe_debug_candidates", level, 64)) == 0, what
        assert len(_debug(ex, "orbfe_debug_selected", level, 64)) == 0, what
    _assert_rows(_debug(ex, "orbfe_debug_candidates", case.level, len(i.K) + 8), i.K, f"{what}: candidates")
    _assert_rows(_debug(ex, "orbfe_debug_selected", case.level, len(i.kept) + 8), i.kept, f"{what}: selection")
    _assert_output(kps, desc, K.ref(case), what)


@pytest.mark.parametrize("group", GROUPS)
def test_single_extraction(group):
    """k_octree_bins in its 512-thread shape, one image per launch."""
    for case in _group(group):
        ex = ORBextractor(**case.params)
        _assert_case(ex, case, f"{case.name}: extract")
        assert _kernel(ex) == 0, case.name


@pytest.mark.parametrize("group", GROUPS)
def test_per_candidate_kernel(group):
    """k_octree forced, then the bins kernel again on the same handle."""
    for case in _group(group):
        ex = ORBextractor(**case.params)
        call("orbfe_set_octree_kernel", ex.handle, 1)
        _assert_case(ex, case, f"{case.name}: k_octree")
        assert _kernel(ex) == 1, case.name
        call("orbfe_set_octree_kernel", ex.handle, 0)
        _assert_case(ex, case, f"{case.name}: k_octree_bins after k_octree")
        assert _kernel(ex) == 0, case.name


@pytest.fixture(scope="module")
def oracle_at():
    """The oracle's output of a case's image under another case's parameters, computed once."""
    memo = {}

    def get(image_case, params_case):
        if image_case.params == params_case.params:
            return K.ref(image_case)
        key = (image_case.name, params_case.name)
        if key not in memo:
            memo[key] = O.OracleExtractor(**params_case.params).extract(K.image(image_case))
        return memo[key]
    return get


def _check_batch(fe, slots, refs, what):
    assert fe.overflow() == 0, what
    for s, (name, ref) in enumerate(zip(slots, refs)):
        kps, desc = fe.fetch_image(s)
        _assert_output(kps, desc, ref, f"{what}, slot {s} ({name})")


@pytest.mark.parametrize("group", GROUPS)
def test_batches_in_both_shapes(group, oracle_at):
    """Per image size and parameters: the group's cases, repeated, as the 32 images of one enqueue with an
    all-background image between two dense ones (the 256-thread shape by the launcher's rule), then both
    shapes forced with the later stages re-run, then a short batch of other content on the same handle."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd.batch import StereoFrontEnd
    ms = C.c_float()
    by_handle = {}
    for case in _group(group):
        by_handle.setdefault((case.size, tuple(sorted(case.params.items()))), []).append(case)
    for (size, _), cases in by_handle.items():
        w, h = size
        flat = np.full((h, w), K.BG, np.uint8)
        none = (np.zeros(0, O.KP_DTYPE), np.zeros((0, 32), np.uint8))
        cyc = itertools.cycle(cases)
        slots = [next(cyc) for _ in range(2 * BATCH_PAIRS)]
        images = [K.image(c) for c in slots]
        names, refs = [c.name for c in slots], [K.ref(c) for c in slots]
        images[1], names[1], refs[1] = flat, "background", none
        fe = StereoFrontEnd(w, h, max_pairs=BATCH_PAIRS, lanes=1, **cases[0].params)
        dev = torch.from_numpy(np.stack(images)).cuda()
        fe.enqueue(dev, BATCH_PAIRS, bf=BF, fx=FX)
        what = f"{cases[0].name} ({w} x {h}, N = {cases[0].N})"
        _check_batch(fe, names, refs, f"{what}: batch")
        for variant, shape in ((1, "256 threads"), (2, "512 threads")):
            call("orbfe_microbench", fe.handle, 2, variant, 1, C.byref(ms))
            for later in (3, 4):
                call("orbfe_microbench", fe.handle, later, 0, 1, C.byref(ms))
            _check_batch(fe, names, refs, f"{what}: forced {shape}")
        # a shorter batch of other content: what the longer one left in the key cache and counters must not leak
        others = [c for c in K.CASES if c.size == size and c.level == cases[0].level and c not in cases][:3] or cases[:1]
        short = [others[k % len(others)] for k in range(2 * SHORT_PAIRS)]
        simg = [K.image(c) for c in short]
        sref = [oracle_at(c, cases[0]) for c in short]
        snames = [c.name for c in short]
        simg[2], snames[2], sref[2] = flat, "background", none
        fe.enqueue(torch.from_numpy(np.stack(simg)).cuda(), SHORT_PAIRS, bf=BF, fx=FX)
        _check_batch(fe, snames, sref, f"{what}: short batch after the full one")


def test_dense_then_one_key_then_dense(oracle_at):
    """One handle per image size: the densest case, the K = 1 case's image, the densest case again."""
    for size in sorted({c.size for c in K.CASES if not c.level}):
        same = [c for c in K.CASES if c.size == size and not c.level]
        dense = max(same, key=lambda c: len(K.dots_of(c)))
        one = next(c for c in K.CASES if len(K.dots_of(c)) == 1 and not c.level)
        if one.size != size:   # the K = 1 dot of another geometry, on this one's background
            x, y, v = K.dots_of(one)[0]
            one = K.Case(f"one dot on {size}", dense.geo, "mixed", (0, ((min(x, size[0] - 20), min(y, size[1] - 20), v),), 0),
                         dense.N, ())
        ex = ORBextractor(**dense.params)
        _assert_case(ex, dense, f"{dense.name}: first")
        kps, desc = ex.extract(K.image(one))
        _assert_output(kps, desc, oracle_at(one, dense), f"{one.name} after {dense.name}")
        assert len(kps) == 1
        _assert_case(ex, dense, f"{dense.name}: after one key")
