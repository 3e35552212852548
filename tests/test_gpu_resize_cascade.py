"""k_resize_cascade at the smallest geometries that reach each of its decisions: the pyramid of a noise image
(every byte matters) from the one-launch cascade at a placed strip count, bit for bit against the oracle's.

The cascade is forced through orbfe_microbench (stage 0: 100 + S = S strips, 6 = the automatic count), as
tests/test_gpu_paths.py does.  tests/test_resize_cascade_cases_cpu.py shows that the cases reach what they are
here for: the staged run's misalignments and pass boundaries, strips without a halo, of one top row and of fewer
rows than waves, the 64-group chunk boundary, area / wide / linear steps with every scalar tail, both parities of
the level ping-pong, the widest levels the cascade takes and the search for a strip count that fits the LDS.

A forced run writes over the pyramid the automatic one left, so a row that no strip stored would go unseen here;
test_stores_happen_and_images_read_their_own_rows replaces the batch's input between the two and so sees it."""
import ctypes as C

import numpy as np
import pytest

import resize_cascade_cases as K
import resize_rows_cases as R
import sweep_cases as S
from pyorbslam_amd._lib import OrbfeError, call, lib
from pyorbslam_amd.pyORBExtractor import ORBextractor

pytestmark = pytest.mark.gpu
ORBFE_ESTATE = -5


def _cus() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _extractor(case) -> ORBextractor:
    h, w, nlevels, scale, simd, _ = case
    return ORBextractor(**K.case_params(nlevels, scale, simd, K.nfeatures(case)))


def _assert_pyramid(got, case, what):
    h, w, nlevels, scale, simd, strips = case
    ref = K.reference_pyramid(h, w, nlevels, scale, simd)
    assert len(got) == len(ref) == nlevels
    for l, (g, o) in enumerate(zip(got, ref)):
        assert g.shape == o.shape, (K.case_id(case), what, "level", l, g.shape, o.shape)
        if not np.array_equal(g, o):
            ys, xs = np.nonzero(g != o)
            raise AssertionError(f"{K.case_id(case)} {what}: level {l} ({o.shape[1]} x {o.shape[0]}) differs in "
                                 f"{len(ys)} bytes, columns {xs.min()} .. {xs.max()}, rows {ys.min()} .. {ys.max()}")


def _taken_strips(handle, n_images: int) -> int:
    """The strip count of the cascade the last enqueue took (orbfe_debug_cascade_profile), 0 for the per-level
    launches."""
    marks = np.zeros(n_images * 1024 * 32, np.int64)
    n = C.c_int32()
    rc = lib().orbfe_debug_cascade_profile(handle, C.c_void_p(marks.ctypes.data), marks.size, C.byref(n))
    if rc == ORBFE_ESTATE:
        return 0
    assert rc == 0, rc
    return n.value


@pytest.mark.parametrize("case", K.ALL, ids=K.case_id)
def test_pyramid_bytes(case):
    """Every level of the automatic extraction, then of the forced cascade, equals the oracle's."""
    h, w, nlevels, scale, simd, strips = case
    ex = _extractor(case)
    ex.extract(R.noise(h, w))
    _assert_pyramid(ex.GetImagePyramid(sheared=False), case, "automatic")
    ms = C.c_float()
    if strips != K.AUTO:
        assert K.forced_strips(h, w, nlevels, scale, strips) == strips
        call("orbfe_microbench", ex.handle, 0, 100 + strips, 1, C.byref(ms))
        _assert_pyramid(ex.GetImagePyramid(sheared=False), case, f"S={strips}")
    elif K.chosen_strips(h, w, nlevels, scale, _cus(), 1):
        call("orbfe_microbench", ex.handle, 0, 6, 1, C.byref(ms))
        _assert_pyramid(ex.GetImagePyramid(sheared=False), case, "variant 6")
    else:  # no strip count serves this geometry: asking for the cascade is an error, not another kernel
        with pytest.raises(OrbfeError):
            call("orbfe_microbench", ex.handle, 0, 6, 1, C.byref(ms))


@pytest.mark.parametrize("n", [1, 3])
def test_stores_happen_and_images_read_their_own_rows(n):
    """n pairs on one StereoFrontEnd at W * H odd: the batch's input is replaced in place after the enqueue, then
    the forced cascade and every later stage run on it.  A row that no strip stored still holds the first batch's
    bytes, and an image staged from another image's rows (or at another misalignment) its neighbour's, so every
    image's keypoints, descriptors and stereo result must be the second batch's."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd.batch import StereoFrontEnd
    h, w, nlevels = K.BATCH
    assert nlevels == S.MIXED_NLEVELS and (w * h) % 2
    first, second = S.mixed_batch(h, w, n, *K.BATCH_FIRST), S.mixed_batch(h, w, n, *K.BATCH_SECOND)
    fe =StereoFrontEnd(w, h, max_pairs=n, lanes=1, **S.params(nlevels))
    dev = torch.from_numpy(first.images).cuda()
    fe.enqueue(dev, n, bf=S.BF, fx=S.FX)

    def check(mb, what):
        assert fe.overflow() == 0, what
        for p in range(n):
            kl, dl = fe.fetch_image(2 * p)
            kr, dr = fe.fetch_image(2 * p + 1)
            S.assert_image(kl, dl, mb.image_refs[2 * p], (what, "pair", p, mb.kinds[p], "left"))
            S.assert_image(kr, dr, mb.image_refs[2 * p + 1], (what, "pair", p, mb.kinds[p], "right"))
            S.assert_stereo(fe.fetch_stereo(p), kl, mb.pair_refs[p], (what, "pair", p, mb.kinds[p]))

    check(first, "enqueue")
    for a, b, ra, rb in zip(first.images, second.images, first.image_refs, second.image_refs):
        assert (a != b).any() and ra.levels_with_keypoints() - {0} and rb.levels_with_keypoints() - {0}
    assert K.level_sizes(h, w, nlevels, 1.2)[-1][1] in K.BATCH_STRIPS
    ms = C.c_float()
    # the two batches in turn, so that before every forced run the workspace holds the other batch's pyramid
    for strips, batch in zip(K.BATCH_STRIPS, (second, first, second)):
        dev.copy_(torch.from_numpy(batch.images))
        torch.cuda.synchronize()
        assert K.forced_strips(h, w, nlevels, 1.2, strips) == strips
        call("orbfe_microbench", fe.handle, 0, 100 + strips, 1, C.byref(ms))
        for later in range(1, 5):
            call("orbfe_microbench", fe.handle, later, 0, 1, C.byref(ms))
        check(batch, ("cascade", strips))


@pytest.mark.parametrize("case", K.PATHS, ids=K.case_id)
def test_path_taken(case):
    """The launch path of an automatic extraction of one image and of a pair (two images in one enqueue): the
    cascade with the strip count of prepare_pyramid's search, or the per-level launches; the pyramid is the
    oracle's either way."""
    h, w, nlevels, scale, simd, _ = case
    cus = _cus()
    img = R.noise(h, w)
    ex = _extractor(case)
    ex.extract(img)
    assert _taken_strips(ex.handle, 1) == K.chosen_strips(h, w, nlevels, scale, cus, 1), (K.case_id(case), cus, 1)
    _assert_pyramid(ex.GetImagePyramid(sheared=False), case, "one image")
    # a pair: the right extractor only receives its results
    from oracle.oracle import sheared
    right = _extractor(case)
    ex.operator_kd_stereo(img, img, right, S.BF, np.float32(S.FX), want_pyramid=False)
    assert _taken_strips(ex.handle, 2) == K.chosen_strips(h, w, nlevels, scale, cus, 2), (K.case_id(case), cus, 2)
    ref = K.reference_pyramid(h, w, nlevels, scale, simd)
    for side, e in enumerate((ex, right)):
        got = e.GetImagePyramid()
        for l, (g, o) in enumerate(zip(got, ref)):
            assert np.array_equal(g, sheared(o)), (K.case_id(case), "pair, side", side, "level", l)
