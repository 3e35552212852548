"""k_resize_rows at the smallest geometries that reach each of its paths: the pyramid of a noise image (every byte
matters) from the per-level launches, with and without the remainder wave, bit for bit against the oracle's.

One image takes the cascade, so the per-level launches are forced through orbfe_microbench (stage 0: 7 = with
the remainder wave, 5 = without), as tests/test_gpu_sweep.py does.  tests/test_resize_rows_cases_cpu.py shows
that the geometries reach what they are here for: the source stride's residues mod 4 and the staged run's
misalignments, the scalar tail in the only wave / a full wave / the remainder wave / the last of several chunks,
every block size, the shortest and the longest staging, band and row-set remainders.

The issue's 2 100 x 40 is 2 100 x 56 here (the oracle refuses 40 rows at three levels) and serves the 448-thread
block; its level 1 is 1 750 px, one chunk per wave, so the several-chunk case is 2 461 x 56 (level 1: 2 051 px)."""
import ctypes as C

import numpy as np
import pytest

import resize_rows_cases as R
import sweep_cases as S
from pyorbslam_amd._lib import call
from pyorbslam_amd.pyORBExtractor import ORBextractor

pytestmark = pytest.mark.gpu


def _check_pyramids(h, w, nlevels, simds):
    img = R.noise(h, w)
    ms = C.c_float()
    for simd in simds:
        ref = R.reference_pyramid(h, w, nlevels, simd)
        ex = ORBextractor(**R.params(nlevels, simd))
        ex.extract(img)
        for variant in (7, 5):
            call("orbfe_microbench", ex.handle, 0, variant, 1, C.byref(ms))
            got = ex.GetImagePyramid(sheared=False)
            assert len(got) == len(ref) == nlevels
            for l, (g, o) in enumerate(zip(got, ref)):
                assert g.shape == o.shape and np.array_equal(g, o), ((h, w), "simd", simd, "variant", variant, "level", l)


def _id(geo):
    return f"{geo[1]}x{geo[0]}"


@pytest.mark.parametrize("geo", R.STRIDES, ids=_id)
def test_source_stride_residues(geo):
    """Level-0 widths 0 .. 3 mod 4: the hoisted window alignment (stride a multiple of 4) and the per-row one, every
    misalignment of a band's staged run; level 2 reads level 1 at its 16-byte pitch."""
    _check_pyramids(*geo, simds=(16,))


@pytest.mark.parametrize("simd", R.SIMD_MODES)
@pytest.mark.parametrize("geo", R.TAILS, ids=_id)
def test_scalar_tail_placements(geo, simd):
    """The tail's groups in the level's only wave, in a full wave of a last chunk of 40, in the remainder wave of a
    last chunk of 1 and of 39, and in the last of the chunks a wave walks; without a vector span (every group in
    the tail) and with 32-lane steps."""
    _check_pyramids(*geo, simds=(simd,))


@pytest.mark.parametrize("geo", R.BLOCKS + R.SLOTS, ids=_id)
def test_block_sizes_and_staging_lengths(geo):
    """Blocks of 256, 320, 384, 448 and 512 threads (512 with one chunk per wave and with several); bands whose
    staged run fills a pass exactly (24 dwords per thread) and needs a second one."""
    _check_pyramids(*geo, simds=(16,))


@pytest.mark.parametrize("geo", R.HEIGHTS, ids=_id)
def test_band_and_row_set_remainders(geo):
    """Level heights 0, 1 and 15 mod 16 (the 1-row band stages less than a dword per thread); row sets of an odd
    number of rows and sets without a row."""
    _check_pyramids(*geo, simds=(16,))


def test_batch_through_the_per_level_launches():
    """Three pairs on one StereoFrontEnd: the batch's input is replaced in place after the enqueue (whose pyramid
    came from the cascade), then the per-level launches and every later stage run on it, so each image's results
    show that its own bands were computed from its own rows (image index, block remap in the grid's y)."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd.batch import StereoFrontEnd
    h, w, nlevels = R.BATCH
    assert nlevels == S.MIXED_NLEVELS
    n = 3
    first, second = S.mixed_batch(h, w, n, 7000, 1), S.mixed_batch(h, w, n, 8000, 4)
    assert first.kinds != second.kinds
    fe = StereoFrontEnd(w, h, max_pairs=n, lanes=1, **S.params(nlevels))
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
    assert any(len(r.kps) and set(np.unique(r.kps["octave"])) - {0} for r in second.image_refs)
    dev.copy_(torch.from_numpy(second.images))
    torch.cuda.synchronize()
    ms = C.c_float()
    for variant in (7, 5):
        call("orbfe_microbench", fe.handle, 0, variant, 1, C.byref(ms))
        for later in range(1, 5):
            call("orbfe_microbench", fe.handle, later, 0, 1, C.byref(ms))
        check(second, ("per-level launches", variant))
