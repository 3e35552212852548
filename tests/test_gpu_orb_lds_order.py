"""k_orb takes the distinct BRIEF points in brief_slot_order.inc's order and its horizontal items in orb_tables'
bank-aware order: a wrongly wired position or a dropped item shows only at the angles that steer a sample onto
it.  One noise pair at the smallest geometry the describe tests use (131 x 96, 3 levels), whose oracle keypoints
have angles in every 10 degree sector (the seed was chosen on the CPU; test_fixture_covers_every_sector asserts
it), bit for bit against the oracle in the automatic describe shape (the batch shape) and in every forced
keypoints-per-wave shape of small batches (8, 4 and 2)."""
import ctypes as C
import functools

import numpy as np
import pytest

import sweep_cases as S

H, W, NLEVELS = 96, 131, 3
SEED = 3
DISPARITY = 3
DESCRIBE_SHAPES = ((0, "automatic"), (1, "8 per wave"), (9, "4 per wave"), (2, "2 per wave"))  # stage 3 variants


@functools.lru_cache(maxsize=None)
def fixture():
    """images (2, H, W): a noise image and itself at disparity 3; their oracle references."""
    left = S.noise(SEED, H, W)
    images = np.stack([left, S.shifted(left, DISPARITY)])
    return images, [S.ImageRef(img, NLEVELS) for img in images]


def test_fixture_covers_every_sector():
    """On the oracle's output (no GPU work): each image has a keypoint in each of the 36 sectors of 10 degrees."""
    _, refs = fixture()
    for i, ref in enumerate(refs):
        angles = ref.kps["angle"]
        assert np.all((angles >= 0) & (angles < 360))
        census = np.bincount((angles // 10).astype(int), minlength=36)
        assert len(census) == 36 and np.all(census >= 1), (i, census.tolist())


@pytest.mark.gpu
def test_every_describe_shape_matches_the_oracle_at_every_sector():
    torch = pytest.importorskip("torch")
    from pyorbslam_amd._lib import call
    from pyorbslam_amd.batch import StereoFrontEnd
    images, refs = fixture()
    fe = StereoFrontEnd(W, H, max_pairs=1, lanes=1, **S.params(NLEVELS))
    fe.enqueue(torch.from_numpy(images).cuda(), 1, bf=S.BF, fx=S.FX)
    ms = C.c_float()
    for variant, name in DESCRIBE_SHAPES:
        if variant:
            call("orbfe_microbench", fe.handle, 3, variant, 1, C.byref(ms))
            call("orbfe_microbench", fe.handle, 4, 0, 1, C.byref(ms))
        assert fe.overflow() == 0, name
        for i, ref in enumerate(refs):
            kps, desc = fe.fetch_image(i)
            assert len(ref.kps) > 0
            S.assert_image(kps, desc, ref, (name, "image", i))
