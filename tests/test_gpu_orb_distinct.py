"""k_orb evaluates every distinct BRIEF sample point once per keypoint and reads each bit's two ends back from
LDS: keypoints and descriptors of a natural and a noise pair, bit for bit against the oracle, in the automatic
describe shape and in every forced one (8, 4 and 2 keypoints per wave), at the smallest geometry the suite
already uses (131 x 96, 3 levels).  The fixture's seed was chosen on the CPU so that the oracle's output holds
what the kernel's pair loop and staging distinguish; test_fixture_reaches_the_paths asserts it."""
import ctypes as C
import functools

import numpy as np
import pytest

import sweep_cases as S
from oracle.oracle import OracleExtractor

H, W, NLEVELS = 96, 131, 3
SEED = 7
N_PAIRS = 2
DESCRIBE_SHAPES = ((0, "automatic"), (1, "8 per wave"), (9, "4 per wave"), (2, "2 per wave"))  # stage 3 variants


@functools.lru_cache(maxsize=None)
def fixture():
    """images (4, H, W): a natural pair, then a noise image and itself at disparity 3; their oracle references."""
    nat_l, nat_r = S.natural_pair(SEED, H, W)
    noise = S.noise(SEED, H, W)
    images = np.stack([nat_l, nat_r, noise, S.shifted(noise, 3)])
    return images, [S.ImageRef(img, NLEVELS) for img in images]


def _level_view(ref):
    """Per level: (level width, the kept keypoints' level x in output order)."""
    ox = OracleExtractor(**S.params(NLEVELS))
    sizes, scale = ox.level_sizes(W, H), ref.tables["scale"]
    out = []
    for l in range(NLEVELS):
        k = ref.kps[ref.kps["octave"] == l]
        out.append((sizes[l][0], np.rint(k["x"] / np.float32(scale[l])).astype(int)))
    return out


def test_fixture_reaches_the_paths():
    """On the oracle's output (no GPU work): an odd level count (a wave ends on an unpaired keypoint), a wave of
    exactly one keypoint in each of the three shapes, border-staged keypoints at even and at odd positions of
    their level (A and B of a pair: a wave starts at an even position), and angles in all four quadrants."""
    _, refs = fixture()
    counts, border_parity, quadrants = [], set(), set()
    for ref in refs:
        octaves = ref.kps["octave"]
        assert np.all(np.diff(octaves) >= 0)  # level-major output: a keypoint's position in its level
        for w, lx in _level_view(ref):
            counts.append(len(lx))
            border = (lx < 25) | (lx + 22 >= w)
            border_parity |= set((np.nonzero(border)[0] % 2).tolist())
        quadrants |= set((ref.kps["angle"] // 90).astype(int).tolist())
    assert any(n % 2 == 1 for n in counts), counts
    for kpw in (8, 4, 2):
        assert any(n % kpw == 1 for n in counts), (kpw, counts)
    assert border_parity == {0, 1}, border_parity
    assert quadrants == {0, 1, 2, 3}, quadrants


@pytest.mark.gpu
def test_every_describe_shape_matches_the_oracle():
    torch = pytest.importorskip("torch")
    from pyorbslam_amd._lib import call
    from pyorbslam_amd.batch import StereoFrontEnd
    images, refs = fixture()
    fe = StereoFrontEnd(W, H, max_pairs=N_PAIRS, lanes=1, **S.params(NLEVELS))
    fe.enqueue(torch.from_numpy(images).cuda(), N_PAIRS, bf=S.BF, fx=S.FX)
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
