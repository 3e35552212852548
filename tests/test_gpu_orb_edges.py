"""k_orb at its decision points, bit for bit against the oracle, every keypoint of every image: the window staging
paths (dword / byte columns, reflected rows) at their edges, every misalignment of the dword path at both ends of
its range and at the end of the level-0 buffer, both halves of a wave's keypoint pair, and the orientation
classes (zero moment, axes, diagonals, both sides of every octant boundary, a spread of ratios), through the
single extract, the frame path and the batch path in the automatic describe shape and the three forced ones.

The fixtures are orb_cases.py's; tests/test_orb_cases_cpu.py shows on the CPU that they reach what they promise
and that the oracle's angles and descriptors follow from the stage's definition."""
import ctypes as C

import numpy as np
import pytest

import orb_cases as K

pytestmark = pytest.mark.gpu

DESCRIBE_SHAPES = ((0, "automatic"), (1, "8 per wave"), (9, "4 per wave"), (2, "2 per wave"))  # stage 3 variants
COPIES = 4  # consecutive image slots per placement image: byte offsets i W H = 0, 3, 2, 1 mod 4


def _assert_case(case, kps, desc, path):
    """Keypoint records and descriptors against the oracle; names the first differing keypoint."""
    ref = K.ref(case.name)
    assert len(ref.kps) > 0, case.name
    assert len(kps) == len(ref.kps), f"{path}: image {case.name!r}: {len(kps)} keypoints, the oracle keeps {len(ref.kps)}"
    desc = np.asarray(desc).reshape(-1, 32)
    for i in range(len(ref.kps)):
        if kps[i:i + 1].tobytes() != ref.kps[i:i + 1].tobytes():
            raise AssertionError(f"{path}: keypoint record differs: {K.describe_keypoint(case, ref, i)}: "
                                 f"{kps[i]} != {ref.kps[i]}")
        if not np.array_equal(desc[i], ref.desc[i]):
            raise AssertionError(f"{path}: descriptor differs: {K.describe_keypoint(case, ref, i)}: "
                                 f"bits {np.nonzero(np.unpackbits(desc[i] ^ ref.desc[i], bitorder='little'))[0].tolist()}")


def test_single_extract():
    from pyorbslam_amd.pyORBExtractor import ORBextractor
    extractors = {}
    for case in K.placement_set() + K.orientation_set():
        ex = extractors.setdefault(case.nlevels, ORBextractor(**K.params(case.nlevels)))
        kps, desc = ex.extract(case.image)
        _assert_case(case, kps, desc, "extract")


def test_frame_path_with_a_misaligned_right_image():
    """operator_kd_stereo with a placement image as both sides: the right image lies W H = 3 mod 4 bytes behind
    the left one, so its level 0 has an unaligned base."""
    from pyorbslam_amd.pyORBExtractor import ORBextractor
    prm = K.params(K.PLACEMENT_LEVELS)
    left, right = ORBextractor(**prm), ORBextractor(**prm)
    for case in K.placement_set():
        kl, dl, kr, dr = left.operator_kd_stereo(case.image, case.image.copy(), right, K.BF, np.float32(K.FX),
                                                 want_pyramid=False)
        _assert_case(case, kl, dl, "frame, left")
        _assert_case(case, kr, dr, "frame, right")


def _batch_in_every_shape(cases, nlevels, copies, offset):
    """One enqueue of every case `copies` times in consecutive slots, from a buffer whose first image starts
    `offset` bytes past a dword boundary; then the three forced describe shapes on the same buffers."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd._lib import call
    from pyorbslam_amd.batch import StereoFrontEnd
    slots = [c for c in cases for _ in range(copies)]
    if len(slots) % 2:
        slots.append(slots[-1])
    n_pairs = len(slots) // 2
    host = np.stack([c.image for c in slots])
    buf = torch.zeros(host.size + 4, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    view = buf[offset:offset + host.size]
    view.copy_(torch.from_numpy(host.reshape(-1)))
    images = view.view(len(slots), K.H, K.W)
    assert images.is_contiguous() and images.data_ptr() == buf.data_ptr() + offset
    if copies == COPIES:
        assert sorted((offset + i * K.W * K.H) % 4 for i in range(copies)) == [0, 1, 2, 3]
    fe = StereoFrontEnd(K.W, K.H, max_pairs=n_pairs, lanes=1, **K.params(nlevels))
    fe.enqueue(images, n_pairs, bf=K.BF, fx=K.FX)
    ms = C.c_float()
    for variant, name in DESCRIBE_SHAPES:
        if variant:
            call("orbfe_microbench", fe.handle, 3, variant, 1, C.byref(ms))
            call("orbfe_microbench", fe.handle, 4, 0, 1, C.byref(ms))
        assert fe.overflow() == 0, name
        for i, case in enumerate(slots):
            kps, desc = fe.fetch_image(i)
            _assert_case(case, kps, desc, f"batch from byte {offset}, {name}, slot {i} "
                                          f"(level-0 base {(offset + i * K.W * K.H) % 4} mod 4)")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned base", "base + 1 byte"])
def test_placement_batch_in_every_describe_shape(offset):
    _batch_in_every_shape(K.placement_set(), K.PLACEMENT_LEVELS, COPIES, offset)


def test_orientation_batch_in_every_describe_shape():
    _batch_in_every_shape(K.orientation_set(), 1, 1, 0)
