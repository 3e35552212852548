"""The distinct-point tables of the steered-BRIEF pattern (pyorbslam_amd/csrc/brief_distinct.inc, what k_orb
reads) against the pattern itself (brief_pattern.inc, what the oracle reads).  Both files are parsed here
with parsers of this test's own; tools/gen_pattern.py is used only to regenerate."""
import importlib.util
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pyorbslam_amd" / "csrc"
SLOTS = 384           # 6 per lane of a wavefront
# the largest sample radius of the pattern plus the rounding of a rotated coordinate (k_orb's header): the
# disc whose horizontal items orb_tables builds
DISC_R2 = (18.385 + 0.708) ** 2


def _pattern():
    text = "\n".join(l for l in (CSRC / "brief_pattern.inc").read_text().splitlines() if not l.startswith("//"))
    v = [int(t) for t in re.findall(r"-?\d+", text)]
    assert len(v) == 1024
    return [((v[i], v[i + 1]), (v[i + 2], v[i + 3])) for i in range(0, 1024, 4)]


def _tables():
    text = "\n".join(l for l in (CSRC / "brief_distinct.inc").read_text().splitlines() if not l.startswith("//"))
    points = [(int(x), int(y)) for x, y in re.findall(r"BRIEF_POINT\(\s*(-?\d+),\s*(-?\d+)\)", text)]
    bits = [(int(a), int(b)) for a, b in re.findall(r"BRIEF_BIT\(\s*(-?\d+),\s*(-?\d+)\)", text)]
    # nothing but the two macros' invocations
    assert not re.sub(r"BRIEF_(POINT|BIT)\(\s*-?\d+,\s*-?\d+\)", "", text).strip()
    return points, bits


def test_distinct_points_and_slots():
    pattern = _pattern()
    points, bits = _tables()
    ends = [p for pair in pattern for p in pair]
    distinct = list(dict.fromkeys(ends))  # first-occurrence order
    assert len(ends) == 512 and len(distinct) == 375
    assert len(points) == SLOTS
    assert points[:375] == distinct
    assert points[375:] == [(0, 0)] * (SLOTS - 375)


def test_every_bit_maps_back_to_its_pair():
    pattern = _pattern()
    points, bits = _tables()
    assert len(bits) == 256
    for bit, ((s0, s1), (p0, p1)) in enumerate(zip(bits, pattern)):
        assert 0 <= s0 < SLOTS and 0 <= s1 < SLOTS, bit
        assert points[s0] == p0 and points[s1] == p1, bit
        assert s0 < 375 and s1 < 375, bit  # no bit reads a pad slot


def test_all_points_lie_on_the_sample_disc():
    points, _ = _tables()
    for s, (x, y) in enumerate(points):
        assert x * x + y * y <= DISC_R2, (s, x, y)
    assert all(x * x + y * y <= DISC_R2 for x, y in points[375:])  # the pad points in particular


def test_regenerating_reproduces_the_committed_file():
    spec = importlib.util.spec_from_file_location("gen_pattern", ROOT / "tools" / "gen_pattern.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render_distinct(gen.from_inc()).encode() == (CSRC / "brief_distinct.inc").read_bytes()
