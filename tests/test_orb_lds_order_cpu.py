"""k_orb's bank-aware tables: the order in which its lanes take the distinct BRIEF points
(pyorbslam_amd/csrc/brief_slot_order.inc, composed with brief_distinct.inc at compile time) against the pattern
itself (brief_pattern.inc), and the order of the horizontal items (orb_tables, restated by
tools/orb_lds_model.py).  The three .inc files are parsed here with parsers of this test's own; the tools are
used to regenerate and to model the LDS cycles."""
import importlib.util
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pyorbslam_amd" / "csrc"
SLOTS, REAL = 384, 375  # 6 per lane of a wavefront; the distinct points


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _body(name):
    return "\n".join(l for l in (CSRC / name).read_text().splitlines() if not l.startswith("//"))


def _pattern():
    v = [int(t) for t in re.findall(r"-?\d+", _body("brief_pattern.inc"))]
    assert len(v) == 1024
    return [((v[i], v[i + 1]), (v[i + 2], v[i + 3])) for i in range(0, 1024, 4)]


def _distinct():
    text = _body("brief_distinct.inc")
    points = [(int(x), int(y)) for x, y in re.findall(r"BRIEF_POINT\(\s*(-?\d+),\s*(-?\d+)\)", text)]
    bits = [(int(a), int(b)) for a, b in re.findall(r"BRIEF_BIT\(\s*(-?\d+),\s*(-?\d+)\)", text)]
    assert len(points) == SLOTS and len(bits) == 256
    return points, bits


def _order():
    text = _body("brief_slot_order.inc")
    order = [int(s) for s in re.findall(r"BRIEF_SLOT\(\s*(\d+)\)", text)]
    assert not re.sub(r"BRIEF_SLOT\(\s*\d+\)", "", text).strip()  # nothing but the macro's invocations
    return order


def _composed():
    """What orbfe_kernels.hip composes: the point at every position and, per bit, the positions of its ends."""
    points, bits = _distinct()
    order = _order()
    position = {s: p for p, s in enumerate(order)}
    return [points[s] for s in order], [(position[s0], position[s1]) for s0, s1 in bits]


def test_order_is_a_permutation():
    assert sorted(_order()) == list(range(SLOTS))


def test_every_bit_maps_back_to_its_pair_and_reads_no_pad():
    order = _order()
    pos_points, bit_pos = _composed()
    assert len(bit_pos) == 256
    for bit, ((p0, p1), (e0, e1)) in enumerate(zip(bit_pos, _pattern())):
        assert 0 <= p0 < SLOTS and 0 <= p1 < SLOTS, bit
        assert pos_points[p0] == e0 and pos_points[p1] == e1, bit
        assert order[p0] < REAL and order[p1] < REAL, bit  # a pad position holds a slot >= 375


def test_regenerating_reproduces_the_committed_file():
    gen = _tool("gen_pattern")
    assert gen.render_slot_order(gen.from_inc()).encode() == (CSRC / "brief_slot_order.inc").read_bytes()


def test_modelled_brief_cycles():
    """The issue's bounds: phase 1 <= 100 and phase 2 <= 30 LDS-array cycles per keypoint on 720 angles; the
    first-occurrence order models at 157.2 and 30."""
    model = _tool("orb_lds_model")
    points, bits = _distinct()
    pos_points, bit_pos = _composed()
    assert (pos_points, bit_pos) == model.compose(points, bits, _order())
    ident_points, ident_bits = model.compose(points, bits, list(range(SLOTS)))
    assert abs(model.phase1_cycles(ident_points) - 157.2) < 0.05 and model.phase2_cycles(ident_bits) == 30
    p1, p2 = model.phase1_cycles(pos_points), model.phase2_cycles(bit_pos)
    print("phase 1", p1, "phase 2", p2)
    assert p1 <= 100
    assert p2 <= 30


def test_reordered_items_are_the_row_major_items():
    """orb_tables' order (restated by the tool) holds each of the 189 items once and 3 dummies, saves at least 12
    of the row-major order's 72 source-read cycles and does not raise its 35 H-store cycles."""
    model = _tool("orb_lds_model")
    row_major, ordered = model.row_major_order(), model.h_item_order()
    assert len(ordered) == 192 and ordered.count(None) == 3
    items = [it for it in ordered if it is not None]
    assert len(items) == 189 and len(set(items)) == 189
    assert set(items) == {it for it in row_major if it is not None}
    assert model.hpass_cycles(row_major) == (72, 35)
    reads, stores = model.hpass_cycles(ordered)
    print("source reads", reads, "H stores", stores)
    assert reads <= 72 - 12
    assert stores <= 35
