"""LDS bank-conflict model of k_orb's table-driven accesses (development aid; tests/test_orb_lds_order_cpu.py
holds the committed tables to it).

It reads brief_distinct.inc and brief_slot_order.inc, restates orb_tables' item list (orbfe_host.hip) and prints
the modelled LDS-array cycles per keypoint of

  * BRIEF phase 1: the H gathers.  Lane j evaluates positions 2 (j + 64 i) + e (i = 0..2, e = 0, 1), each with
    4 dword reads (2 ds_read2_b32) at H dwords 40 (floor(R / 2) + 9 + k) + C + 21, k = 0..3, where
    R = rint(x b + y a), C = rint(x a - y b) of the position's point (x, y) and the angle's a = cos, b = sin;
  * BRIEF phase 2: lane j's ds_read_u8 of the two ends of its bits j + 64 i (i = 0..3); a position is the byte
    index in the wave's s_val buffer;
  * hpass source reads: lane j's item j + 64 k (k = 0..2) reads source dwords 24 m + gx + {0, 1, 2, 12, 13, 14};
  * hpass H stores: ds_write_b128 at H dwords 40 m + 4 gx .. + 3.

The bank rule (MI355X LDS): for ds_read_b32, ds_read2_b32, ds_read_u8 and every ds_write the bank of a byte
address is (address / 4) mod 32; reads go in lane groups {0..31}, {32..63}, ds_write_b128 in groups of 8
consecutive lanes.  A group costs the maximum over the banks of the number of distinct dwords on that bank (the
same dword broadcasts), one LDS-array cycle when conflict-free.

usage: python tools/orb_lds_model.py [--angles N]
"""
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pyorbslam_amd" / "csrc"
SLOTS, REAL = 384, 375
H_PITCH, SRC_PITCH = 40, 12   # dwords: H row pair, staged source row
DISC_R = 18.384776310850235 + 0.7072


def read_distinct(path=CSRC / "brief_distinct.inc"):
    """(points of the 384 slots, per bit the slots of its two ends)."""
    text = "\n".join(l for l in Path(path).read_text().splitlines() if not l.startswith("//"))
    points = [(int(x), int(y)) for x, y in re.findall(r"BRIEF_POINT\(\s*(-?\d+),\s*(-?\d+)\)", text)]
    bits = [(int(a), int(b)) for a, b in re.findall(r"BRIEF_BIT\(\s*(-?\d+),\s*(-?\d+)\)", text)]
    assert len(points) == SLOTS and len(bits) == 256
    return points, bits


def read_order(path=CSRC / "brief_slot_order.inc"):
    """position -> slot."""
    text = "\n".join(l for l in Path(path).read_text().splitlines() if not l.startswith("//"))
    order = [int(t) for t in re.findall(r"BRIEF_SLOT\(\s*(\d+)\)", text)]
    assert len(order) == SLOTS
    return order


def angles(n=720):
    """(a, b) = (cos, sin) in float32 of theta_k = (k + 0.11) 2 pi / n."""
    th = (np.arange(n) + 0.11) * (2 * np.pi / n)
    return np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)


def h_dwords(points, a, b):
    """[angle, position]: the H dword of the first of a point's four vertical-tap reads."""
    p = np.asarray(points, np.float32)
    x, y = p[None, :, 0], p[None, :, 1]
    a, b = a[:, None], b[:, None]
    r = np.rint(x * b + y * a).astype(np.int64)
    c = np.rint(x * a - y * b).astype(np.int64)
    return H_PITCH * (r // 2 + 9) + c + 21


def group_cost(dw):
    """dw [..., lanes]: dword index per lane of one lane group -> cycles [...]: max over the 32 banks of the
    number of distinct dwords on the bank."""
    dw = np.sort(np.asarray(dw, np.int64), axis=-1)
    first = np.ones(dw.shape, bool)
    first[..., 1:] = dw[..., 1:] != dw[..., :-1]
    flat = dw.reshape(-1, dw.shape[-1])
    rows = np.arange(flat.shape[0])[:, None]
    cnt = np.zeros((flat.shape[0], 32), np.int64)
    np.add.at(cnt, (rows, flat % 32), first.reshape(flat.shape))
    return cnt.max(axis=1).reshape(dw.shape[:-1])


def phase1_groups():
    """[12, 32]: the positions that one half-wave reads together (iteration i, end e, half h)."""
    j = np.arange(32)
    return np.array([2 * (j + 32 * h + 64 * i) + e for i in range(3) for e in range(2) for h in range(2)])


def phase1_cycles(pos_points, ab=None):
    """Mean over the angles of the cycles per keypoint of the H gathers (4 reads per group: the reads of a
    point are 40 dwords = 8 banks apart, so all four cost what the first does)."""
    a, b = ab if ab is not None else angles()
    dw = h_dwords(pos_points, a, b)
    return float(4 * group_cost(dw[:, phase1_groups()]).sum(axis=1).mean())


def phase2_detail(bit_pos):
    """bit_pos [256, 2]: the positions of each bit's ends; lane j reads bits j + 64 i, one end at a time.
    (cycles per keypoint of the 16 half-wave reads, reads that collide with another dword on their bank)."""
    dw = np.sort((np.asarray(bit_pos) // 4).reshape(8, 32, 2).transpose(0, 2, 1).reshape(16, 32), axis=1)
    first = np.ones(dw.shape, bool)
    first[:, 1:] = dw[:, 1:] != dw[:, :-1]
    cnt = np.zeros((16, 32), np.int64)
    np.add.at(cnt, (np.arange(16)[:, None], dw % 32), first)
    return int(cnt.max(axis=1).sum()), int(np.maximum(cnt - 1, 0).sum())


def phase2_cycles(bit_pos):
    return phase2_detail(bit_pos)[0]


def compose(points, bits, order):
    """What orbfe_kernels.hip composes: the point at every position, and per bit the positions of its ends."""
    inv = {s: p for p, s in enumerate(order)}
    return [points[s] for s in order], [(inv[s0], inv[s1]) for s0, s1 in bits]


# ---- hpass ---------------------------------------------------------------------------------------------------------
def h_items():
    """orb_tables' 189 (row pair m, 4-column group gx) items, row-major."""
    need = np.zeros((44, 40), bool)
    for row in range(-18, 19):
        for col in range(-18, 19):
            if row * row + col * col <= DISC_R * DISC_R:
                need[row + 18:row + 25, col + 21] = True
    return [(m, gx) for m in range(22) for gx in range(10) if need[2 * m:2 * m + 2, 4 * gx:4 * gx + 4].any()]


def src_bank(item):
    m, gx = item
    return (2 * m * SRC_PITCH + gx) % 32


def h_item_order():
    """orb_tables' placement of the items on 192 (lane, k) slots, index lane + 64 k; None = the dummy item.
    Restates orbfe_host.hip: the r-th item (row-major) of a source bank goes to 32-lane group min(r, 5).  Every
    bank holds 5 to 8 items, so groups 0 .. 4 hold one item of every bank and read without a conflict, and the
    items no order can separate (a bank with 8 items takes 2 extra cycles per read in any order) share group 5.
    Inside a group the items are dealt into runs of 8 lanes with distinct H store banks (the b128 store of item
    (m, gx) covers banks 4 q .. 4 q + 3, q = (2 m + gx) mod 8) as far as a first-fit pass finds them."""
    groups, seen = [[] for _ in range(6)], {}
    for it in h_items():
        r = seen.get(src_bank(it), 0)
        seen[src_bank(it)] = r + 1
        groups[min(r, 5)].append(it)
    out = []
    for grp in groups:
        assert len(grp) <= 32
        left = list(grp)
        while left:
            run, used = [], set()
            for it in list(left):
                q = (2 * it[0] + it[1]) % 8
                if len(run) < 8 and q not in used:
                    used.add(q)
                    run.append(it)
                    left.remove(it)
            while len(run) < 8 and left:
                run.append(left.pop(0))
            out += run
        out += [None] * (32 - len(grp))
    return out


def row_major_order():
    items = h_items()
    return items + [None] * (192 - len(items))


def hpass_cycles(order):
    """(source-read cycles, H-store cycles) per keypoint of a 192-slot item order."""
    src = np.array([0 if it is None else 2 * it[0] * SRC_PITCH + it[1] for it in order])
    hst = np.array([0 if it is None else H_PITCH * it[0] + 4 * it[1] for it in order])
    reads = sum(int(group_cost(src[g:g + 32] + off)) for g in range(0, 192, 32) for off in (0, 1, 2, 12, 13, 14))
    stores = 0
    for g in range(0, 192, 8):
        dw = (hst[g:g + 8, None] + np.arange(4)[None, :]).reshape(-1)
        stores += int(group_cost(dw))
    return reads, stores


def main():
    n = int(sys.argv[sys.argv.index("--angles") + 1]) if "--angles" in sys.argv else 720
    points, bits = read_distinct()
    ident = list(range(SLOTS))
    rows = []
    for name, order in (("first-occurrence order", ident), ("brief_slot_order.inc", read_order())):
        pp, bp = compose(points, bits, order)
        rows.append((name, phase1_cycles(pp, angles(n)), phase2_cycles(bp)))
    print(f"modelled LDS-array cycles per keypoint ({n} angles)")
    print(f"{'access':44s} {'before':>8s} {'committed':>10s} {'conflict-free':>14s}")
    print(f"{'BRIEF phase 1, H gathers':44s} {rows[0][1]:8.1f} {rows[1][1]:10.1f} {48:14d}")
    print(f"{'BRIEF phase 2, byte reads of s_val':44s} {rows[0][2]:8d} {rows[1][2]:10d} {16:14d}")
    r0, s0 = hpass_cycles(row_major_order())
    r1, s1 = hpass_cycles(h_item_order())
    print(f"{'hpass source reads':44s} {r0:8d} {r1:10d} {36:14d}")
    print(f"{'hpass H stores (array cycles)':44s} {s0:8d} {s1:10d} {24:14d}")


if __name__ == "__main__":
    main()
