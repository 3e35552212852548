"""Cases for k_bow_match: crafted descriptors (bit flips of one base row give exact Hamming distances) and
hand-written CSR feature vectors; no vocabulary.  Each case carries the claim it exists for as a `check`
over the array oracle's results, which tests/test_bow_match_cases_cpu.py runs, so the GPU test that compares
the kernel with the oracle cannot pass on inputs that miss the situation.

A case: name, frames (bow_match_oracle frame dicts), pairs [(f1, f2)], th, inclusive, nnratio, use_elig1,
use_elig2, check(results) with results[p] = (match12, match21, bin12, hist, n_raw), and stable_cut (False only
for the case that breaks the rotation-cut condition on purpose).
"""
from __future__ import annotations

import numpy as np

import bow_match_oracle as O

WAVES = 8   # waves per k_bow_match workgroup (kBmWaves): nodes of one pair in flight
CHUNK = 64  # features of frame 2's run a wave looks at per step; the first chunk stays in registers

_BASE = np.random.Generator(np.random.PCG64(4242)).integers(0, 256, 32, dtype=np.uint8)


def D(*bits):
    """The base descriptor with the given bit positions flipped: hamming(D(A), D(B)) = |A xor B|."""
    d = _BASE.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def R(a, b):
    return tuple(range(a, b))


class FrameBuilder:
    def __init__(self):
        self.desc, self.angle, self.elig, self.nodes = [], [], [], {}

    def add(self, node, desc, angle=0.0, elig=1):
        i = len(self.desc)
        self.desc.append(desc)
        self.angle.append(angle)
        self.elig.append(elig)
        self.nodes.setdefault(node, []).append(i)
        return i

    def empty_node(self, node):
        self.nodes.setdefault(node, [])

    def reverse(self, node):
        self.nodes[node].reverse()

    def build(self):
        nodes = sorted(self.nodes)
        idx = [i for k in nodes for i in self.nodes[k]]
        return dict(desc=np.array(self.desc, np.uint8).reshape(-1, 32), angle=np.array(self.angle, np.float32),
                    elig=np.array(self.elig, np.uint8), fv_node=np.array(nodes, np.int32),
                    fv_end=np.cumsum([len(self.nodes[k]) for k in nodes]).astype(np.int32),
                    fv_idx=np.array(idx, np.int32))


def pack(frames):
    """The host entry's arrays of a list of frames."""
    cat = lambda k, dt: (np.concatenate([f[k] for f in frames]).astype(dt) if frames else np.zeros(0, dt))  # noqa: E731
    off = np.zeros(len(frames) + 1, np.int64)
    np.cumsum([len(f["desc"]) for f in frames], out=off[1:])
    fv_off = np.zeros(len(frames) + 1, np.int64)
    np.cumsum([len(f["fv_node"]) for f in frames], out=fv_off[1:])
    fv_idx = np.zeros(int(off[-1]), np.int32)
    for k, f in enumerate(frames):
        fv_idx[off[k]:off[k] + len(f["fv_idx"])] = f["fv_idx"]
    return dict(desc=cat("desc", np.uint8).reshape(-1, 32), angle=cat("angle", np.float32), elig=cat("elig", np.uint8),
                off=off, fv_off=fv_off, fv_node=cat("fv_node", np.int32), fv_end=cat("fv_end", np.int32), fv_idx=fv_idx)


def oracle(case, block=True):
    return [O.match_pair(case["frames"][a], case["frames"][b], case["use_elig1"], case["use_elig2"], case["th"],
                         case["inclusive"], case["nnratio"], block) for a, b in case["pairs"]]


def _case(name, frames, pairs=((0, 1),), th=50, inclusive=False, nnratio=1.0, use_elig1=True, use_elig2=True,
          check=None, stable_cut=True):
    return dict(name=name, frames=[f.build() if isinstance(f, FrameBuilder) else f for f in frames],
                pairs=[tuple(p) for p in pairs], th=th, inclusive=inclusive, nnratio=nnratio, use_elig1=use_elig1,
                use_elig2=use_elig2, check=check or (lambda res: None), stable_cut=stable_cut)


def _filler(j):
    """Far from every query used below: 60 + j % 5 bits of the low range."""
    return D(*R(0, 60 + j % 5))


# ---- run lengths ---------------------------------------------------------------------------------------------

def run2_case(L):
    """Side 2's run has L features; the best of q0 sits at the run's last position, the best of q1 in its middle."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    q0 = f1.add(7, D())
    q1 = f1.add(7, D(*R(200, 210)))
    f2.empty_node(7)
    want = {}
    for j in range(L):
        if j == L - 1:
            want[q0] = f2.add(7, D(0, 1, 2))
        elif j == L // 2:
            want[q1] = f2.add(7, D(*R(200, 210), 5))
        else:
            f2.add(7, _filler(j))

    def check(res):
        m12, m21, _, hist, n_raw = res[0]
        assert len(m21) == L
        assert n_raw == len(want) and hist[0] == n_raw
        for q, c in want.items():
            assert m12[q] == c and m21[c] == q
    return _case(f"run2_{L}", [f1, f2], check=check)


def run1_case(L):
    """Side 1's run has L features, each with a candidate of its own at distance 1 (the others at 9) among 45
    candidates in a fixed shuffled order."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    f1.empty_node(3)
    qs = [f1.add(3, D(*R(4 * k, 4 * k + 4))) for k in range(L)]
    order = np.random.Generator(np.random.PCG64(L)).permutation(45).tolist()
    pos = {}
    for j in order:
        pos[j] = f2.add(3, D(*R(4 * j, 4 * j + 4), 200 + j) if j < 40 else D(*R(160, 200 + j)))

    def check(res):
        m12, m21, _, _, n_raw = res[0]
        assert n_raw == L and len(m12) == L
        for k, q in enumerate(qs):
            assert m12[q] == pos[k]
    return _case(f"run1_{L}", [f1, f2], check=check)


# ---- eligibility ---------------------------------------------------------------------------------------------

def elig_cases():
    out = []
    f1, f2 = FrameBuilder(), FrameBuilder()
    f1.add(1, D())
    for j in range(5):
        f2.add(1, D(j), elig=0)
    out.append(_case("elig_no_candidate", [f1, f2], check=lambda res: _assert(res[0][4] == 0)))

    f1, f2 = FrameBuilder(), FrameBuilder()
    skipped = f1.add(1, D(), elig=0)          # would take the candidate at distance 0
    q = f1.add(1, D(1))
    for j in range(70):
        c = f2.add(1, D() if j == 66 else D(2, j + 10), elig=1 if j == 66 else 0)
        if j == 66:
            only = c

    def check(res, skipped=skipped, q=q, only=only):
        m12, m21, _, _, n_raw = res[0]
        assert n_raw == 1 and m12[skipped] == -1 and m12[q] == only and m21[only] == q
    out.append(_case("elig_only_in_second_chunk", [f1, f2], nnratio=0.7, check=check))

    f1, f2 = FrameBuilder(), FrameBuilder()
    q = f1.add(1, D())
    c = f2.add(1, D(0, 1, 2))
    # best2 stays 256: 3 < 0.02 * 256 holds, 3 < 0.01 * 256 does not
    out.append(_case("single_candidate_accept", [f1, f2], nnratio=0.02,
                     check=lambda res, q=q, c=c: _assert(res[0][0][q] == c)))
    out.append(_case("single_candidate_reject", [f1, f2], nnratio=0.01, check=lambda res: _assert(res[0][4] == 0)))

    # the kf_f form: side 2 carries eligibility bytes that must be ignored
    f1, f2 = FrameBuilder(), FrameBuilder()
    q = f1.add(1, D())
    c = f2.add(1, D(0), elig=0)
    out.append(_case("side2_eligibility_unused", [f1, f2], inclusive=True, use_elig2=False,
                     check=lambda res, q=q, c=c: _assert(res[0][0][q] == c)))
    return out


def _assert(cond):
    assert cond


# ---- ties ----------------------------------------------------------------------------------------------------

def tie_cases():
    out = []
    for name, n, pa, pb in (("in_chunk", 20, 3, 9), ("across_chunks", 80, 10, 70)):
        f1, f2 = FrameBuilder(), FrameBuilder()
        q = f1.add(2, D())
        idx = [f2.add(2, D(*R(100, 105)) if j == pa else D(*R(110, 115)) if j == pb else _filler(j)) for j in range(n)]
        first = idx[pa]
        out.append(_case(f"tie_{name}_rejected", [f1, f2], nnratio=1.0, check=lambda res: _assert(res[0][4] == 0)))
        out.append(_case(f"tie_{name}_first_wins", [f1, f2], nnratio=1.5,
                         check=lambda res, q=q, first=first: _assert(res[0][0][q] == first)))
    # run order not ascending in feature index: the first in RUN order wins, which is the larger index
    f1, f2 = FrameBuilder(), FrameBuilder()
    q = f1.add(2, D())
    a = f2.add(2, D(*R(100, 105)))
    f2.add(2, _filler(0))
    b = f2.add(2, D(*R(110, 115)))
    f2.reverse(2)
    out.append(_case("tie_run_order_descending", [f1, f2], nnratio=1.5,
                     check=lambda res: _assert(res[0][0][q] == b and b > a)))
    return out


# ---- blocking ------------------------------------------------------------------------------------------------

def blocking_case(k, nnratio):
    """k side-1 features whose best is c0; the later ones take their next best, with best2 over what remains."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    qs = [f1.add(5, d) for d in (D(1), D(1, 2), D(1, 2, 3))[:k]]
    cs = [f2.add(5, d) for d in (D(), D(1, 2, *R(10, 15)), D(1, 2, 3, *R(20, 28)), D(*R(40, 70)))]

    def check(res):
        m12, _, _, _, n_raw = res[0]
        assert n_raw == k and [int(m12[q]) for q in qs] == cs[:k]
    c = _case(f"blocking_{k}_nn{nnratio}", [f1, f2], nnratio=nnratio, check=check)
    free = oracle(c, block=False)[0][0]
    assert [int(free[q]) for q in qs] == [cs[0]] * k  # without blocking every one of them takes c0
    return c


# ---- thresholds and ratio ------------------------------------------------------------------------------------

def threshold_case(inclusive):
    f1, f2 = FrameBuilder(), FrameBuilder()
    qs = {}
    for node, d in enumerate((49, 50, 51)):
        qs[d] = (f1.add(node, D()), f2.add(node, D(*R(0, d))))

    def check(res):
        m12 = res[0][0]
        assert m12[qs[49][0]] == qs[49][1] and m12[qs[51][0]] == -1
        assert (m12[qs[50][0]] == qs[50][1]) == bool(inclusive)
    return _case(f"threshold_inclusive{int(inclusive)}", [f1, f2], inclusive=inclusive, check=check)


def ratio_case(pairs, nnratio):
    f1, f2 = FrameBuilder(), FrameBuilder()
    ent = []
    for node, (b1, b2) in enumerate(pairs):
        q = f1.add(node, D())
        f2.add(node, D(*R(100, 100 + b2)))
        c = f2.add(node, D(*R(0, b1)))
        ent.append((q, c, float(b1) < nnratio * float(b2)))  # Python's own double product decides the side

    def check(res):
        m12 = res[0][0]
        for q, c, acc in ent:
            assert m12[q] == (c if acc else -1)
    return _case(f"ratio_{nnratio}", [f1, f2], nnratio=nnratio, check=check)


# ---- rotation ------------------------------------------------------------------------------------------------

def half_bin_split():
    """float32 angles (a1, a2) whose difference the reference's rot * (1 / 30) and a division rot / 30 put in
    different bins, or None when the search finds none."""
    f = 1.0 / 30
    for k in range(12):
        for e in range(40, 60):
            for s in (-1.0, 1.0):
                a1, a2 = np.float32(30 * k + 15), np.float32(s * 2.0 ** -e)
                rot = float(a1) - float(a2)
                if rot >= 0.0 and round(rot * f) != round(rot / 30):
                    return a1, a2
    return None


def rotation_pairs():
    up = np.nextafter(np.float32(45), np.float32(400))
    lst = [(15.0, 0.0), (45.0, 0.0), (350.0, 5.0), (5.0, 20.0), (359.99, 0.0), (float(up), 0.0), (100.0, 25.0),
           (20.0, 215.0), (200.0, 20.0)]
    sp = half_bin_split()
    if sp is not None:
        lst.append((float(sp[0]), float(sp[1])))
    return lst


def rotation_case():
    """One match per node with the angle differences 15, 45, 345, -15, 359.99, one ulp above 45, 75, -195, 180 and
    the rot * (1 / 30) against rot / 30 split.  The bin counts come out 3, 3, 2, 2: the third and fourth ranks
    tie, so this case breaks the rotation-cut condition on purpose."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    ent = []
    for node, (a1, a2) in enumerate(rotation_pairs()):
        q = f1.add(node, D(), angle=a1)
        f2.add(node, D(1), angle=a2)
        rot = float(np.float32(a1)) - float(np.float32(a2))
        rot = rot + 360.0 if rot < 0.0 else rot
        b = round(rot * (1.0 / 30))
        ent.append((q, 0 if b == 30 else b, rot))

    def check(res):
        _, _, bin12, hist, n_raw = res[0]
        assert n_raw == len(ent) and [int(bin12[q]) for q, _, _ in ent] == [b for _, b, _ in ent]
        prod = [rot * (1.0 / 30) for _, _, rot in ent]
        assert any(p - np.floor(p) == 0.5 for p in prod)                      # a product exactly on k + 0.5
        assert any(round(rot * (1.0 / 30)) != round(rot / 30) for _, _, rot in ent)  # multiply, not divide
        assert sum(rot == 345.0 for _, _, rot in ent) == 2                    # 350 - 5 and 5 - 20 + 360
        assert not O.cut_is_stable(hist)
    return _case("rotation", [f1, f2], check=check, stable_cut=False)


# ---- node lists ----------------------------------------------------------------------------------------------

def node_list_cases():
    def frame(nodes):
        f = FrameBuilder()
        for k in nodes:
            f.add(k, D(k % 200))
        return f
    lists = dict(disjoint=([1, 3, 5], [2, 4, 6], 0), identical=([1, 3, 5], [1, 3, 5], 3), one_empty=([1, 3, 5], [], 0),
                 both_empty=([], [], 0), interleaved=([1, 2, 5, 8, 9, 12], [0, 2, 3, 8, 10, 12, 13], 3),
                 common_last=([1, 3, 9], [2, 4, 6, 9], 1),
                 many=(list(range(0, 60, 2)), list(range(0, 60, 3)), 10))
    out = []
    for name, (n1, n2, common) in lists.items():
        out.append(_case(f"nodes_{name}", [frame(n1), frame(n2)],
                         check=lambda res, common=common: _assert(res[0][4] == common)))
    # a frame with features but an empty feature vector, against itself and a full one
    f = frame([1, 2])
    e = frame([1, 2]).build()
    e.update(fv_node=np.zeros(0, np.int32), fv_end=np.zeros(0, np.int32), fv_idx=np.zeros(0, np.int32))
    out.append(_case("nodes_features_without_vector", [f, e], pairs=[(0, 1), (1, 0), (1, 1)],
                     check=lambda res: _assert([r[4] for r in res] == [0, 0, 0])))
    return out


# ---- frame sharing -------------------------------------------------------------------------------------------

def sharing_frames():
    rng = np.random.Generator(np.random.PCG64(99))
    frames = []
    for _ in range(4):
        f = FrameBuilder()
        for i in range(30):
            f.add(int(rng.integers(0, 6)), D(*rng.choice(256, int(rng.integers(0, 40)), replace=False).tolist()),
                  angle=0.0, elig=int(rng.random() < 0.8))
        frames.append(f.build())
    return frames


def sharing_cases():
    frames = sharing_frames()
    pairs = [(0, 3), (1, 3), (2, 3), (3, 0), (0, 0), (1, 2), (2, 1), (3, 3), (0, 1)]
    assert len(pairs) == WAVES + 1

    def check(res):
        assert all(r[4] > 0 for r in res)
        m12, m21 = res[4][0], res[4][1]  # a frame against itself: every eligible feature in a run meets itself
        assert any(m12[i] == i for i in range(len(m12))) and np.array_equal(m12 >= 0, m21 >= 0)
        assert not np.array_equal(res[0][1], res[1][1])  # frame 3 on side 2 of several pairs, each its own answer
    return [_case("sharing_one_pair", frames, pairs=pairs[:1], nnratio=0.9),
            _case("sharing_waves_plus_one_pairs", frames, pairs=pairs, nnratio=0.9, check=check)]


def all_cases():
    cases = [run2_case(L) for L in (0, 1, 2, 63, 64, 65, 127, 128, 129)]
    cases += [run1_case(L) for L in (0, 1, 40)]
    cases += elig_cases() + tie_cases()
    cases += [blocking_case(2, 1.0), blocking_case(3, 1.0), blocking_case(3, 0.6)]
    cases += [threshold_case(False), threshold_case(True)]
    cases += [ratio_case([(35, 50), (34, 50), (36, 50), (42, 60), (49, 70)], 0.7), ratio_case([(30, 50)], 0.6)]
    cases += [rotation_case()] + node_list_cases() + sharing_cases()
    return cases
