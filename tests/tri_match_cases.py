"""Cases for k_tri_match: crafted descriptors (bit flips of one base row give exact Hamming distances), hand-written
CSR feature vectors and a geometry in which both gates are decided by small integers.  Each case carries the claim
it exists for as a `check` over the array oracle's results, which tests/test_tri_match_cpu.py runs, so the GPU test
that compares the kernel with the oracle cannot pass on inputs that miss the situation.

Geometry.  F_ROW makes the epipolar line of (x1, y1) the row y = y1 (a = 0, b = 1, c = -y1), so the line test is
(y2 - y1)^2 < thr_epi[octave2]: with thr_epi[0] = 3.84 a candidate on the same row passes and one five rows away
fails.  The epipole is FAR unless a case puts it near a candidate; thr_ex[0] = 100 is a radius of ten pixels.

A case: name, frames (tri_match_oracle frame dicts), pairs [(f1, f2)], F12 and epi per pair, th, only_stereo,
check(results) with results[p] = (match12, bin12, hist, n_raw, status, stopped), and empty (True for the cases built
to produce no match).
"""
from __future__ import annotations

import numpy as np

import tri_match_oracle as O
from bow_match_cases import D, R, _filler

WAVES = 8   # waves per k_tri_match workgroup (kTmWaves): visited node pairs of one keyframe pair in flight
CHUNK = 64  # features of frame 2's run a wave looks at per step; the first chunk stays in registers

F_ROW = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
FAR = (-1000.0, -1000.0)
THR_EX = [float(100 * s) for s in (1.0, 1.2, 1.44)]
THR_EPI = [float(3.84 * s) for s in (1.0, 1.44, 2.0736)]


class FrameBuilder:
    def __init__(self):
        self.desc, self.angle, self.xy, self.octave, self.flags, self.nodes = [], [], [], [], [], {}

    def add(self, node, desc, x=10.0, y=50.0, stereo=False, free=True, octave=0, angle=0.0):
        i = len(self.desc)
        self.desc.append(desc)
        self.angle.append(angle)
        self.xy.append((x, y))
        self.octave.append(octave)
        self.flags.append((O.ELIGIBLE if free else 0) | (O.STEREO if stereo else 0))
        self.nodes.setdefault(node, []).append(i)
        return i

    def build(self, thr_epi=THR_EPI, thr_ex=THR_EX):
        nodes = sorted(self.nodes)
        idx = [i for k in nodes for i in self.nodes[k]]
        return dict(desc=np.array(self.desc, np.uint8).reshape(-1, 32), angle=np.array(self.angle, np.float32),
                    xy=np.array(self.xy, np.float64).reshape(-1, 2), octave=np.array(self.octave, np.int32),
                    flags=np.array(self.flags, np.uint8), fv_node=np.array(nodes, np.int32),
                    fv_end=np.cumsum([len(self.nodes[k]) for k in nodes]).astype(np.int32),
                    fv_idx=np.array(idx, np.int32), thr_epi=np.array(thr_epi, np.float64),
                    thr_ex=np.array(thr_ex, np.float64))


def pack(frames):
    """The host entry's arrays of a list of frames."""
    def cat(k, dt):
        return np.concatenate([f[k] for f in frames]).astype(dt) if frames else np.zeros(0, dt)
    offs = {}
    for name, key in (("off", "desc"), ("fv_off", "fv_node"), ("lvl_off", "thr_epi")):
        offs[name] = np.zeros(len(frames) + 1, np.int64)
        np.cumsum([len(f[key]) for f in frames], out=offs[name][1:])
    fv_idx = np.zeros(int(offs["off"][-1]), np.int32)
    for k, f in enumerate(frames):
        fv_idx[offs["off"][k]:offs["off"][k] + len(f["fv_idx"])] = f["fv_idx"]
    return dict(desc=cat("desc", np.uint8).reshape(-1, 32), angle=cat("angle", np.float32),
                xy=cat("xy", np.float64).reshape(-1, 2), octave=cat("octave", np.int32), flags=cat("flags", np.uint8),
                fv_node=cat("fv_node", np.int32), fv_end=cat("fv_end", np.int32), fv_idx=fv_idx,
                thr_epi=cat("thr_epi", np.float64), thr_ex=cat("thr_ex", np.float64), **offs)


def oracle(case, **kw):
    return [O.match_pair(case["frames"][a], case["frames"][b], F, e[0], e[1], case["th"], case["only_stereo"], **kw)
            for (a, b), F, e in zip(case["pairs"], case["F12"], case["epi"])]


def _case(name, frames, pairs=((0, 1),), F12=None, epi=None, th=50, only_stereo=False, check=None, empty=False):
    pairs = [tuple(p) for p in pairs]
    return dict(name=name, frames=[f.build() if isinstance(f, FrameBuilder) else f for f in frames], pairs=pairs,
                F12=[F_ROW] * len(pairs) if F12 is None else list(F12),
                epi=[FAR] * len(pairs) if epi is None else list(epi),
                th=th, only_stereo=only_stereo, check=check or (lambda res: None), empty=empty)


def _assert(cond):
    assert cond


# ---- run lengths ---------------------------------------------------------------------------------------------

def run2_case(L):
    """Frame 2's run has L features; the best of q0 sits at the run's last position, the best of q1 in its middle."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    q0 = f1.add(7, D())
    q1 = f1.add(7, D(*R(200, 210)))
    want = {}
    for j in range(L):
        if j == L - 1:
            want[q0] = f2.add(7, D(0, 1, 2))
        elif j == L // 2:
            want[q1] = f2.add(7, D(*R(200, 210), 5))
        else:
            f2.add(7, _filler(j))

    def check(res):
        m12, _, hist, n_raw = res[0][:4]
        assert n_raw == len(want) and hist[0] == n_raw
        for q, c in want.items():
            assert m12[q] == c
    return _case(f"run2_{L}", [f1, f2], check=check)


# ---- ties: the last minimum wins -----------------------------------------------------------------------------

def tie_cases():
    out = []
    for name, n, pa, pb in (("in_chunk", 20, 3, 9), ("across_chunks", 80, 10, 70)):
        f1, f2 = FrameBuilder(), FrameBuilder()
        q = f1.add(2, D())
        idx = [f2.add(2, D(*R(100, 105)) if j == pa else D(*R(110, 115)) if j == pb else _filler(j)) for j in range(n)]
        out.append(_case(f"tie_{name}_last_wins", [f1, f2],
                         check=lambda res, q=q, last=idx[pb]: _assert(res[0][0][q] == last)))
    return out


# ---- threshold -----------------------------------------------------------------------------------------------

def threshold_case():
    f1, f2 = FrameBuilder(), FrameBuilder()
    qs = {}
    for node, d in enumerate((49, 50, 51)):
        qs[d] = (f1.add(node, D()), f2.add(node, D(*R(0, d))))

    def check(res):
        m12 = res[0][0]
        assert m12[qs[49][0]] == qs[49][1] and m12[qs[50][0]] == qs[50][1] and m12[qs[51][0]] == -1
    return _case("threshold_50_taken_51_not", [f1, f2], check=check)


# ---- blocking ------------------------------------------------------------------------------------------------

def blocking_case():
    """Two features of frame 1 whose best is c0; the second takes its next best."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    qs = [f1.add(5, d) for d in (D(1), D(1, 2))]
    cs = [f2.add(5, d) for d in (D(), D(1, 2, *R(10, 15)), D(*R(40, 70)))]

    def check(res):
        assert [int(res[0][0][q]) for q in qs] == cs[:2]
    c = _case("blocking", [f1, f2], check=check)
    free = oracle(c, block=False)[0][0]
    assert [int(free[q]) for q in qs] == [cs[0]] * 2  # without blocking both take c0
    return c


# ---- the two gates -------------------------------------------------------------------------------------------

def line_gate_case():
    """The nearer candidate lies five rows off the epipolar line, the farther one on it; a third sits just inside
    the gate of its octave (1.44 * 3.84 = 5.53 > 2.3^2) where octave 0 would refuse it."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    q = f1.add(1, D(), y=50.0)
    off_line = f2.add(1, D(0), y=55.0)
    on_line = f2.add(1, D(*R(0, 9)), y=50.0)
    q2 = f1.add(2, D(), y=80.0)
    refused = f2.add(2, D(0), y=82.3, octave=0)
    coarse = f2.add(2, D(0, 1), y=82.3, octave=1)

    def check(res):
        m12 = res[0][0]
        assert m12[q] == on_line and m12[q2] == coarse and off_line != on_line and refused != coarse
    return _case("line_gate", [f1, f2], check=check)


def epipole_gate_case():
    """Per node one feature of frame 1 and two candidates: the nearer one three pixels from the epipole, the farther
    one far from it.  Only when both features are mono does the epipole gate refuse the nearer one."""
    f1, f2 = FrameBuilder(), FrameBuilder()
    ent = []
    for node, (s1, s2) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        q = f1.add(node, D(), x=300.0, y=100.0, stereo=s1)
        near = f2.add(node, D(0), x=103.0, y=100.0, stereo=s2)
        far = f2.add(node, D(*R(0, 9)), x=400.0, y=100.0, stereo=s2)
        ent.append((q, far if not s1 and not s2 else near))

    def check(res):
        assert [int(res[0][0][q]) for q, _ in ent] == [w for _, w in ent]
    return _case("epipole_gate_only_when_both_mono", [f1, f2], epi=[(100.0, 100.0)], check=check)


def only_stereo_case():
    f1, f2 = FrameBuilder(), FrameBuilder()
    mono1 = f1.add(1, D(), stereo=False)           # skipped: would take the mono candidate at distance 1
    st1 = f1.add(1, D(1, 2), stereo=True)
    mono2 = f2.add(1, D(1), stereo=False)          # skipped, although nearest to both
    st2 = f2.add(1, D(*R(0, 12)), stereo=True)

    def check(res):
        m12 = res[0][0]
        assert m12[mono1] == -1 and m12[st1] == st2 and mono2 != st2
    c = _case("only_stereo_both_sides", [f1, f2], only_stereo=True, check=check)
    loose = oracle(dict(c, only_stereo=False))[0][0]
    assert loose[mono1] == mono2  # without the flag the mono features match each other
    return c


def map_point_case():
    f1, f2 = FrameBuilder(), FrameBuilder()
    held1 = f1.add(1, D(), free=False)             # holds a map point: skipped
    q = f1.add(1, D(1))
    held2 = f2.add(1, D(1), free=False)            # holds a map point: no candidate, although at distance 0
    c = f2.add(1, D(*R(0, 7)))

    def check(res):
        m12 = res[0][0]
        assert m12[held1] == -1 and m12[q] == c and held2 != c
    return _case("map_point_on_either_side", [f1, f2], check=check)


def zero_f12_case():
    f1, f2 = FrameBuilder(), FrameBuilder()
    f1.add(1, D())
    f2.add(1, D(0))
    return _case("zero_F12_no_match", [f1, f2], F12=[np.zeros((3, 3))], empty=True,
                 check=lambda res: _assert(res[0][3] == 0 and res[0][4] == 0))


# ---- the walk ------------------------------------------------------------------------------------------------

def _node_frame(nodes, bit):
    f = FrameBuilder()
    for k in nodes:
        f.add(k, D(k % 200, bit))
    return f


def walk_cases():
    out = []
    n1, n2 = [0, 1, 3, 7, 9], [0, 2, 3, 7, 9]
    vis, stopped = O.walk(n1, n2)
    assert not stopped and [n1[a] for a, _ in vis] == [0, 9] and O.merge_common(n1, n2) == [0, 3, 7, 9]

    def check(res):
        m12 = res[0][0]
        assert res[0][3] == 2 and m12[0] == 0 and m12[4] == 4 and m12[2] == -1 and m12[3] == -1
    out.append(_case("walk_skips_common_nodes", [_node_frame(n1, 250), _node_frame(n2, 251)], check=check))
    assert O.walk([1], [2]) == ([], True) and O.walk([0, 5], [0, 6]) == ([], True)
    out.append(_case("walk_stops", [_node_frame([0, 5], 250), _node_frame([0, 6], 251)], empty=True,
                     check=lambda res: _assert(res[0][5] == 1 and res[0][3] == 0 and (res[0][0] == -1).all())))
    many = list(range(0, 3 * WAVES - 4))
    out.append(_case("more_nodes_than_waves", [_node_frame(many, 250), _node_frame(many, 251)],
                     check=lambda res: _assert(res[0][3] == len(many) > WAVES)))
    return out


# ---- frame sharing -------------------------------------------------------------------------------------------

def sharing_frames():
    """Four random frames on the rows 50, 51 and 60 (row differences 0, 1 pass every octave's line test, 9 and 10
    none) with integer columns around an epipole at (100.5, 50.25), so that no gate comes near its threshold."""
    rng = np.random.Generator(np.random.PCG64(77))
    frames = []
    for _ in range(4):
        f = FrameBuilder()
        for _i in range(40):
            f.add(int(rng.integers(0, 6)), D(*rng.choice(256, int(rng.integers(0, 25)), replace=False).tolist()),
                  x=float(rng.integers(90, 130)), y=float(rng.choice([50, 51, 60])), stereo=bool(rng.random() < 0.4),
                  free=bool(rng.random() < 0.8), octave=int(rng.integers(0, 3)),
                  angle=float(np.float32(rng.choice([0.0, 10.0, 95.0, 200.0]))))
        frames.append(f.build())
    return frames


SHARING_PAIRS = [(0, 3), (1, 3), (2, 3), (3, 0), (0, 0), (1, 2), (2, 1), (3, 3), (0, 1)]


def sharing_cases():
    frames = sharing_frames()
    pairs = SHARING_PAIRS
    assert len(pairs) == WAVES + 1
    epi = [(100.5, 50.25)] * len(pairs)

    def check(res):
        assert all(r[3] > 0 and r[4] == 0 and r[5] == 0 for r in res)
        m12 = res[4][0]  # a frame against itself: a free feature meets itself at distance 0
        assert any(m12[i] == i for i in range(len(m12)))
        assert not np.array_equal(res[0][0], res[8][0])  # frame 0 on side 1 of several pairs, each its own answer
        assert len({int(b) for r in res for b in r[1] if b >= 0}) > 2
    return [_case("sharing_nine_pairs", frames, pairs=pairs, epi=epi, check=check),
            _case("sharing_nine_pairs_only_stereo", frames, pairs=pairs, epi=epi, only_stereo=True,
                  check=lambda res: _assert(sum(r[3] for r in res) > 0))]


# ---- empty frames --------------------------------------------------------------------------------------------

def empty_frame_case():
    e = FrameBuilder().build()
    f = FrameBuilder()
    f.add(1, D())
    return _case("empty_frames", [f, e], pairs=[(0, 1), (1, 0), (1, 1)], empty=True,
                 check=lambda res: _assert([r[3] for r in res] == [0, 0, 0]))


# ---- marginal ------------------------------------------------------------------------------------------------

def marginal_case():
    """Three pairs over three frames; in pair 1 the line test's left side is exactly its threshold (thr_epi = 4.0,
    y2 - y1 = 2.0), the other two are clear of it."""
    f1, f2, f3 = FrameBuilder(), FrameBuilder(), FrameBuilder()
    f1.add(1, D(), y=50.0)
    f2.add(1, D(0), y=52.0)
    f3.add(1, D(0, 1), y=50.0)
    thr = [4.0, 4.0, 4.0]
    frames = [f1.build(thr_epi=thr), f2.build(thr_epi=thr), f3.build(thr_epi=thr)]

    def check(res):
        assert [r[4] for r in res] == [0, O.MARGINAL, 0] and [r[3] for r in res] == [1, 0, 1]
    return _case("marginal", frames, pairs=[(0, 2), (0, 1), (1, 1)], check=check)


def all_cases():
    cases = [run2_case(L) for L in (1, 63, 64, 65, 129)]
    cases += tie_cases() + [threshold_case(), blocking_case(), line_gate_case(), epipole_gate_case()]
    cases += [only_stereo_case(), map_point_case(), zero_f12_case()] + walk_cases() + sharing_cases()
    cases += [empty_frame_case(), marginal_case()]
    return cases


# ---- matcher_world worlds as array frames, and their compact storage (tests/golden/tri_match.npz) ------------

def quantise_world(z, n_kf):
    """Keypoint positions to quarter pixels (none below 0), angles to half degrees, in place: they then store as 16-bit integers."""
    for j in range(n_kf):
        for k, q in (("x", 4.0), ("y", 4.0), ("angle", 2.0)):
            v = np.maximum(z[f"kf{j}_{k}"].astype(np.float64), 0.0)
            z[f"kf{j}_{k}"] = (np.round(v * q) / q).astype(np.float32)
        z[f"kf{j}_angle"] = (z[f"kf{j}_angle"] % np.float32(360)).astype(np.float32)
        z[f"kf{j}_uR"] = np.where(z[f"kf{j}_uR"] >= 0, 1.0, -1.0).astype(np.float32)  # only the sign is read
    return z


def encode_world(z, n_kf):
    """The arrays search_for_triangulation reads, compactly: descriptors of keyframes 1.. as the XOR with their
    nearest descriptor of keyframe 0 where that is close (re-observations differ from their source in a few bits)."""
    out = {"n_kf": np.int32(n_kf)}
    d0 = z["kf0_desc"]
    b0 = np.unpackbits(d0, axis=1).astype(np.int16)
    for j in range(n_kf):
        for k, q in (("x", 4.0), ("y", 4.0), ("angle", 2.0)):
            v = z[f"kf{j}_{k}"].astype(np.float64) * q
            assert np.array_equal(v, np.round(v)) and v.min() >= 0 and v.max() < 65536
            out[f"kf{j}_{k}"] = v.astype(np.uint16)
        out[f"kf{j}_octave"] = z[f"kf{j}_octave"].astype(np.uint8)
        assert z[f"kf{j}_word"].max() < 256
        out[f"kf{j}_word"] = z[f"kf{j}_word"].astype(np.uint8)
        out[f"kf{j}_stereo"] = z[f"kf{j}_uR"] >= 0
        out[f"kf{j}_held"] = z[f"kfmp{j}"] >= 0
        out[f"kf{j}_T"] = z[f"kf{j}_T"].astype(np.float32)
        d = z[f"kf{j}_desc"]
        if j == 0:
            out["kf0_desc"] = d
            continue
        bj = np.unpackbits(d, axis=1).astype(np.int16)
        dist = bj.sum(1)[:, None] + b0.sum(1)[None, :] - 2 * (bj @ b0.T)
        src = dist.argmin(1)
        src = np.where(dist[np.arange(len(d)), src] <= 48, src, -1).astype(np.int16)
        out[f"kf{j}_src"] = src
        out[f"kf{j}_desc"] = np.where((src >= 0)[:, None], d ^ d0[np.maximum(src, 0)], d)
    return out


def decode_world(g):
    """matcher_world arrays (z of matcher_world.build, without map points' own data) from encode_world's."""
    n_kf = int(g["n_kf"])
    z = {"n_kf": np.int32(n_kf)}
    d0 = g["kf0_desc"]
    for j in range(n_kf):
        for k, q in (("x", 4.0), ("y", 4.0), ("angle", 2.0)):
            z[f"kf{j}_{k}"] = (g[f"kf{j}_{k}"].astype(np.float64) / q).astype(np.float32)
        z[f"kf{j}_octave"] = g[f"kf{j}_octave"].astype(np.int32)
        z[f"kf{j}_word"] = g[f"kf{j}_word"].astype(np.int32)
        z[f"kf{j}_uR"] = np.where(g[f"kf{j}_stereo"], 1.0, -1.0).astype(np.float32)
        z[f"kf{j}_T"] = g[f"kf{j}_T"]
        held = g[f"kf{j}_held"]
        z[f"kfmp{j}"] = np.where(held, np.cumsum(held) - 1, -1).astype(np.int32)
        if j == 0:
            z["kf0_desc"] = d0
        else:
            src = g[f"kf{j}_src"].astype(np.int64)
            d = g[f"kf{j}_desc"]
            z[f"kf{j}_desc"] = np.where((src >= 0)[:, None], d ^ d0[np.maximum(src, 0)], d)
    return z


def build_world(z):
    """Keyframes of matcher_world over z; every held slot gets a map point of its own (only its truthiness is read)."""
    import matcher_world as MW
    w = MW.World()
    z3 = np.zeros(3, np.float32)
    for j in range(int(z["n_kf"])):
        a = {k: z[f"kf{j}_{k}"] for k in ("x", "y", "octave", "angle", "desc", "uR", "word")}
        kf = MW.KeyFrame(w, j, a, z[f"kf{j}_T"])
        for i in np.flatnonzero(z[f"kfmp{j}"] >= 0).tolist():
            mp = MW.MapPoint(w, len(w.mps), z3, a["desc"][i], z3, 1.0, 2.0)
            w.mps.append(mp)
            kf.mvpMapPoints[i] = mp
        w.kfs.append(kf)
    return w


def world_frame(z, j):
    """Keyframe j of z as an oracle frame, from the arrays alone."""
    import matcher_world as MW
    f = FrameBuilder()
    a = {k: z[f"kf{j}_{k}"] for k in ("x", "y", "octave", "angle", "desc", "uR", "word")}
    for i in range(len(a["x"])):
        f.add(int(a["word"][i]), a["desc"][i], x=float(a["x"][i]), y=float(a["y"][i]), stereo=bool(a["uR"][i] >= 0),
              free=bool(z[f"kfmp{j}"][i] < 0), octave=int(a["octave"][i]), angle=float(a["angle"][i]))
    return f.build(thr_epi=[float(3.84 * s) for s in MW.SIG2], thr_ex=[float(100 * s) for s in MW.SF])


def world_epipole(T1, T2):
    """The epipole of camera 1 in keyframe 2 as search_for_triangulation computes it from float32 poses
    (ORBMatcher.py:589-595), widened."""
    import matcher_world as MW
    T1, T2 = T1.astype(np.float32), T2.astype(np.float32)
    Cw = -T1[:3, :3].T @ T1[:3, 3:4]
    C2 = T2[:3, :3] @ Cw + T2[:3, 3:4]
    invz = 1.0 / C2[2]
    ex = MW.FX * C2[0] * invz + MW.CX
    ey = MW.FY * C2[1] * invz + MW.CY
    return float(ex.item()), float(ey.item())
