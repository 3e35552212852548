"""Generate the goldens of the BoW-guided match: tests/golden/bow_match_kf_kf.npz and bow_match_kf_f.npz.

Imports the REFERENCE ORBMatcher.py read-only from the directory given on the command line (it imports only
numpy) and runs its own search_by_BoW_kf_kf / search_by_BoW_kf_f on stand-in keyframes and frames
(tests/matcher_world.py) built from array frames: worlds of about 300 features per frame with map points that
are None or bad, and a subset of the crafted cases of tests/bow_match_cases.py.  Every feature that holds a
map point holds one of its own, so the returned map points name feature indices.  Each scene runs with nnratio
1 and 0.7 and the orientation check on and off; the input arrays, the returned match indices and the counts are
stored.  A scene whose rotation cut would hinge on how equal bin counts are ranked is refused: NumPy's argsort
order of equal counts is not portable, and these files are read on other hosts.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bow_match.py <reference directory>
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import bow_match_cases as BC  # noqa: E402
import bow_match_oracle as O  # noqa: E402
import matcher_world as MW  # noqa: E402

COMBOS = [(1.0, True), (1.0, False), (0.7, True), (0.7, False)]
KEYS = ("desc", "angle", "elig", "fv_node", "fv_end", "fv_idx")


def world_frame(a, slots, bad):
    """Array frame of a matcher_world keyframe: feature vector from its words, eligibility from its slots."""
    n = len(a["x"])
    f = BC.FrameBuilder()
    for i in range(n):
        f.add(int(a["word"][i]), a["desc"][i], float(a["angle"][i]), int(slots[i] >= 0 and not bad[slots[i]]))
    return f.build()


def world_scenes(seed, n, n_mp, n_words):
    rng = np.random.Generator(np.random.PCG64(seed))
    z = MW.make_world(rng, n_kf=2, n=n, n_mp=n_mp, with_frame=True, n_words=n_words)
    bad = z["mp_bad"].copy()
    bad[::7] = True  # make_world marks 3 % bad; these make the bad ones a visible share
    k0 = world_frame(MW.sub(_Arrays(z), "kf0_"), z["kfmp0"], bad)
    k1 = world_frame(MW.sub(_Arrays(z), "kf1_"), z["kfmp1"], bad)
    fr = world_frame(MW.sub(_Arrays(z), "fr_"), np.zeros(n, np.int32), np.zeros(len(bad), bool))
    # make_world's re-observations keep their angle (three bins at most): turn a share of them by multiples of
    # 30 degrees so that the rotation cut has something to drop
    for f in (k1, fr):
        turn = 30.0 * rng.integers(1, 12, n) * (rng.random(n) < 0.35)
        f["angle"] = ((f["angle"].astype(np.float64) + turn) % 360.0).astype(np.float32)
    return (k0, k1), (k0, fr)


class _Arrays:
    def __init__(self, d):
        self._d = d
        self.files = list(d.keys())

    def __getitem__(self, k):
        return self._d[k]


def stand_in(w, f, kid, with_points):
    """A matcher_world keyframe / frame over an array frame.  Eligible features hold a map point of their own;
    ineligible ones alternate between None and a bad map point."""
    n = len(f["desc"])
    a = dict(x=np.full(n, 100, np.float32), y=np.full(n, 100, np.float32), octave=np.zeros(n, np.int32),
             angle=f["angle"], desc=f["desc"], uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    kf = MW.Frame(w, a, np.eye(4, dtype=np.float32)) if kid < 0 else MW.KeyFrame(w, kid, a, np.eye(4, dtype=np.float32))
    kf.mFeatVec = O.runs(f)
    owner = {}
    if with_points:
        z3 = np.zeros(3, np.float32)
        for i in range(n):
            if f["elig"][i] or i % 2:
                mp = MW.MapPoint(w, len(w.mps), z3, f["desc"][i], z3, 1.0, 2.0, bad=not f["elig"][i])
                w.mps.append(mp)
                kf.mvpMapPoints[i] = mp
                owner[id(mp)] = i
    return kf, owner


def run_scene(RM, kind, f1, f2):
    res = {}
    for c, (nn, ori) in enumerate(COMBOS):
        w = MW.World()
        k1, own1 = stand_in(w, f1, 0, True)
        k2, own2 = stand_in(w, f2, 1 if kind == "kf_kf" else -1, kind == "kf_kf")
        m = RM.ORBMatcher(nn, ori)
        if kind == "kf_kf":
            n, lst = m.search_by_BoW_kf_kf(k1, k2)
            match = np.array([own2[id(p)] if p else -1 for p in lst], np.int32)  # match12
        else:
            n, lst = m.search_by_BoW_kf_f(k1, k2)
            match = np.array([own1[id(p)] if p else -1 for p in lst], np.int32)  # match21
        if ori:
            raw = O.match_pair(f1, f2, True, kind == "kf_kf", 50, kind == "kf_f", nn)
            if not O.cut_is_stable(raw[3]):
                raise SystemExit(f"{kind}: the rotation cut of this scene depends on how ties are ranked; not written")
        res[f"r{c}_n"] = np.int32(n)
        res[f"r{c}_match"] = match
    return res


def crafted():
    names = ("run2_65", "run2_129", "run1_40", "elig_only_in_second_chunk", "tie_across_chunks_first_wins",
             "tie_run_order_descending", "blocking_3_nn0.6", "threshold_inclusive0", "ratio_0.7", "nodes_interleaved",
             "sharing_one_pair")
    by = {c["name"]: c for c in BC.all_cases()}
    return [(by[k]["frames"][by[k]["pairs"][0][0]], by[k]["frames"][by[k]["pairs"][0][1]]) for k in names]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import ORBMatcher as RM  # noqa: E402
    kk_a, kf_a = world_scenes(9300, 300, 200, 40)
    kk_b, kf_b = world_scenes(9301, 320, 220, 4)  # runs of about 80 features: more than one chunk of 64
    for kind, scenes in (("kf_kf", [kk_a, kk_b] + crafted()), ("kf_f", [kf_a, kf_b] + crafted())):
        out = {"n_scenes": np.int32(len(scenes)), "nnratio": np.array([c[0] for c in COMBOS]),
               "check_ori": np.array([c[1] for c in COMBOS])}
        for s, (f1, f2) in enumerate(scenes):
            for side, f in (("f1", f1), ("f2", f2)):
                out.update({f"s{s}_{side}_{k}": f[k] for k in KEYS})
            res = run_scene(RM, kind, f1, f2)
            out.update({f"s{s}_{k}": v for k, v in res.items()})
            print(kind, s, len(f1["desc"]), len(f2["desc"]), [int(res[f"r{c}_n"]) for c in range(len(COMBOS))])
        np.savez_compressed(HERE / f"bow_match_{kind}.npz", **out)


if __name__ == "__main__":
    main()
