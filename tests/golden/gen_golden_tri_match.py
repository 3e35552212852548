"""Generate the golden of the triangulation match: tests/golden/tri_match.npz.

Imports the REFERENCE ORBMatcher.py read-only from the directory given on the command line (it imports only numpy)
and runs its own search_for_triangulation on a tests/matcher_world.py world: keyframe 0 against 8 neighbours of 300
features each, with nnratio 0.6 as LocalMapping constructs its matcher, bOnlyStereo off and on and the orientation
check on and off.  Most slots of keyframe 0 are emptied first (LocalMapping's shape: a fresh keyframe holds few map
points), positions are put on quarter pixels and angles on half degrees (tri_match_cases.quantise_world) so that
the world stores compactly, a share of the neighbours' angles is turned by 90 degrees or another multiple of 30 so
that the rotation cut has something to drop, and the neighbours' features that re-observe nothing get noisy copies
of keyframe 0's descriptors (a world that stores smaller).  The world (tri_match_cases.encode_world), every F12 and
every result list are stored; a search out of which StopIteration escaped is stored as stopped.  A world in which
a rotation cut would hinge on how equal bin counts are ranked is passed over for the next seed: NumPy's argsort
order of equal counts is not portable.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tri_match.py <reference directory>
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import matcher_world as MW  # noqa: E402
import tri_match_cases as TC  # noqa: E402
import tri_match_oracle as O  # noqa: E402

N_KF = 9
COMBOS = [(False, True), (False, False), (True, True), (True, False)]  # (bOnlyStereo, checkOri)


def make(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    z = MW.make_world(rng, n_kf=N_KF, n=300, n_mp=220, n_words=40)
    z["kfmp0"] = np.where(rng.random(300) < 0.75, -1, z["kfmp0"]).astype(np.int32)
    for j in range(1, N_KF):
        turn = np.where(rng.random(300) < 0.25, 90.0, 30.0 * rng.integers(1, 12, 300) * (rng.random(300) < 0.1))
        z[f"kf{j}_angle"] = ((z[f"kf{j}_angle"].astype(np.float64) + turn) % 360.0).astype(np.float32)
    # the neighbours' features that re-observe nothing get a noisy copy of some descriptor of keyframe 0 as well:
    # candidates within the distance threshold that only the two gates can refuse (and a world that stores smaller)
    for j in range(1, N_KF):
        for i in np.flatnonzero(TC.encode_world(TC.quantise_world(z, N_KF), N_KF)[f"kf{j}_src"] < 0).tolist():
            z[f"kf{j}_desc"][i] = MW.noisy_desc(rng, z["kf0_desc"][int(rng.integers(0, 300))], int(rng.integers(0, 24)))
    return TC.decode_world(TC.encode_world(TC.quantise_world(z, N_KF), N_KF))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import ORBMatcher as RM  # noqa: E402
    for seed in range(9500, 9600):  # the first world whose rotation cuts are all stable
        out = scene(RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with stable rotation cuts; not written")
    np.savez_compressed(HERE / "tri_match.npz", **out)
    print("seed", seed, (HERE / "tri_match.npz").stat().st_size, "bytes")


def scene(RM, seed):
    z = make(seed)
    out = TC.encode_world(z, N_KF)
    out["only_stereo"] = np.array([c[0] for c in COMBOS])
    out["check_ori"] = np.array([c[1] for c in COMBOS])
    frames = [TC.world_frame(z, j) for j in range(N_KF)]
    for j in range(1, N_KF):
        w = TC.build_world(z)
        F12 = MW.fundamental(w.kfs[0], w.kfs[j])
        out[f"F12_{j}"] = F12
        for c, (only, ori) in enumerate(COMBOS):
            w = TC.build_world(z)
            try:
                pairs = RM.ORBMatcher(0.6, ori).search_for_triangulation(w.kfs[0], w.kfs[j], F12, only)
                stop = 0
            except StopIteration:
                pairs, stop = [], 1
            raw = O.match_pair(frames[0], frames[j], F12, *TC.world_epipole(z["kf0_T"], z[f"kf{j}_T"]), 50, only)
            if ori and not stop and not O.cut_is_stable(raw[2]):
                print("seed", seed, "neighbour", j, ": the rotation cut depends on how ties are ranked")
                return None
            out[f"r{c}_{j}_pairs"] = np.array(pairs, np.int32).reshape(-1, 2)
            out[f"r{c}_{j}_stop"] = np.int32(stop)
            print(j, only, ori, "stop" if stop else len(pairs), "raw", int(raw[3]), "marginal", int(raw[4]))
    return out


if __name__ == "__main__":
    main()
