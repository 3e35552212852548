"""Generate the golden of tracking's motion-model search for many pairs: tests/golden/ff_many.npz.

Imports the REFERENCE Frame.py and ORBMatcher.py read-only from the directory given on the command line and runs the
reference's own ORBMatcher.search_by_projection_f_f on Frame.__new__ instances that share the attributes of the
stand-in frames of tests/ff_cases.py (so Frame.get_features_in_area is the reference's too).  Six (current frame, last
frame) pairs of 300 features each in the camera of the matcher goldens: the last frame stands still, ahead of or behind
the current one (all three motion modes, twice), the poses and positions are float32 in the first three pairs and
float64 in the others, th is 7 or 15.  Most current features have a right coordinate that agrees with the depth of the
point aimed at them; some disagree by more than a radius, so the stereo gate decides.  Some current slots are filled
before the call, by points with and without observations; three in ten last-frame points have no observations, so a
later point can overwrite them.  Nearly every last-frame point is aimed at a current feature of its own; a few share
one, which makes a point overtake another.

Seeds are searched until the array oracle with its redo (tests/ff_oracle.py) reproduces the reference on every pair,
every pair assigns at least 20 points, some item is redone because its feature was taken, some feature is assigned
twice, and the items redone (marked, overtaken, not expressible) number more than 0 and fewer than 5 % of the items
sent; a file that breaks any of this is not written.  Stored per pair, under the prefix p<k>_, in the layout of
matcher_ff_*.npz: the two frames' arrays, the poses, the last frame's points, what was filled in before, th, and the
reference's match count and the slots it leaves behind.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ff_many.py <reference directory>
"""
from __future__ import annotations

import sys
import types
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import ff_cases as FC  # noqa: E402
import ff_oracle as FO  # noqa: E402
from conftest import BF, FX  # noqa: E402

N = 300
W, H = 1241, 376


def frame_arrays(rng, n):
    return dict(x=rng.uniform(20, W - 20, n).astype(np.float32), y=rng.uniform(20, H - 20, n).astype(np.float32),
                octave=rng.integers(0, FC.LEVELS, n).astype(np.int32), angle=rng.uniform(0, 360, n).astype(np.float32),
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), uR=np.full(n, -1.0, np.float32))


def pose(rng, dtype):
    a = rng.normal(0, 0.02, 3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    U, _, Vt = np.linalg.svd(np.eye(3) + K + K @ K / 2)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = (U @ Vt).astype(dtype)
    T[:3, 3] = rng.normal(0, 0.3, 3).astype(dtype)
    return T


def noisy(rng, d, bits):
    d = d.copy()
    for b in rng.choice(256, bits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def pair(rng, k, N=N, dtype=None):
    """The arrays of pair k: N features a frame; dtype (default: float32 for k < 3, else float64) is the poses' and the
    positions'."""
    dtype = dtype or (np.float32 if k < 3 else np.float64)
    ca, la = frame_arrays(rng, N), frame_arrays(rng, N)
    la["desc"][:] = 0   # the search never reads the last frame's own descriptors, and zeros compress
    Tc = pose(rng, dtype)
    Tl = Tc.copy()
    Tl[2, 3] += dtype([0.0, 0.9, -0.9][k % 3])
    Rcw, tcw = Tc[:3, :3].astype(np.float64), Tc[:3, 3].astype(np.float64)
    cx, cy = 607.1928, 185.2157
    mpos, mdesc = np.zeros((N, 3), dtype), np.zeros((N, 32), np.uint8)
    has, outl, obs = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, np.int32)
    target = rng.permutation(N)
    depth = rng.uniform(3, 40, N)
    for i in range(N):
        if rng.random() < 0.1:
            continue
        j = int(target[i]) if rng.random() < 0.96 else int(target[rng.integers(0, N)])   # a few share a feature
        z = float(depth[j])
        u, v = ca["x"][j] + rng.normal(0, 1.5), ca["y"][j] + rng.normal(0, 1.5)
        pc = np.array([(u - cx) * z / FX, (v - cy) * z / FX, z])
        mpos[i] = (Rcw.T @ (pc - tcw)).astype(dtype)
        mdesc[i] = noisy(rng, ca["desc"][j], int(rng.integers(0, 40))) if rng.random() < 0.9 else rng.integers(
            0, 256, 32, dtype=np.uint8)
        la["octave"][i] = int(np.clip(ca["octave"][j] + rng.integers(-1, 2), 0, FC.LEVELS - 1))
        la["angle"][i] = np.float32((ca["angle"][j] + (rng.normal(0, 3) if rng.random() < 0.85 else rng.uniform(0, 360)))
                                    % 360.0)
        has[i] = True
        outl[i] = rng.random() < 0.05
        obs[i] = int(rng.choice([0, 1, 2, 3], p=[0.3, 0.2, 0.3, 0.2]))
    # right coordinates: most agree with the depth of the point aimed at the feature, some are off by more than a radius
    for j in range(N):
        r = rng.random()
        if r < 0.85:
            ca["uR"][j] = np.float32(ca["x"][j] - BF / depth[j] + (rng.normal(0, 1.0) if r < 0.7 else rng.choice(
                [-1, 1]) * rng.uniform(8, 60)))
        elif r < 0.9:
            ca["uR"][j] = np.float32(0.0)
    pre, pre_obs = np.full(N, -1, np.int32), np.zeros(N, np.int32)
    for n, j in enumerate(rng.choice(N, 24, replace=False)):
        pre[j], pre_obs[j] = n, int(rng.choice([0, 2]))
    out = dict(th=np.float64([7.0, 15.0][k % 2]), Tc=Tc, Tl=Tl, mp_pos=mpos, mp_desc=mdesc, mp_has=has, mp_outlier=outl,
               mp_obs=obs, pre=pre, pre_obs=pre_obs)
    out.update({f"cur_{key}": v for key, v in ca.items()})
    out.update({f"last_{key}": v for key, v in la.items()})
    return out


class Npz(dict):
    @property
    def files(self):
        return list(self)


def scene(RFrame, RM, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    z = Npz()
    for k in range(FC.N_PAIRS):
        z.update({f"p{k}_{key}": v for key, v in pair(rng, k).items()})

    def twin(F):
        f = RFrame.Frame.__new__(RFrame.Frame)
        f.__dict__ = F.__dict__
        return f
    jobs, objs = FC.load_world(z)
    ref = [RM.ORBMatcher(0.8, True).search_by_projection_f_f(twin(c), twin(x), th) for c, x, th in jobs]
    left = FC.state(jobs, objs)
    jobs, objs = FC.load_world(z)
    stats = {}
    mine = FO.replay(jobs, stats=stats)
    assert FC.same((mine, FC.state(jobs, objs)), (ref, left)), ("oracle against the reference", seed, mine, ref)
    for k in range(FC.N_PAIRS):
        z[f"p{k}_n_matches"], z[f"p{k}_assigned"] = np.int64(ref[k]), left[k]
    share = len(stats["redone"]) / max(stats["items"], 1)
    print("seed", seed, "matches", ref, {key: (len(v) if key == "redone" else v) for key, v in stats.items()},
          "redone share %.4f" % share)
    modes = [FO.mode_of(c, x) for c, x, _ in jobs]
    assert modes == [0, 1, 2, 0, 1, 2], modes
    if not (min(ref) >= 20 and stats["taken"] > 0 and stats["twice"] > 0 and 0 < share < FC.REDO_CAP):
        return None
    return z


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, sys.argv[1])
    import Frame as RFrame  # noqa: E402
    import ORBMatcher as RM  # noqa: E402
    warnings.simplefilter("ignore")
    for seed in range(7100, 7200):
        out = scene(RFrame, RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with the wanted events; not written")
    np.savez_compressed(HERE / "ff_many.npz", **out)
    print("seed", seed, (HERE / "ff_many.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
