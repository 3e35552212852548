"""Generate the golden of loop closing's Sim3 projection searches: tests/golden/scw_many.npz.

Imports the REFERENCE ORBMatcher.py read-only from the directory given on the command line (it imports only numpy)
and runs its own functions on a tests/fuse_cases.py clone_world of 7 keyframes with 300 features each.

Run (a), LoopClosing.search_and_fuse (LoopClosing.py:352-367): fuse_kf_scw_mp of keyframe 0's map points into
keyframes 1..n with th = 4, each keyframe with an Scw of its own (its pose times 1.0, 1.1 or 0.9), and after each
keyframe the replace loop; n = 1, 3 and 6 on fresh builds, and n = 6 once more without the replace loop (prefix p).
Run (b), LoopClosing.compute_sim3's search_by_projection_ckf_scw_mp of every map point into keyframe 1 with th = 10
and about a third of vpMatched pre-filled.

Seeds are searched until run (a) with 6 keyframes has at least 20 replacements, a point skipped in a later keyframe
because a replace after an earlier one put it there, and an item replayed after its point's descriptor changed, and
run (b) has an item whose best candidate an earlier point of the call took.  The array oracle with its replays
(tests/scw_oracle.py) must reproduce the reference's results on the stored world, with at most 2 % of the items that
reach a cell window marked marginal.  Stored: the world's arrays, the Scws, the pre-filled vpMatched, and per run the
return values, the vpReplacePoint / vpMatched encodings, the event log, the final slots, the bad flags and the
descriptors.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_scw.py <reference directory>
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import fuse_cases as FC  # noqa: E402
import matcher_world as MW  # noqa: E402
import scw_cases as SC  # noqa: E402
import scw_oracle as SO  # noqa: E402


def scene(RM, seed):
    z = FC.clone_world(seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for j in range(1, FC.N_KF):
        z[f"Scw{j}"] = MW.sim3(z[f"kf{j}_T"], SC.SCALES[(j - 1) % 3])
    z["ckf_Scw"] = MW.sim3(z["kf1_T"], 1.1)
    n_feat, n_mp = len(z["kf1_x"]), len(z["mp_desc"])
    pre = np.full(n_feat, -1, np.int32)
    for i in rng.choice(n_feat, n_feat // 3, replace=False).tolist():
        pre[i] = z["kfmp1"][i] if z["kfmp1"][i] >= 0 else rng.integers(0, n_mp)
    z["ckf_pre"] = pre
    zz = FC.Z(z)
    m = RM.ORBMatcher()
    out = dict(z)
    for n, prefix, after in [(n, "n", True) for n in SC.N_KFS] + [(6, "p", False)]:
        w = MW.build(zz)
        state = SC.fuse_state(w, SC.drive_fuse(w, zz, SC.loop_fuse(m.fuse_kf_scw_mp), n, after))
        stats = {}
        w2 = MW.build(zz)
        mine = SC.fuse_state(w2, SC.drive_fuse(
            w2, zz, lambda kfs, S, pts, th, aft: SO.replay_fuse(kfs, S, pts, th, aft, stats=stats), n, after))
        SC.assert_state(mine, state, f"oracle against the reference, {prefix}{n}")
        out.update({f"{prefix}{n}_{k}": v for k, v in state.items()})
        if prefix == "n" and n == 6:
            fuse_stats, n_replace = stats, int((state["log"][:, 0] == MW.EV_REPLACE).sum())
    ckf_stats = {}
    n_ref, vm_ref = SC.drive_ckf(MW.build(zz), zz, m.search_by_projection_ckf_scw_mp)
    n_mine, vm_mine = SC.drive_ckf(MW.build(zz), zz, lambda kf, S, pts, vm, th: SO.replay_ckf(kf, S, pts, vm, th,
                                                                                            stats=ckf_stats))
    assert n_ref == n_mine and np.array_equal(vm_ref, vm_mine), "oracle against the reference, ckf"
    out["ckf_n"], out["ckf_matched"] = np.int32(n_ref), vm_ref
    share = max(s["marginal"] / max(s["reached"], 1) for s in (fuse_stats, ckf_stats))
    print("seed", seed, "replace", n_replace, fuse_stats, "ckf", n_ref, ckf_stats, "marginal share %.4f" % share)
    ok = (n_replace >= 20 and fuse_stats["already_later"] > 0 and fuse_stats["changed"] > 0 and fuse_stats["added"] > 0
          and ckf_stats["taken"] > 0 and n_ref > 20 and share <= 0.02)
    return out if ok else None


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import ORBMatcher as RM  # noqa: E402
    for seed in range(7300, 7400):
        out = scene(RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with the wanted events; not written")
    np.savez_compressed(HERE / "scw_many.npz", **out)
    print("seed", seed, (HERE / "scw_many.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
