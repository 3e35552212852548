"""Tracking.search_local_points on the first frames of the C3 golden (tests/seq_harness.py,
tests/golden/sequence_kitti_synth.npz), shared by tests/test_local_search_cpu.py and tests/test_gpu_local_search.py.

The golden records, per frame, the local map points the reference's Frame.is_in_frustum left in view with their
projections, levels and viewing cosines, and what search_by_projection_f_p then assigned; it does not record the map
points' normals and distance bounds.  SeqMP restates MapPoint.__init__'s kframe_bool=False branch (MapPoint.py:31-55)
from the recorded position, the frame and keypoint the point was made from, and that frame's tracked pose; the
recorded projection bits pin the restatement.  The local map is rebuilt as the generator built it: the map points of
the last LOCAL_WINDOW frames, newest frame first, each once.
"""
from __future__ import annotations

import numpy as np

import seq_harness as H

FRAMES = (1, 2, 3)


class SeqMP(H.ReplayMP):
    """ReplayMP with what Frame.is_in_frustum and Tracking.search_local_points read besides (MapPoint.py)."""

    def __init__(self, mp_id, pos, desc, obs, ref_frame, kp):
        super().__init__(mp_id, pos, desc, obs)
        Ow = ref_frame.mOw.copy()
        self._normal = self._pos - Ow
        self._normal = self._normal / np.linalg.norm(self._normal)
        PC = self._pos - Ow
        dist = np.linalg.norm(PC)
        level = ref_frame.mvKeysUn[kp].octave
        self.mfMaxDistance = dist * ref_frame.mvScaleFactors[level]
        self.mfMinDistance = self.mfMaxDistance / ref_frame.mvScaleFactors[ref_frame.mnScaleLevels - 1]
        self.mnLastFrameSeen = 0
        self.mnVisible = 1
        self.mnId = mp_id

    def get_normal(self):
        return self._normal.copy()

    def get_min_distance_invariance(self):
        return 0.8 * self.mfMinDistance

    def get_max_distance_invariance(self):
        return 1.2 * self.mfMaxDistance

    def predict_scale(self, current_dist, pKF):
        ratio = self.mfMaxDistance / current_dist
        n = int(np.ceil(np.log(ratio) / pKF.mfLogScaleFactor))
        return max(0, min(n, pKF.mnScaleLevels - 1))

    def increase_visible(self, n=1):
        self.mnVisible += n


def scenes(g, sequence, extractors, frame_cls):
    """Yields (k, frame, local map) for k in FRAMES with the frame as Tracking has it before search_local_points:
    the predicted pose, the slots search_by_projection_f_f left (the golden's), those map points marked seen.  After
    the caller is done with a scene the frame gets its tracked pose and the golden's final slots."""
    import json
    meta = json.loads(str(g["meta"]))
    s = H.settings(meta["cam"])
    fa = H.frame_args(s, meta["width"], meta["height"])
    exL, exR = extractors
    reg, frames = {}, []

    def mp(i):
        m = reg.get(i)
        if m is None:
            f, kp = int(g["mp_frame"][i]), int(g["mp_kp"][i])
            m = reg[i] = SeqMP(i, g["mp_pos"][i].reshape(3, 1).astype(np.float32), frames[f].mDescriptors[kp],
                               int(g["mp_obs"][i]), frames[f], kp)
        return m

    for k in range(max(FRAMES) + 1):
        p = f"f{k}_"
        L, R = sequence.frame(k)
        cur = frame_cls(L, R, float(k), exL, exR, None, s["mK"], s["mDistCoef"], s["mbf"], s["mThDepth"], fa)
        cur.mnId = k
        if k in FRAMES:
            cur.set_pose(g[p + "Tpred"])
            cur.mvpMapPoints = [None if i < 0 else mp(int(i)) for i in g[p + "ff_assign"]]
            for q in cur.mvpMapPoints:
                if q is not None:
                    q.mnLastFrameSeen = cur.mnId
                    q.mbTrackInView = False
            local, seen = [], set()
            for fr in frames[-H.LOCAL_WINDOW:][::-1]:
                for q in fr.mvpMapPoints:
                    if q is not None and id(q) not in seen and not q.is_bad():
                        seen.add(id(q))
                        local.append(q)
            yield k, cur, local
        cur.set_pose(g[p + "Tgt"])
        frames.append(cur)
        cur.mvpMapPoints = [None if i < 0 else mp(int(i)) for i in g[p + "slots"]]
        if k >= 2:
            frames[k - 2].mvImagePyramidLeft = frames[k - 2].mvImagePyramidRight = None


def in_view(local):
    return [q for q in local if q.mbTrackInView]


def frustum_differs(g, k, local, kinds):
    """What is_in_frustum left on the local map against the golden's record of frame k: the in-view set in order, and
    every value bit for bit with the recorded type.  Returns the names that differ."""
    p = f"f{k}_"
    seen = in_view(local)
    bad = []
    if [q.mp_id for q in seen] != g[p + "local_ids"].tolist():
        return ["local_ids"]
    if [int(q.mnTrackScaleLevel) for q in seen] != g[p + "local_level"].tolist():
        bad.append("local_level")
    for name, attr, kd in (("local_px", "mTrackProjX", kinds["x"]), ("local_py", "mTrackProjY", kinds["y"]),
                           ("local_pxr", "mTrackProjXR", kinds["xr"]), ("local_vcos", "mTrackViewCos", kinds["vcos"])):
        for q, x in zip(seen, g[p + name]):
            a, want = getattr(q, attr), H.proj_value(x, kd)
            if not (type(a) is type(want) and a.dtype == want.dtype and a.shape == want.shape
                    and a.tobytes() == want.tobytes()):
                bad.append(name)
                break
    return bad


def search_differs(g, k, cur, res):
    """(nToMatch, n) and the frame's slots against the golden's record of frame k."""
    p = f"f{k}_"
    bad = []
    if res[0] != len(g[p + "local_ids"]):
        bad.append("nToMatch")
    if res[1] != int(g[p + "fp_n"]):
        bad.append("fp_n")
    if not np.array_equal(H.encode_slots(cur), g[p + "fp_assign"]):
        bad.append("fp_assign")
    return bad
