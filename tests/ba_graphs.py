"""Graph shapes shared by the reduced-system and solve tests, and the dense float64 Schur complement of the oracle's H.

Every builder takes the class (svi_mapper_amd.BundleAdjuster or oracle.OracleBA) and its keyword arguments, so the product
and the oracle see the same graph."""
import numpy as np

from svi_mapper_amd import synth

ID = synth.POSE_ID_SHIFT


def make(cls, prob, **kw):
    cam = prob["cam"]
    ba = cls(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline_m"], **kw)
    synth.build_ba_graph(ba, prob)
    return ba


def _z(prob, kf, lm):
    Rt, tt = prob["R_true"], prob["t_true"]
    return np.einsum("nji,nj->ni", Rt[kf], prob["lm_true"][lm] - tt[kf])


def loop_closure(cls, prob, n_extra=60, seed=2, **kw):
    """landmarks first seen early re-observed from the last ten key frames (test_loop_closure_tracks_break_the_band): fill"""
    r = np.random.default_rng(seed)
    last_seen = np.full(prob["n_lm"], -1)
    np.maximum.at(last_seen, prob["obs_lm"], prob["obs_kf"])
    early = np.nonzero((last_seen >= 0) & (last_seen < prob["n_kf"] - 30))[0]
    extra_lm = r.choice(early, n_extra, replace=False)
    extra_kf = (prob["n_kf"] - 1 - r.integers(0, 10, n_extra)).astype(np.int64)
    ba = make(cls, prob, **kw)
    info = np.tile(np.array([10.0, 0, 0, 10.0, 0, 10.0]), (n_extra, 1))
    ba.add_edges_bulk(np.zeros(n_extra, np.int32), ID + extra_kf, extra_lm, _z(prob, extra_kf, extra_lm), info, np.ones(n_extra, np.int32))
    return ba


def hub_landmark(cls, prob, **kw):
    """one extra landmark observed by every key frame: every pair of poses couples, S is dense"""
    ba = make(cls, prob, **kw)
    n = prob["n_kf"]
    far = prob["t_true"].mean(0) + np.array([0.0, -30.0, 0.0])     # above the whole trajectory
    lm = prob["n_lm"]
    ba.add_landmark(lm, far + 0.3)
    kf = np.arange(n, dtype=np.int64)
    Rt, tt = prob["R_true"], prob["t_true"]
    z = np.einsum("nji,nj->ni", Rt, far[None] - tt)
    info = np.tile(np.array([1.0, 0, 0, 1.0, 0, 1.0]), (n, 1))
    ba.add_edges_bulk(np.zeros(n, np.int32), ID + kf, np.full(n, lm), z, info, np.ones(n, np.int32))
    return ba


def chain(ba, prob, pose_base=ID, lm_base=0, fixed=()):
    """build_ba_graph with the ids shifted and the key frames in `fixed` added as fixed poses (no odometry edge to them)"""
    n_kf = prob["n_kf"]
    ba.add_pose(pose_base, synth.pose12(prob["R_init"][0], prob["t_init"][0]), fixed=True)
    ba.add_landmarks(lm_base + np.arange(prob["n_lm"], dtype=np.int64), prob["lm_init"])
    starts = np.searchsorted(prob["obs_kf"], np.arange(n_kf + 1))
    for k in range(n_kf):
        T = synth.pose12(prob["R_init"][k], prob["t_init"][k])
        if k in fixed:
            ba.add_pose(pose_base + k, T, fixed=True)
        elif k > 0:
            ba.add_keyframe(pose_base + k, pose_base + k - 1, T)
        a, b = starts[k], starts[k + 1]
        if b > a:
            ba.add_measurements(pose_base + k, lm_base + prob["obs_lm"][a:b].astype(np.int64), prob["uvL"][a:b], prob["uvR"][a:b],
                                prob["xyz"][a:b])
    return ba


def new(cls, prob, **kw):
    cam = prob["cam"]
    return cls(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline_m"], **kw)


def interleaved_fixed(cls, prob, every=7, **kw):
    """every `every`-th key frame fixed: free and fixed poses interleave along the trajectory"""
    return chain(new(cls, prob, **kw), prob, fixed=set(range(every, prob["n_kf"], every)))


def two_trajectories(cls, prob_a, prob_b, **kw):
    """two disconnected trajectories in one graph, each with its own fixed first pose: independent chains per level"""
    ba = chain(new(cls, prob_a, **kw), prob_a)
    return chain(ba, prob_b, pose_base=ID + 100000, lm_base=10 ** 7)


def tiny(cls, n_free, n_lm, seed, **kw):
    """pose 1000000 fixed at the origin, n_free poses along +z, every landmark seen by every pose (test_ba_gpu._tiny_graph)"""
    r = np.random.default_rng(seed)
    cam = synth.kitti_camera()
    ba = cls(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline_m"], **kw)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.0])
    ba.add_pose(ID, ident, True)
    for k in range(n_free):
        T = ident.copy()
        T[9:] = [0.02 * (k + 1), 0.0, 0.8 * (k + 1)]
        ba.add_pose(ID + 1 + k, T + np.concatenate([np.zeros(9), r.normal(0, 0.02, 3)]), False)
    pts = np.stack([r.uniform(-3, 3, n_lm), r.uniform(-1, 1, n_lm), 0.8 * n_free + r.uniform(6, 20, n_lm)], 1)
    for l in range(n_lm):
        ba.add_landmark(l, pts[l] + r.normal(0, 0.05, 3))
        for k in range(n_free + 1):
            z = pts[l] - np.array([0.02 * k, 0.0, 0.8 * k]) + r.normal(0, 0.01, 3)
            ba.add_edges_bulk([0], [ID + k], [l], z[None], (1000.0 / z[2] * np.array([1, 0, 0, 1, 0, 1.0]))[None], [1])
    return ba


def oracle_schur(o, lam):
    """float64 reduced camera system of the oracle's dense H at damping lam (on every diagonal entry, landmarks included):
    S = Hpp - Hpl (Hll)^-1 Hlp, g = bp - Hpl Hll^-1 bl, poses in natural (insertion) order.  Hll is inverted block by block
    when it is block diagonal (no landmark-landmark edge), as a whole otherwise."""
    H, b, pc, lc = o.dense_system()
    n = len(b)
    H[np.diag_indices(n)] += lam
    nl = 3 * int((lc >= 0).sum())
    Hll, Hpl, Hpp = H[:nl, :nl], H[nl:, :nl], H[nl:, nl:]
    L = nl // 3
    blocks = Hll.reshape(L, 3, L, 3)[np.arange(L), :, np.arange(L), :]           # (L, 3, 3)
    if np.count_nonzero(Hll) == np.count_nonzero(blocks):                          # nothing off the 3 x 3 blocks
        X = np.linalg.solve(blocks, Hpl.T.reshape(L, 3, -1))                       # Hll^-1 Hlp, block by block
        y = np.linalg.solve(blocks, b[:nl].reshape(L, 3, 1))
        X, y = X.reshape(nl, -1), y.reshape(nl)
    else:
        X = np.linalg.solve(Hll, Hpl.T)
        y = np.linalg.solve(Hll, b[:nl])
    return Hpp - Hpl @ X, b[nl:] - Hpl @ y
