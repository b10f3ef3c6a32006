"""The reduced-camera-system solve (tile Cholesky + backward substitution, ba_chol.hip) against a float64 reference.

svi_ba_debug_solve runs the production factorisation and backward substitution on the reduced system of the handle's current
estimate; reduced_system(lam) returns that same system densely.  The reference is scipy's LAPACK Cholesky in float64 plus one
step of iterative refinement with the residual in extended precision.  Checked per case:

  * the factorisation succeeds (status 0);
  * the normwise backward error |S dx - g| / (|S| |dx| + |g|) (infinity norms, residual in long double) is within C_BWD * u,
    and the componentwise one (row by row) within C_CW * u - bounds that do not depend on the conditioning of S;
  * the forward error against the reference is within C_FWD * u * kappa(S), kappa estimated from the reference factor;
  * a second call returns the same dx bit for bit (the design keeps the chain bit-identical run to run: the one-launch
    backward substitution waits for its inputs but sums them in a fixed order).

The graphs cover the four solve kernels (SVI_SOLVE_K_*), padding of the last tile column, band and fill, fixed poses inside
the trajectory, several chains per level, a dense S, pose-only edges, the production shapes, the boundary of positive
definiteness and state left behind by earlier solves."""
import numpy as np
import pytest
import scipy.linalg as sla
from scipy.sparse.linalg import LinearOperator, onenormest

import ba_graphs as bg
from svi_mapper_amd import synth
from svi_mapper_amd.optimizer import BundleAdjuster as _BA

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# Normwise backward error bound.  Measured on an MI355X over every case of this module: at most 0.71 u (most cases 0.1-0.5 u).
# The worst-case bound of a Cholesky grows with n; what a blocked factorisation with fused multiply-adds reaches in practice is
# a few u, so C_BWD = 8 leaves an order of magnitude of headroom and still fails a tile whose entries are off by 1e-10
# relative: that moves the error by about 1e-10 |S_ij| |x_j| / (|S| |x|), for a diagonal tile ~1e-12 = 10^4 u.
C_BWD = 8
# Componentwise (row by row, Oettli-Prager) backward error max_i |S dx - g|_i / (|S| |dx| + |g|)_i: a wrong entry in one
# row is measured against that row only, not against the largest row of S, so a single update element off by 2^-30 in one
# tile is seen (the normwise error hardly moves: 0.08 u -> 0.13 u).  A Cholesky's componentwise error is bounded through
# |L| |L'|, not |S|, so it runs higher: measured at most 131 u (64 free poses; the 2100-pose trajectory), 2-30 u elsewhere.
# C_CW = 1024 leaves a factor 8 over that; the element off by 2^-30 gave 5000-29000 u on the near-singular cases.
C_CW = 1024
# Forward error |dx - x| / |x| <= 2 kappa (backward error) to first order, i.e. ~ 2 u kappa with the errors above; measured at
# most 0.004 u kappa (kappa_inf is an upper estimate).  C_FWD = 4 keeps the first-order bound with the backward errors seen.
C_FWD = 4

_ALL, _INL, _LEVEL, _TRSM = _BA.SOLVE_K_ALL, _BA.SOLVE_K_INL, _BA.SOLVE_K_LEVEL, _BA.SOLVE_K_TRSM
_SEEN = {"kernels": 0, "bwd": 0.0, "cw": 0.0}   # over the module: union of the solve kernels that ran, largest backward errors


# -- float64 reference ----------------------------------------------------------------------------------------------------
def _norm_inf(S, rows=1024):
    return max(float(np.abs(S[i:i + rows]).sum(1).max()) for i in range(0, len(S), rows))


def _residual(S, x, g, rows=1024):
    """g - S x in long double, a block of rows at a time (S may be a gigabyte)"""
    xl = x.astype(np.longdouble)
    r = np.empty(len(g), np.longdouble)
    for i in range(0, len(g), rows):
        r[i:i + rows] = g[i:i + rows].astype(np.longdouble) - S[i:i + rows].astype(np.longdouble) @ xl
    return r


def _bandwidth(S, rows=1024):
    bw = 0
    for i in range(0, len(S), rows):
        r, c = np.nonzero(S[i:i + rows])
        if len(r):
            bw = max(bw, int((r + i - c).max()))
    return bw


def _reference(S, g):
    """(x, kappa_inf): x from LAPACK's Cholesky in float64 + one refinement step with a long double residual; kappa_inf(S) =
    |S|_inf |S^-1|_inf, the second factor estimated (Hager / Higham) through the factor.  A banded S (long trajectories) is
    factorised in band storage."""
    n = len(g)
    bw = _bandwidth(S)
    if n > 4096 and bw < n // 8:
        ab = np.zeros((bw + 1, n))
        for d in range(bw + 1):
            ab[d, :n - d] = np.diagonal(S, -d)
        cb = sla.cholesky_banded(ab, lower=True)

        def solve(b):
            return sla.cho_solve_banded((cb, True), b)
    else:
        cf = sla.cho_factor(S, lower=True)

        def solve(b):
            return sla.cho_solve(cf, b)
    x = solve(g)
    x = x + solve(_residual(S, x, g).astype(np.float64))
    inv = LinearOperator((n, n), matvec=solve, rmatvec=solve, dtype=np.float64)
    kappa = _norm_inf(S) * onenormest(inv)
    return x, kappa


def _backward_errors(S, dx, g, rows=1024):
    """(normwise, componentwise) backward error of dx, residual in long double"""
    r = np.abs(_residual(S, dx, g)).astype(np.float64)
    ax = np.abs(dx)
    den = np.empty(len(g))
    for i in range(0, len(g), rows):
        den[i:i + rows] = np.abs(S[i:i + rows]) @ ax + np.abs(g[i:i + rows])
    return float(r.max() / (_norm_inf(S) * ax.max() + np.abs(g).max())), float((r / den).max())


def _solve(ba, lam, repeat=True):
    """debug_solve(lam) twice (bitwise the same), returns (dx, kernels) after status 0"""
    dx, st, k = ba.debug_solve(lam)
    assert st == 0, "factorisation failed: status %d" % st
    assert np.isfinite(dx).all()
    if repeat:
        dx2, st2, k2 = ba.debug_solve(lam)
        assert st2 == 0 and k2 == k
        assert np.array_equal(dx, dx2), "two solves of the same system differ"
    _SEEN["kernels"] |= k
    return dx, k


def _check(ba, lam, repeat=True):
    """the production solve of the handle's reduced system against the reference; returns the kernel bits"""
    S, g = ba.reduced_system(lam)
    dx, k = _solve(ba, lam, repeat)
    _check_against(S, g, dx)
    return k


def _check_against(S, g, dx):
    assert dx.shape == g.shape
    eta, omega = _backward_errors(S, dx, g)
    _SEEN["bwd"] = max(_SEEN["bwd"], eta)
    _SEEN["cw"] = max(_SEEN["cw"], omega)
    x, kappa = _reference(S, g)
    fwd = np.abs(dx - x).max() / np.abs(x).max()
    print("n %d: backward error %.2f u, componentwise %.2f u, forward error %.2e, kappa %.2e" % (len(g), eta / U, omega / U, fwd, kappa))
    assert eta <= C_BWD * U, "backward error %.3e = %.1f u" % (eta, eta / U)
    assert omega <= C_CW * U, "componentwise backward error %.3e = %.1f u" % (omega, omega / U)
    assert fwd <= C_FWD * U * max(kappa, 1.0), "forward error %.3e, kappa %.3e" % (fwd, kappa)


def _lam0(S):
    """a damping of the size the LM starts with (1e-5 x the largest diagonal entry)"""
    return 1e-5 * float(np.diag(S).max())


def _init(ba):
    ba.initialize()
    return ba


# -- padding of the last tile column: 6 Pf mod 48 (mod 96) in {6, 42, 0} ------------------------------------------------------
# Pf = 1: 6 / 6, 7: 42 / 42, 8: 0 / 48, 16: 0 / 0, 49: 6 / 6, 55: 42 / 42, 64: 0 / 0
@pytest.mark.parametrize("tile", [48, 96])
@pytest.mark.parametrize("pf", [1, 7, 8, 16, 49, 55, 64])
def test_padding_of_the_last_tile_column(svi, tile, pf):
    orders = (0, 1) if pf >= tile else (0,)          # (nested dissection needs six tile columns or more)
    for order in orders:
        if pf == 1:
            ba = _init(bg.tiny(svi.BundleAdjuster, 1, 12, seed=3, chol_tile=tile, chol_order=order))
        else:
            prob = synth.make_ba_problem(pf + 1, 40 * pf, 300 * pf, seed=100 + pf)
            ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile, chol_order=order))
        assert ba.stats().n_poses_free == pf
        _check(ba, 1e-3)
        ba.close()


# -- band and fill ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [48, 96])
@pytest.mark.parametrize("order", [0, 1])
def test_straight_trajectory(svi, tile, order):
    n = 80
    prob = synth.make_ba_problem(n, 3000, 20000, seed=31, traj=synth.trajectory(n, straight=10 ** 6))
    ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile, chol_order=order))
    S, _ = ba.reduced_system(0.0)
    _check(ba, _lam0(S))


@pytest.mark.parametrize("tile", [48, 96])
@pytest.mark.parametrize("order", [0, 1])
def test_loop_closure_fill(svi, tile, order):
    prob = synth.make_ba_problem(90, 3000, 24000, seed=13)
    ba = _init(bg.loop_closure(svi.BundleAdjuster, prob, chol_tile=tile, chol_order=order))
    S, _ = ba.reduced_system(0.0)
    _check(ba, _lam0(S))


# -- structure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [48, 96])
@pytest.mark.parametrize("order", [0, 1])
def test_fixed_poses_inside_the_trajectory(svi, tile, order):
    prob = synth.make_ba_problem(100, 3000, 22000, seed=41)
    ba = _init(bg.interleaved_fixed(svi.BundleAdjuster, prob, every=7, chol_tile=tile, chol_order=order))
    assert ba.stats().n_poses_free == 99 - 14
    S, _ = ba.reduced_system(0.0)
    _check(ba, _lam0(S))


@pytest.mark.parametrize("tile", [48, 96])
@pytest.mark.parametrize("order", [0, 1])
def test_two_disconnected_trajectories(svi, tile, order):
    pa = synth.make_ba_problem(60, 2000, 14000, seed=51)
    pb = synth.make_ba_problem(45, 1500, 10000, seed=52)
    ba = _init(bg.two_trajectories(svi.BundleAdjuster, pa, pb, chol_tile=tile, chol_order=order))
    S, _ = ba.reduced_system(0.0)
    na = 6 * 59
    assert not S[:na, na:].any()                       # two independent blocks
    _check(ba, _lam0(S))
    if order == 0:
        st = ba.stats()
        assert st.chol_steps < -(-st.chol_n // tile)  # several chains per level


@pytest.mark.parametrize("tile", [48, 96])
def test_dense_system_from_a_landmark_seen_by_every_pose(svi, tile):
    """S dense: at tile 48 the early columns hold more sub-diagonal tiles than the one-launch records do, so the per-level
    kernels run (the inline one for the levels whose columns are short enough)"""
    prob = synth.make_ba_problem(120, 2500, 18000, seed=61)
    ba = _init(bg.hub_landmark(svi.BundleAdjuster, prob, chol_tile=tile))
    S, _ = ba.reduced_system(0.0)
    assert (S != 0).mean() > 0.99
    k = _check(ba, _lam0(S))
    if tile == 48:
        assert k & _LEVEL and k & _INL and not k & _ALL, k
    else:
        assert k & _LEVEL and k & _TRSM, k


@pytest.mark.parametrize("tile", [48, 96])
def test_vi_graph(svi, tile):
    """real gravity measurements and the odometry edges of the key frames: pose-only terms in S"""
    prob = synth.make_vi_problem(40, 3000, 20000)
    ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile))
    st = ba.stats()
    assert st.n_edges_se3 > 0 and st.n_edges_accel > 0
    S, _ = ba.reduced_system(0.0)
    _check(ba, _lam0(S))


# -- production shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["c3", "c4"])
def test_production_shapes(svi, cfg):
    """configs 3 and 4 at the lambda the LM uses next (after its first iteration): the one-launch backward substitution"""
    prob = synth.make_c3() if cfg == "c3" else synth.make_c4()
    ba = _init(bg.make(svi.BundleAdjuster, prob))
    assert ba.optimize(1) == 1
    k = _check(ba, ba.lm_lambda)
    assert k == _ALL, k


def test_long_trajectory_per_level_kernels(svi):
    """2100 key frames (test_long_trajectory_takes_the_per_level_backward_substitution): more tile columns than the one-launch
    backward substitution may hold resident.  One solve; S is 1.3 GB dense, the reference works on its band."""
    prob = synth.make_ba_problem(2100, 6000, 30000, seed=0x2100)
    ba = _init(bg.make(svi.BundleAdjuster, prob))
    k = _check(ba, 1e-2, repeat=False)
    assert not k & _ALL and k & (_LEVEL | _INL), k


# -- conditioning ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [48, 96])
def test_undamped_system_with_a_fixed_gauge(svi, tile):
    """lambda = 0 (every landmark observed: synth's graphs can hold landmarks whose edges were all refused, and their
    undamped blocks are singular)"""
    ba = _init(bg.tiny(svi.BundleAdjuster, 30, 60, seed=7, chol_tile=tile))
    _check(ba, 0.0)


def test_tiny_damping(svi):
    prob = synth.make_ba_problem(40, 2000, 14000, seed=72)
    ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=96))
    S, _ = ba.reduced_system(0.0)
    _check(ba, 1e-9 * float(np.diag(S).max()))


@pytest.mark.parametrize("tile", [48, 96])
def test_landmark_depths_from_1_to_1000_m(svi, tile):
    prob = synth.make_ba_problem(50, 4000, 20000, seed=73, depth_range=(1.0, 1000.0), max_depth=1001.0)
    ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile))
    S, _ = ba.reduced_system(0.0)
    _check(ba, 1e-9 * float(np.diag(S).max()))


# -- the boundary of positive definiteness ------------------------------------------------------------------------------------------
def _critical_lambda(ba):
    """lam* < 0 at which the reduced system S(lam) = (Hpp + lam) - Hpl (Hll + lam)^-1 Hlp of the handle becomes singular
    (bisection on the eigenvalues of the tap's S).  d S / d lam >= I while the landmark blocks stay positive definite, so
    lambda_min(S(lam)) rises with lam at slope >= 1: S(lam) is positive definite above lam* and indefinite below."""
    def lmin(lam):
        S, _ = ba.reduced_system(lam)
        return np.linalg.eigvalsh(S)[0]

    lo = -lmin(0.0)                       # S(lo) <= S(0) + lo I: not positive definite
    hi = 0.0
    assert lmin(lo) <= 0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if lmin(mid) > 0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def _landmark_block_eig(oracle, builder):
    """smallest eigenvalue of the undamped landmark blocks (oracle's H): it must stay clear of |lam*|, or a landmark block
    and not the reduced system would be what fails"""
    o = builder(oracle.OracleBA)
    o.initialize()
    H, _, _, lc = o.dense_system()
    nl = 3 * int((lc >= 0).sum())
    L = nl // 3
    blocks = H[:nl, :nl].reshape(L, 3, L, 3)[np.arange(L), :, np.arange(L), :]
    return float(np.linalg.eigvalsh(blocks).min())


def _boundary_graph(cls, **kw):
    return bg.tiny(cls, 20, 30, seed=5, **kw)


@pytest.mark.parametrize("tile", [48, 96])
def test_negative_damping_near_the_boundary(svi, oracle, tile):
    ba = _init(_boundary_graph(svi.BundleAdjuster, chol_tile=tile))
    lam_c = _critical_lambda(ba)
    assert lam_c < 0 and _landmark_block_eig(oracle, _boundary_graph) > 10 * abs(lam_c)
    _check(ba, 0.999 * lam_c)                                    # just inside: positive definite, same accuracy
    _, st, _ = ba.debug_solve(1.001 * lam_c)                     # just outside: a failed pivot (dx is not read)
    assert st > 0, st
    _check(ba, 1e-3)                                             # a failed solve leaves nothing behind


# -- state left behind -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [48, 96])
def test_second_lambda_on_the_same_handle(svi, tile):
    """lambda_1 then lambda_2: the second solve owes nothing to the first (pending markers, forward vector) - correct, and
    bit for bit what a fresh handle computes"""
    prob = synth.make_ba_problem(60, 2500, 16000, seed=81)
    ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile))
    S, _ = ba.reduced_system(0.0)
    l1, l2 = _lam0(S), 37.0 * _lam0(S)
    _check(ba, l1)
    _check(ba, l2)
    fresh = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile))
    dx_f, _ = _solve(fresh, l2, repeat=False)
    dx_b, _ = _solve(ba, l2, repeat=False)
    assert np.array_equal(dx_f, dx_b)


@pytest.mark.parametrize("tile", [48, 96])
def test_solve_after_optimize(svi, tile):
    """the tap behind optimize(3) (a speculated linearisation may sit in the buffers): the system of the current estimate,
    and the handle's estimates are untouched by the tap"""
    prob = synth.make_ba_problem(60, 2500, 16000, seed=82)
    ba = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile))
    assert ba.optimize(3) == 3
    T0 = ba.get_poses()[1].copy()
    _check(ba, ba.lm_lambda)
    assert np.array_equal(ba.get_poses()[1], T0)
    ref = _init(bg.make(svi.BundleAdjuster, prob, chol_tile=tile))
    assert ref.optimize(3) == 3
    assert ba.optimize(2) == ref.optimize(2)                   # and the LM goes on as if no tap had run
    assert np.array_equal(ba.get_poses()[1], ref.get_poses()[1])


# -- coverage (keep last) ---------------------------------------------------------------------------------------------------------------
def test_every_solve_kernel_is_covered(svi):
    """The union of the solve kernels that ran in this module covers all four.  When the module runs in part, the smallest
    graph known to reach a missing kernel is solved here.  (k_trsm runs at tile 96 only: at tile 48 it is folded into
    k_potrf_inv.  k_back_solve_inl and k_back_solve at tile 48 need a plan without the one-launch records: a column with more
    than 12 sub-diagonal tiles, as the dense system below has, or more columns than there are compute units.)"""
    prob = synth.make_ba_problem(120, 2500, 18000, seed=61)
    reach = {_ALL: dict(chol_tile=48), _TRSM: dict(chol_tile=96), _INL: dict(chol_tile=48), _LEVEL: dict(chol_tile=96)}
    for bit, kw in reach.items():
        if not _SEEN["kernels"] & bit:
            build = bg.hub_landmark if bit == _INL else bg.make
            ba = _init(build(svi.BundleAdjuster, prob, **kw))
            S, _ = ba.reduced_system(0.0)
            _check(ba, _lam0(S), repeat=False)
    assert _SEEN["kernels"] == _ALL | _INL | _LEVEL | _TRSM, _SEEN["kernels"]
    print("largest backward errors of the module: normwise %.2f u, componentwise %.2f u" % (_SEEN["bwd"] / U, _SEEN["cw"] / U))
