"""The Newton-step precision helpers (tests/kkt_ref.py) on the CPU: the float64 restatements of the
null-space and Schur-complement solves against the mpmath truth, on the graded systems the GPU tests
(test_gpu_kkt_precision.py) use — and that the bounds those tests set can fail: on the span-8 systems
a null-space solve WITHOUT its refinement step is far outside 8 x the refined solve's error, so a
kernel whose refinement is broken (a wrong sign, a dropped delta_w dw term) cannot pass them."""
import numpy as np

import kkt_ref as R

SPAN8 = dict(B=8, nw=47, m=30, seed=11, span=8)  # test_gpu_kkt_precision.py's (47, 30) B = 8 span-8 case
N_TRUTH = 6


def test_truth_solves_exactly_and_takes_longdouble_data():
    rng = np.random.default_rng(0)
    K = rng.normal(size=(9, 9))
    x = rng.normal(size=9)
    # a right-hand side whose exact solution is not representable: truth rounds the exact one
    xt = R.truth(K, K @ x)
    assert R.ferr(xt, x) < 1e-12  # (K @ x is rounded: x solves the system only to cond(K) eps)
    np.testing.assert_allclose(K @ xt, K @ x, rtol=0, atol=1e-13 * np.abs(K @ x).max())
    # longdouble data are taken exactly
    Kl = K.astype(np.longdouble) + np.longdouble(2.0) ** -60
    assert np.array_equal(R.truth(Kl, (K @ x).astype(np.longdouble)), R.truth(Kl, K @ x))


def test_refined_nullspace_restatement_is_at_rounding_level_and_unrefined_is_not():
    M, A, r1, r2 = R.ipm_like_systems(**SPAN8)
    nw = SPAN8["nw"]
    differ = 0
    for b in range(N_TRUTH):
        xt = R.truth(R.kkt_matrix(M[b], A[b]), np.concatenate([r1[b], r2[b]]))
        dw1, dy1 = R.nullspace_solve(M[b], A[b], r1[b], r2[b], refine=True)
        dw0, dy0 = R.nullspace_solve(M[b], A[b], r1[b], r2[b], refine=False)
        e1 = (R.ferr(dw1, xt[:nw]), R.ferr(dy1, xt[nw:]))
        e0 = (R.ferr(dw0, xt[:nw]), R.ferr(dy0, xt[nw:]))
        print(f"system {b}: refined dw {e1[0]:.2e} dy {e1[1]:.2e}, unrefined dw {e0[0]:.2e} dy {e0[1]:.2e}")
        assert max(e1) <= 64 * R.EPS
        differ += e0[0] > 8 * e1[0] and e0[1] > 8 * e1[1]
    assert differ >= 1


def test_schur_restatement_against_truth_and_the_dense_solve():
    """The quasi-definite system's Schur-complement solve against the truth: within 64 eps cond(K_S) of
    it (the forward bound of a Cholesky solve, K_S = W + A^T D^-1 A) on ungraded and graded systems.  On
    the span-6 systems the METHOD loses digits that a dense solve of the full system keeps (its error
    exceeds 8 x LAPACK's on at least one system), so the GPU bound is set against this restatement, not
    against eps — and a solve with D in place of D^-1 is outside that bound on every one of them."""
    nw, m = 47, 30
    for span in (0, 6):
        W, A, Dinv, r1, r2 = R.qd_like_systems(3, nw, m, seed=5, span=span)
        worse = 0
        for b in range(3):
            rhs = np.concatenate([r1[b], r2[b]])
            xt = R.truth(R.kkt_matrix(W[b], A[b], Dinv=Dinv[b]), rhs)
            K = R.kkt_matrix(W[b], A[b], D=1.0 / Dinv[b])
            dw, dy = R.qd_schur_solve(W[b], A[b], Dinv[b], r1[b], r2[b])
            xn = np.linalg.solve(K, rhs)
            es = (R.ferr(dw, xt[:nw]), R.ferr(dy, xt[nw:]))
            en = (R.ferr(xn[:nw], xt[:nw]), R.ferr(xn[nw:], xt[nw:]))
            cond = np.linalg.cond(W[b] + A[b].T @ (Dinv[b][:, None] * A[b]))
            print(f"span {span} system {b}: Schur dw {es[0]:.2e} dy {es[1]:.2e}, dense dw {en[0]:.2e} dy {en[1]:.2e}, "
                  f"cond(K_S) {cond:.1e}")
            assert es[0] <= 64 * R.EPS * cond
            worse += max(es) > 8 * max(en)
            if span:
                bw, by = R.qd_schur_solve(W[b], A[b], 1.0 / Dinv[b], r1[b], r2[b])  # the wrong D
                assert R.ferr(bw, xt[:nw]) > 8 * max(es[0], 4 * R.EPS)
                assert R.ferr(by, xt[nw:]) > 8 * max(es[1], 4 * R.EPS)
        if span:
            assert worse >= 1


def test_delta_w_schedule_and_inertia():
    assert R.delta_w_schedule(0.0, 4) == [1e-4, 1e-2, 1.0, 100.0]
    assert R.delta_w_schedule(0.6, 3) == [0.6 / 3, 0.6 / 3 * 8, 0.6 / 3 * 8 * 8]
    np.testing.assert_allclose(R.delta_w_schedule(0.6, 2), [0.2, 1.6], rtol=4 * R.EPS)
    assert R.delta_w_schedule(1e-21, 1) == [1e-20]
    H = np.diag([2.0, 1.0, -0.3])
    assert R.inertia_delta_w(H, 0.0) == 1.0
    assert R.inertia_delta_w(H, 0.6) == 0.6 / 3 * 8
    assert R.inertia_delta_w(np.eye(3), 0.6) == 0.0
    # a pivot at the rounding level counts as zero
    assert R.inertia_delta_w(np.diag([1.0, 1e-20]), 0.0, pivot_min=R.EPS) == 1e-4


def test_prescribed_reduced_spectrum_and_rank_deficiency():
    nw, m = 39, 14
    lam = np.concatenate([[-0.3], np.linspace(0.5, 2.0, nw - m - 1)])
    M, A, _, r2 = R.ipm_like_systems(3, nw, m, seed=2, span=0, reduced_spectrum=lam, rank_def=[False, True, False])
    for b in range(3):
        np.testing.assert_array_equal(M[b], M[b].T)
        if b == 1:
            assert np.linalg.matrix_rank(A[b]) == m - 1 and r2[b, -1] == r2[b, 0] + r2[b, 1]
            continue
        Z = np.linalg.qr(A[b].T, mode="complete")[0][:, m:]
        np.testing.assert_allclose(np.linalg.eigvalsh(Z.T @ M[b] @ Z), np.sort(lam), rtol=0, atol=1e-13)
    W = R.qd_like_systems(2, 20, 0, seed=3, span=0, spectrum=np.concatenate([[-0.3], np.linspace(0.5, 2.0, 19)]))[0]
    np.testing.assert_allclose(np.linalg.eigvalsh(W[1]).min(), -0.3, rtol=0, atol=1e-13)
