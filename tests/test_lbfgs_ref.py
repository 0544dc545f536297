"""tests/lbfgs_ref.py checked on the CPU: the reference the GPU tests of the limited-memory kernels compare
against, and the generators behind their cases."""
import numpy as np
import pytest

import lbfgs_ref as R

LD = R.LD
LDEPS = float(np.finfo(LD).eps)


def test_one_pair_model_in_closed_form():
    """nf = 2, s = (1, 0), y = (2, 1): sigma = s'y / s's = 2, B s = (2, 0), s'B s = 2, so
    B = 2 I - diag(2, 0) + y y' / 2 = [[2, 1], [1, 2.5]]."""
    S, Y = np.array([[1.0, 0.0]]), np.array([[2.0, 1.0]])
    take, guard, sy, ss, yy = R.decision(S, Y)
    assert take[0] and (sy[0], ss[0], yy[0]) == (2, 1, 5) and guard[0] > 1e6
    assert R.sigma_of(sy, ss)[0] == 2
    B = R.dense_model(S, Y, 2.0)
    assert (B == np.array([[2, 1], [1, 2.5]], dtype=LD)).all()
    assert (R.dense_model(S, Y, 2.0, dtype=np.float64) == np.array([[2, 1], [1, 2.5]])).all()
    # the same model in compact form: u = B0 s / sqrt(s'B0 s) = (sqrt 2, 0), w = y / sqrt(s'y)
    U, W = np.array([[np.sqrt(LD(2)), 0]]), Y.astype(LD) / np.sqrt(LD(2))
    assert np.abs(R.expand(2.0, 1, U, W) - B).max() <= 4 * LDEPS


@pytest.mark.parametrize("span", [0, 4, 8])
@pytest.mark.parametrize("nf", [2, 39, 75])
def test_secant_equation_symmetry_and_definiteness_at_every_memory_length(nf, span):
    rng = np.random.default_rng(10 * nf + span)
    S, Y = R.spd_pairs(rng, R.LM_HIST, nf, span)
    assert ((S * Y).sum(1) > 0).all()
    for nc in range(1, R.LM_HIST + 1):
        sigma = float(R.sigma_of(*R.decision(S[nc - 1:nc], Y[nc - 1:nc])[2:4])[0])
        B = R.dense_model(S[:nc], Y[:nc], sigma)
        res = np.abs(B @ S[nc - 1].astype(LD) - Y[nc - 1]).max() / np.abs(Y[nc - 1]).max()
        # (each update cancels B s against itself: the residual carries the model's size over the pair's)
        size = float(np.abs(B).max() * np.abs(S[nc - 1]).max() / np.abs(Y[nc - 1]).max())
        assert res <= 64 * nf * LDEPS * max(1.0, size)
        assert np.abs(B - B.T).max() <= 8 * LDEPS * np.abs(B).max()
        Bs = 0.5 * (B + B.T).astype(np.float64)
        assert np.linalg.eigvalsh(Bs).min() > 0


def test_longdouble_recursion_against_mpmath():
    """The longdouble recursion is the GPU tests' truth: against 40 digits it is 2^11 times closer than the
    float64 recursion on the same pairs (64 against 53 bits; asserted: 2^8), here where float64 has lost
    digits (span 8, nf 5)."""
    import mpmath

    rng = np.random.default_rng(3)
    S, Y = R.spd_pairs(rng, 4, 5, 8)
    Bm = R.dense_model_mp(S, Y, 0.7)

    def err(B):  # a longdouble entry as the sum of two doubles, exactly
        with mpmath.workdps(40):
            hi = B.astype(np.float64)
            lo = (B - hi.astype(LD)).astype(np.float64)
            scale = max(abs(Bm[i, j]) for i in range(5) for j in range(5))
            return float(max(abs(mpmath.mpf(float(hi[i, j])) + mpmath.mpf(float(lo[i, j])) - Bm[i, j])
                             for i in range(5) for j in range(5)) / scale)

    e_ld = err(R.dense_model(S, Y, 0.7))
    e_64 = err(R.dense_model(S, Y, 0.7, dtype=np.float64).astype(LD))
    assert e_64 > 64 * R.EPS, e_64
    assert e_ld * 2 ** 8 < e_64, (e_ld, e_64)


def test_every_state_transition_by_hand():
    t = R.transition
    for cnt in range(R.LM_HIST + 1):
        assert t(cnt, 0, 0, True) == (min(cnt + 1, 6), 0, "take")
        assert t(cnt, 2, 0, True) == (min(cnt + 1, 6), 0, "take")  # a taken pair clears the skip count
        assert t(cnt, 0, 0, False) == (cnt, 1, "skip")
        assert t(cnt, 1, 0, False) == (cnt, 2, "skip")
        assert t(cnt, 2, 0, False) == (0, 0, "reset")  # the third skip in a row
        for skip in range(3):
            for take in (False, True):
                assert t(cnt, skip, 1, take) == (0, 0, "reset")  # failed resets whatever the pair
    S = np.arange(12.0).reshape(6, 2)
    Y = -S
    s, y = np.array([100.0, 101.0]), np.array([200.0, 201.0])
    S1, Y1, c1 = R.memory_after(S, Y, 6, s, y)  # a full memory drops its oldest
    assert c1 == 6 and (S1[:5] == S[1:]).all() and (S1[5] == s).all() and (Y1[:5] == Y[1:]).all() and (Y1[5] == y).all()
    S2, Y2, c2 = R.memory_after(S, Y, 3, s, y)
    assert c2 == 4 and (S2[:3] == S[:3]).all() and (S2[3] == s).all() and (S2[4:] == S[4:]).all() and (Y2[3] == y).all()
    S3, _, c3 = R.memory_after(S, Y, 0, s, y)
    assert c3 == 1 and (S3[0] == s).all() and (S3[1:] == S[1:]).all()
    assert (S == np.arange(12.0).reshape(6, 2)).all()  # the inputs are left alone


def test_sigma_clamps():
    assert R.sigma_of(LD(1e-10), LD(1.0)) == LD(1e-8) and R.sigma_of(LD(1e10), LD(1.0)) == LD(1e8)
    assert R.sigma_of(LD(3.0), LD(2.0)) == LD(1.5)


def test_pair_conventions_by_hand():
    """m = 2, nf = 2: column 0 reads record entry 1 (row 0) and the constant 1 (row 1); column 1 is
    structurally zero in row 0 and reads entry 0, a NaN at the new point, in row 1."""
    c = dict(n=3, m=2, nf=2, nw=3, nnz_rec=3, amap=np.array([[1, -1], [-2, 0]], dtype=np.int32),
             free_idx=np.array([0, 2], dtype=np.int32), w_old=np.array([[1.0, 2.0, 3.0]]),
             w_new=np.array([[1.5, 1.0, 9.0]]), y=np.array([[1.0, 2.0]]), dy=np.array([[2.0, -2.0]]),
             alpha=np.array([0.5]), gw_old=np.array([[0.25, 0.5, 77.0]]), J_old=np.array([[3.0, 5.0, 99.0]]),
             J_new=np.array([[np.nan, 7.0, 99.0]]), grad_new=np.array([[10.0, 55.0, 20.0]]))
    s, yk, yabs = R.pair(c)
    # yn = (2, 1); new: col 0 = 7 * 2 + 1 * 1 = 15, col 1 = 0; old: col 0 = 5 * 2 + 1 = 11, col 1 = 3 * 1 = 3
    assert (s == [[0.5, -1.0]]).all()
    assert (yk == [[(10 + 15) - (0.25 + 11), (20 + 0) - (0.5 + 3)]]).all()
    # |yn| is bounded by |y| + |alpha dy| = (2, 3)
    assert (yabs == [[10 + 0.25 + (7 + 5) * 2 + 2 * 3, 20 + 0.5 + 3 * 3]]).all()
    c["grad_new"] = None
    assert (R.pair(c)[1] == [[15 - 11.25, 0 - 3.5]]).all()


@pytest.mark.parametrize("m,nf", [(0, 1), (31, 39), (54, 64), (17, 75), (54, 128)])
def test_generators_reach_every_branch(m, nf):
    rng = np.random.default_rng(m + nf)
    c = R.inputs(rng, 6, m, nf, n_slack=0 if nf == 128 else 3)
    assert c["nw"] <= 128 and c["nf"] <= c["nw"] and c["n"] > nf
    assert (np.diff(c["free_idx"]) >= 1).all() and c["free_idx"].max() < c["n"]
    assert nf == 1 or (np.diff(c["free_idx"]) > 1).any()  # fixed variables in between
    if m * nf >= 31:
        for kind in (-1, -2):
            assert (c["amap"] == kind).any()
        pos = c["amap"][c["amap"] >= 0]
        assert len(pos) and len(np.unique(pos)) == len(pos) and pos.max() < c["nnz_rec"]
        assert np.isnan(c["J_old"][:, pos]).any() and np.isnan(c["J_new"][:, pos]).any()
    s, yk, yabs = R.pair(c)
    assert np.isfinite(yk.astype(np.float64)).all() and (np.abs(yk) <= yabs).all()
    # aim_pair lands the pair where it is told to, on both sides of the decision
    S, Y = R.spd_pairs(rng, 1, nf, 4)
    R.aim_pair(c, 0, S[0], Y[0])
    R.aim_pair(c, 1, S[0], -Y[0])
    s, yk, _ = R.pair(c)
    take, guard, *_ = R.decision(s, yk)
    assert take[0] and not take[1] and (guard[:2] > 1e-6).all()
    assert np.abs(yk[0] - Y[0]).max() <= 8 * R.EPS * np.abs(yabs[0]).max()


def test_float64_baseline_loses_digits_with_the_span():
    """What lets the graded cases tell a good recursion from a bad one: the float64 dense recursion is at
    rounding level on span-0 pairs and loses digits as the pairs' curvatures spread."""
    worst = {}
    for nf in (5, 39):
        for span in (0, 4, 8):
            errs = []
            for seed in range(8):
                rng = np.random.default_rng(100 * span + seed)
                S, Y = R.spd_pairs(rng, R.LM_HIST, nf, span)
                take, guard, sy, ss, _ = R.decision(S, Y)
                assert take.all() and (guard > 1e3).all()  # every generated pair is far on the taken side
                sigma = float(R.sigma_of(sy[-1:], ss[-1:])[0])
                errs.append(R.ferr(R.dense_model(S, Y, sigma, dtype=np.float64), R.dense_model(S, Y, sigma)))
            worst[nf, span] = max(errs)
        assert worst[nf, 0] < 16 * R.EPS, worst
        assert worst[nf, 4] > worst[nf, 0] and worst[nf, 8] > 100 * worst[nf, 4], worst  # two digits and more
    assert worst[5, 4] > 100 * worst[5, 0], worst
