"""References for the Superquadric part of the analytic Lagrangian Hessian
(cpl_lagrangian_hessian_ex, csrc/cpl_kernels.hip sq_axis_terms / sq_pair_entry).

A Superquadric contact's environment row S(p) - 1 (multiplier y_e) and its three normal rows
n + nu(p) (multipliers y_k) are the only rows with curvature in p alone; they add one 3 x 3 block
per contact on p_i x p_i.  Three things live here:

  * `sq_blocks`: the numpy float64 restatement of the closed form, in the kernel's operation order
    (d_a = p_a - C_a; e, h, t; r = |e|; nu = e / r; M_ka = delta_ka - nu_k nu_a; D_ka = M_ka h_a / r),
    with the degenerate-contact rule (r zero or not finite, or a non-finite entry: the whole block
    counts as 0) and, per entry, the magnitude sum A of its terms — the products of the factors'
    absolute values, with |delta_ka| + |nu_k nu_a| for M_ka, so that A does not shrink where
    1 - nu_k^2 cancels;
  * `mp_blocks`: the same blocks by 60-digit mpmath differentiation of the restated rows
    y_e S(p) + sum_k y_k nu_k(p) themselves (mpmath.diff, no closed form);
  * `lagrangian_hessian`: the whole Hessian — pyoracle.lagrangian_hessian (cost, torque, cones: it
    reads only the row layout from the template) plus the blocks.

The parameter sets and points of the accuracy tests (tests/test_sq_hessian_ref.py on the CPU,
tests/test_gpu_sq_hessian.py on the GPU) are built here once and cached.
"""
import functools

import numpy as np

U = 2.0 ** -53  # unit round-off of float64

# TestBasic's Superquadric (tests/TestBasic.cpp:150-157) and three other exponent sets on its C, R
SQ_C = (0.0, 0.0, 1.0)
SQ_R = (0.3, 0.3, 10.0)
PARAM_SETS = {
    "testbasic": (SQ_C, SQ_R, (10.0, 10.0, 10.0)),
    "p222": (SQ_C, SQ_R, (2.0, 2.0, 2.0)),
    "p352": (SQ_C, SQ_R, (3.0, 5.0, 2.0)),
    "p25_37_4": (SQ_C, SQ_R, (2.5, 3.7, 4.0)),  # non-integer exponents: points with d > 0 only
}
CURVED_SETS = ("testbasic", "p352", "p25_37_4")  # P > 2 somewhere: the t term does not vanish

# The float64 restatement against the exact value, relative to A: every term is a chain of at most
# 14 multiplications / divisions of factors that are themselves within 1 (a power: numpy's pow, the
# kernel's double-double ladder), 3 (r: three squares, two sums, a square root) or 5 (nu = e / r)
# round-offs of exact — at most 14 + 2 (powers) + 4 * 5 (four nu or r factors) + 3 (M's difference
# against |delta| + |nu nu|) = 39 round-offs — and the sum of the terms adds at most 13 more.
RHO_NUMPY_BOUND = 52 * U
# cpl_lagrangian_hessian_ex may lie this many times further from the exact value than the numpy
# restatement does on the same inputs (the figure tests/test_gpu_kkt_precision.py settled on for
# the same kind of bound; the measured ratios are in tests/test_gpu_sq_hessian.py's docstring)
GPU_MARGIN = 8.0


def make_sq_problem(N, params, env="superquadric"):
    """A Superquadric (or mixed Ground + Superquadric) template with the given (C, R, P)."""
    from centroidalplanner_amd.problem import CplProblem, Ground, MixedEnvironment, Superquadric
    from centroidalplanner_amd.workload import GROUND_Z, MU, WRENCH

    C, R, P = params
    s = Superquadric()
    s.SetParameters(np.array(C), np.array(R), np.array(P))
    if env == "mixed":
        g = Ground()
        g.SetGroundZ(GROUND_Z)
        e = MixedEnvironment(g, s)
    else:
        e = s
    e.SetMu(MU)
    prob = CplProblem([f"contact{i + 1}" for i in range(N)], 100.0, e)
    prob.SetManipulationWrench(WRENCH)
    return prob


def points(N, B, params, seed, positive=None):
    """(X [B, n], y [B, m]): the workload's Superquadric instances (p from its box
    [-0.5, 0.5]^2 x [0.5, 1.5] with |d_a| >= 1e-3), d > 0 for non-integer exponents."""
    from centroidalplanner_amd.workload import generate

    C, _, P = params
    X, _, _ = generate(N, "superquadric", B, seed)
    if positive is None:
        positive = any(float(q) != np.floor(q) for q in P)
    if positive:
        for i in range(N):
            p = X[:, 6 + 9 * i: 9 + 9 * i]
            p[:] = np.asarray(C) + np.abs(p - np.asarray(C))
    y = np.random.default_rng(seed + 1).normal(scale=50.0, size=(B, 6 + 6 * N))
    return X, y


def sq_blocks(params, p, ye, yk, drop=None):
    """The closed-form blocks of contacts at p [B, 3] with multipliers ye [B], yk [B, 3]:
    (H [B, 3, 3], A [B, 3, 3], ok [B]).  H is 0 where ok is False (a degenerate contact).
    drop: "t" leaves the t_a term out, "r2" the 1 / r^2 term (wrong formulas: the tests show that
    the accuracy bound rejects them)."""
    C, R, P = (np.asarray(v, dtype=np.float64) for v in params)
    p = np.asarray(p, dtype=np.float64)
    B = p.shape[0]
    with np.errstate(all="ignore"):
        d = -C + p
        EJ = P / np.power(R, P)
        e = EJ * np.power(d, P - 1.0)
        h = (EJ * (P - 1.0)) * np.power(d, P - 2.0)
        t = np.where(P == 2.0, 0.0, ((EJ * (P - 1.0)) * (P - 2.0)) * np.power(d, np.where(P == 2.0, 1.0, P - 3.0)))
        r = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        nu = e / r[:, None]
        H = np.zeros((B, 3, 3))
        A = np.zeros((B, 3, 3))

        def M(k, c):
            return (1.0 if k == c else 0.0) - nu[:, k] * nu[:, c]

        def Ma(k, c):
            return (1.0 if k == c else 0.0) + np.abs(nu[:, k] * nu[:, c])

        def D(k, c):
            return M(k, c) * h[:, c] / r

        def Da(k, c):
            return Ma(k, c) * np.abs(h[:, c]) / r

        for a in range(3):
            for b in range(a, 3):
                v = ye * h[:, a] if a == b else np.zeros(B)
                m = np.abs(v)
                for k in range(3):
                    term = M(k, a) * t[:, a] / r if (a == b and drop != "t") else np.zeros(B)
                    mag = Ma(k, a) * np.abs(t[:, a]) / r if a == b else np.zeros(B)
                    term = term - (D(k, b) * nu[:, a] + nu[:, k] * D(a, b)) * h[:, a] / r
                    mag = mag + (Da(k, b) * np.abs(nu[:, a]) + np.abs(nu[:, k]) * Da(a, b)) * np.abs(h[:, a]) / r
                    if drop != "r2":
                        term = term - M(k, a) * h[:, a] * nu[:, b] * h[:, b] / (r * r)
                    mag = mag + Ma(k, a) * np.abs(h[:, a] * nu[:, b] * h[:, b]) / (r * r)
                    v = v + yk[:, k] * term
                    m = m + np.abs(yk[:, k]) * mag
                H[:, a, b] = H[:, b, a] = v
                A[:, a, b] = A[:, b, a] = m
        ok = (r > 0.0) & np.isfinite(r) & np.isfinite(H).all(axis=(1, 2))
    H[~ok] = 0.0
    return H, A, ok


def contact_blocks(prob, params, X, y, drop=None):
    """sq_blocks of every contact of every instance: (H [B, N, 3, 3], A, ok [B, N])."""
    d = prob.desc()
    N = int(d.n_contacts)
    B = X.shape[0]
    H, A, ok = np.zeros((B, N, 3, 3)), np.zeros((B, N, 3, 3)), np.zeros((B, N), dtype=bool)
    for k in range(N):
        i = int(d.map_order[k])  # contact i sits at block position k of the rows
        r0 = 6 + 6 * k
        H[:, i], A[:, i], ok[:, i] = sq_blocks(params, X[:, 6 + 9 * i: 9 + 9 * i], y[:, r0], y[:, r0 + 1: r0 + 4],
                                               drop=drop)
    return H, A, ok


def mp_blocks(prob, params, X, y):
    """contact_blocks' H by mpmath differentiation (60 digits) of the restated rows: per contact,
    L(p) = y_e (sum_a ((p_a - C_a) / R_a)^P_a - 1) + sum_k y_k (n_k + nu_k(p)), nu = e / |e|,
    e_a = P_a / R_a^P_a (p_a - C_a)^(P_a - 1) (src/Superquadric.cpp:40-69).  float64 [B, N, 3, 3]
    (each entry the correctly rounded 60-digit value)."""
    import mpmath as mp

    d = prob.desc()
    N = int(d.n_contacts)
    B = X.shape[0]
    out = np.zeros((B, N, 3, 3))
    with mp.workdps(60):
        C, R, P = ([mp.mpf(float(v)) for v in q] for q in params)

        def make(ye, yk):
            def L(p0, p1, p2):
                pp = (p0, p1, p2)
                S = sum(((pp[a] - C[a]) / R[a]) ** P[a] for a in range(3)) - 1
                e = [P[a] / R[a] ** P[a] * (pp[a] - C[a]) ** (P[a] - 1) for a in range(3)]
                r = mp.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2)
                return ye * S + sum(yk[k] * e[k] / r for k in range(3))
            return L

        for b in range(B):
            for k in range(N):
                i = int(d.map_order[k])
                r0 = 6 + 6 * k
                L = make(mp.mpf(float(y[b, r0])), [mp.mpf(float(v)) for v in y[b, r0 + 1: r0 + 4]])
                pt = tuple(mp.mpf(float(v)) for v in X[b, 6 + 9 * i: 9 + 9 * i])
                for a in range(3):
                    for c in range(a, 3):
                        order = [0, 0, 0]
                        order[a] += 1
                        order[c] += 1
                        v = float(mp.diff(L, pt, tuple(order)))
                        out[b, i, a, c] = out[b, i, c, a] = v
    return out


def rho(Hblk, Hmp, A):
    """max |H - H_mp| / A over the entries of every block, per instance [B]."""
    q = np.abs(Hblk - Hmp) / A
    return q.reshape(q.shape[0], -1).max(axis=1)


def lagrangian_hessian(prob, params, X, y, free=None, sq=None, drop=None, desc=None):
    """The whole Hessian of f + y^T g [B, nf, nf]: cost, torque and cone entries from
    pyoracle.lagrangian_hessian, plus the Superquadric blocks of the instances `sq` (default all).
    desc: the template to take the cost weights from (default prob's)."""
    import pyoracle

    d = prob.desc() if desc is None else desc
    N = int(d.n_contacts)
    H = pyoracle.lagrangian_hessian(d, X, y, None)
    blk, _, _ = contact_blocks(prob, params, X, y, drop=drop)
    rows = np.ones(X.shape[0], dtype=bool) if sq is None else np.asarray(sq, dtype=bool)
    for i in range(N):
        s = slice(6 + 9 * i, 9 + 9 * i)
        H[rows, s, s] += blk[rows, i]
    if free is not None:
        fi = np.asarray(free, dtype=np.int64)
        H = H[:, fi][:, :, fi]
    return H


def free_of(prob):
    xl, xu, _, _ = prob.get_bounds_info()
    return np.where(~(np.abs(xu - xl) <= 1e-14 * np.maximum(1.0, np.abs(xl))))[0]


@functools.lru_cache(maxsize=None)
def accuracy_case(name, N=4, B=37):
    """The accuracy tests' inputs and references for one parameter set, computed once:
    dict(prob, params, X, y, H_np, A, H_mp, rho_np [B], rho_drop_t [B], rho_drop_r2 [B])."""
    params = PARAM_SETS[name]
    prob = make_sq_problem(N, params)
    X, y = points(N, B, params, seed=100 + sorted(PARAM_SETS).index(name))
    H_np, A, ok = contact_blocks(prob, params, X, y)
    assert ok.all()
    H_mp = mp_blocks(prob, params, X, y)
    out = {"prob": prob, "params": params, "X": X, "y": y, "H_np": H_np, "A": A, "H_mp": H_mp,
           "rho_np": rho(H_np, H_mp, A)}
    for drop in ("t", "r2"):
        Hd, _, _ = contact_blocks(prob, params, X, y, drop=drop)
        out["rho_drop_" + drop] = rho(Hd, H_mp, A)
    return out
