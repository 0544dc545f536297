"""Recomputation of IPOPT's unscaled termination measures from the oracle's callbacks alone (shared by
the termination tests): nothing here reads a measure from the solver under test.

  * nlp_scaling_factors: IPOPT's gradient-based scaling factors df [B], dc [B, m] at the start point
    (the rule cpl_solve_options.nlp_scaling documents), in numpy from pyoracle.eval_batch;
  * iterate_x: the last iterate's x (the returned x is its projection onto the original bounds, which
    moves a variable on a relaxed bound by up to 1e-8 max(1, |bound|) — far more than the tolerances the
    tests set) from the returned w;
  * unscaled_measures: at (x, y, z_L, z_U), the unscaled dual infeasibility
        x part      |grad f + J^T y - (z_L - z_U) / df|        (y: the returned, unscaled multipliers)
        slack of r  |-y_r - (z_L - z_U)_s dc_r / df|
    and the unscaled constraint violation of g(x), each with the size of its largest un-cancelled term
    (what a relative tolerance of the recomputation refers to; for g, whose rows are sums of forces and
    of position x force products, |x|max (1 + |x|max)).
"""
import numpy as np

import pyoracle

MAX_GRADIENT, MIN_VALUE = 100.0, 1e-8


def layout(prob):
    """free variable indices, inequality rows, and the bounds (xl, xu, gl, gu)"""
    xl, xu, gl, gu = prob.get_bounds_info()
    fixed = np.abs(xu - xl) <= 1e-14 * np.maximum(1.0, np.abs(xl))
    return np.where(~fixed)[0], np.where(gl != gu)[0], (xl, xu, gl, gu)


def dense_jac(prob, jac):
    n, m, _ = prob.get_nlp_info()
    iRow, jCol = prob.get_structure()
    J = np.zeros((jac.shape[0], m, n))
    J[:, iRow, jCol] = np.nan_to_num(jac, nan=0.0)
    return J


def nlp_scaling_factors(prob, X0, mass):
    free, I, (xl, xu, gl, gu) = layout(prob)
    Xb = np.array(X0, dtype=np.float64)
    fixed = np.setdiff1d(np.arange(Xb.shape[1]), free)
    Xb[:, fixed] = xl[fixed]
    o = pyoracle.eval_batch(prob.desc(), Xb, mass, None, outputs=("jac", "grad"), nthreads=1)
    B, m = Xb.shape[0], gl.size
    gmax = np.abs(np.nan_to_num(o["grad"][:, free], nan=0.0)).max(1)
    df = np.where(gmax > MAX_GRADIENT, np.maximum(MAX_GRADIENT / np.where(gmax > 0, gmax, 1.0), MIN_VALUE), 1.0)
    dc = np.ones((B, m))
    rmax = np.abs(dense_jac(prob, o["jac"])[:, :, free]).max(2)
    for rows in (np.where(gl == gu)[0], I):
        if rows.size == 0:
            continue
        need = rmax[:, rows].max(1) > MAX_GRADIENT
        d = np.maximum(MAX_GRADIENT * (1.0 / np.maximum(rmax[:, rows], MAX_GRADIENT)), MIN_VALUE)
        dc[:, rows] = np.where(need[:, None], d, 1.0)
    return df, dc


def iterate_x(prob, x, w):
    free, _, _ = layout(prob)
    xi = np.array(x, dtype=np.float64)
    xi[:, free] = w[:, :free.size]
    return xi


def unscaled_measures(prob, mass, x, y, zL, zU, df, dc):
    """-> dict(dual_inf, dual_terms, constr_viol, viol_terms), each [B]"""
    free, I, (xl, xu, gl, gu) = layout(prob)
    nf = free.size
    o = pyoracle.eval_batch(prob.desc(), np.ascontiguousarray(x), mass, None, outputs=("g", "jac", "grad"), nthreads=1)
    J = dense_jac(prob, o["jac"])[:, :, free]
    dz = zL - zU
    terms = [o["grad"][:, free], dz[:, :nf] / df[:, None]] + [J[:, r, :] * y[:, r:r + 1] for r in range(y.shape[1])]
    dual_x = o["grad"][:, free] + np.einsum("brk,br->bk", J, y) - dz[:, :nf] / df[:, None]
    sl = dz[:, nf:] * dc[:, I] / df[:, None]
    dual_s = -y[:, I] - sl
    g = o["g"]
    viol = np.maximum(np.maximum(gl - g, g - gu), 0.0).max(1)
    return {"dual_inf": np.maximum(np.abs(dual_x).max(1), np.abs(dual_s).max(1) if I.size else 0.0),
            "dual_terms": np.maximum(np.max([np.abs(t).max(1) for t in terms], axis=0),
                                     np.maximum(np.abs(y[:, I]).max(1), np.abs(sl).max(1)) if I.size else 0.0),
            "constr_viol": viol, "viol_terms": np.abs(x).max(1) * (1.0 + np.abs(x).max(1))}
