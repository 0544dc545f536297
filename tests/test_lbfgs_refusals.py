"""What cpl_ipm_lbfgs_update, cpl_ipm_newton_setup_ex and cpl_ipm_lm_model_doubles refuse before any launch:
bad sizes, sizes beyond the kernels' LDS rows, an unknown form, the one-wave form above nf = 64, a dense
Hessian together with a compact model, a compact model without pairs or without rows, each missing required
buffer; and batch = 0 is CPL_OK.  No device calls, as in test_line_search_refusals.py.

No call here can reach a launch.  The bad-size calls pass no buffer at all.  The missing-buffer calls pass
host addresses for the other buffers and a batch of 2^40 instances, more than a grid holds: were a buffer
check dropped, the call would still end before the launch ("batch too large"), and the test would fail by
the message."""
import pytest

from centroidalplanner_amd import _abi
from test_line_search_refusals import DUMMY, HUGE, _bufs, _refused

LBFGS = ["amap", "free_idx", "act", "failed", "w_old", "w_new", "y", "dy", "alpha", "gw_old", "J_old", "grad_new",
         "J_new", "lm_s", "lm_y", "lm_cnt", "lm_skip", "Hc"]
LBFGS_ROWS = ["amap", "y", "dy", "J_old", "J_new"]  # read only with m > 0
SETUP_IN = ["w", "zL", "zU", "gw", "A", "y", "c", "f", "mu", "hasL", "hasU", "wl0", "wu0"]
SETUP_OUT = ["M", "r1", "r2", "gphi", "mr_diag", "theta", "phi"]
SETUP_ROWS = ["A", "y", "c", "r2"]


def lbfgs(batch=HUGE, n=5, m=2, nf=3, nw=4, nnz=6, form=0, missing="all"):
    return _abi.lib.cpl_ipm_lbfgs_update(batch, n, m, nf, nw, nnz, *_bufs(LBFGS, missing), form, None)


def setup(batch=HUGE, nw=3, m=2, nf=2, H=False, Hc=True, lm_pairs=6, missing="all"):
    ins, outs = _bufs(SETUP_IN, missing), _bufs(SETUP_OUT, missing)
    return _abi.lib.cpl_ipm_newton_setup_ex(batch, nw, m, nf, *ins, DUMMY if H else None, 0, *outs,
                                            DUMMY if Hc else None, lm_pairs, None, None)


def test_model_length():
    f = _abi.lib.cpl_ipm_lm_model_doubles
    assert f(39, 6) == 2 + 2 * 6 * 39 and f(128, 9) == 2 + 2 * 9 * 128 and f(0, 6) == 2
    assert f(-1, 6) == -1 and f(5, 0) == -1 and f(5, -2) == -1


@pytest.mark.parametrize("call,word", [
    (lambda: lbfgs(batch=-1), "bad sizes"), (lambda: lbfgs(nf=0), "bad sizes"), (lambda: lbfgs(nf=-1), "bad sizes"),
    (lambda: lbfgs(nf=5, nw=4), "bad sizes"), (lambda: lbfgs(nf=4, n=3, nw=4), "bad sizes"),
    (lambda: lbfgs(m=-1), "bad sizes"), (lambda: lbfgs(n=0), "bad sizes"), (lambda: lbfgs(nnz=-1), "bad sizes"),
    (lambda: lbfgs(nw=129, nf=100, n=100), "nw > 128"), (lambda: lbfgs(nw=129, nf=129, n=129), "nw > 128"),
    (lambda: lbfgs(m=257), "m > 256"),
    (lambda: lbfgs(form=3), "unknown form"), (lambda: lbfgs(form=-1), "unknown form"),
    (lambda: lbfgs(form=2, nf=65, nw=65, n=65), "one-wave form"),
    (lambda: setup(batch=-1), "bad sizes"), (lambda: setup(nf=4), "bad sizes"), (lambda: setup(nw=129), "nw > 128"),
    (lambda: setup(H=True), "a dense Hessian and a compact model"),
    (lambda: setup(lm_pairs=0), "lm_pairs > 0"), (lambda: setup(lm_pairs=-3), "lm_pairs > 0"),
    (lambda: setup(nf=0), "nf > 0"),
    (lambda: setup(nw=128, nf=128, lm_pairs=8), "too large"),
])
def test_refused_with_no_buffer_at_all(call, word):
    _refused(call(), word)


def test_size_refusals_come_before_the_empty_batch():
    for rc in (lbfgs(batch=0, nw=129, nf=100, n=100), lbfgs(batch=0, form=7),
               lbfgs(batch=0, form=2, nf=65, nw=65, n=65), setup(batch=0, H=True), setup(batch=0, lm_pairs=0),
               setup(batch=0, nf=0)):
        assert rc == _abi.ERR_INVALID_ARGUMENT


def test_an_empty_batch_is_ok_without_buffers():
    for form in (0, 1, 2):
        assert lbfgs(batch=0, form=form) == 0
    assert lbfgs(batch=0, m=0) == 0 and lbfgs(batch=0, nf=128, nw=128, n=128, m=256, form=1) == 0
    assert setup(batch=0) == 0 and setup(batch=0, Hc=False, lm_pairs=0) == 0
    assert setup(batch=0, nw=64, nf=64, lm_pairs=9) == 0 and setup(batch=0, nw=128, nf=128, lm_pairs=7) == 0


@pytest.mark.parametrize("name", [n for n in LBFGS if n != "grad_new"])
def test_each_missing_update_buffer_is_an_invalid_argument(name):
    _refused(lbfgs(missing=name), "missing buffer")
    _refused(lbfgs(missing=name, form=1), "missing buffer")


@pytest.mark.parametrize("name", SETUP_IN + SETUP_OUT)
def test_each_missing_setup_buffer_is_an_invalid_argument_with_a_compact_model(name):
    _refused(setup(missing=name), "missing buffer")


def test_optional_buffers_are_not_required():
    """With every optional buffer absent and every required one present the calls pass their argument checks
    (they end at the grid limit, not at a missing buffer): grad_new, the row buffers of m = 0, the compact
    model itself."""
    for rc in [lbfgs(missing="grad_new"), lbfgs(missing=None)] + [lbfgs(m=0, missing=n) for n in LBFGS_ROWS] + \
              [setup(missing=None), setup(Hc=False, missing=None), setup(Hc=False, lm_pairs=-1, missing=None)] + \
              [setup(m=0, missing=n) for n in SETUP_ROWS]:
        _refused(rc, "batch too large")
