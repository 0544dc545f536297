"""What the five line-search entry points (cpl_ipm_post_step, cpl_ipm_trial_point, cpl_ipm_judge_take,
cpl_ipm_accept, cpl_ipm_masked_rows) refuse before any launch: bad sizes, a mode other than 0, each
missing required buffer; and batch = 0 is CPL_OK.  No device calls, as in test_abi.py.

No call here can reach a launch.  The bad-size calls pass no buffer at all.  The missing-buffer calls pass
host addresses for the other buffers and a batch of 2^40 instances, more than a grid holds: were a buffer
check dropped, the call would still end before the launch ("batch too large"), and the test would fail by
the message."""
import ctypes

import pytest

from centroidalplanner_amd import _abi

_HOST = (ctypes.c_double * 16)()
DUMMY = ctypes.c_void_p(ctypes.addressof(_HOST))
HUGE = 1 << 40
INVALID = _abi.ERR_INVALID_ARGUMENT

TRIAL = ["free_idx", "fixed_idx", "Xbase", "w", "dir", "alpha", "mask", "w_keep", "wt", "X"]
JUDGE = ["row_slack", "gl", "hasL", "hasU", "wl0", "wu0", "wt", "f_t", "g_t", "alpha", "mu", "theta_k", "phi_k", "gd",
         "switch_ok", "theta_max", "filt_t", "filt_p", "extra_mask", "searching", "st_f", "st_g", "st_w", "st_alpha",
         "st_aug", "th_out", "ok_out"]
POST = ["w", "dw", "zL", "zU", "gphi", "mu", "tau", "hasL", "hasU", "wl0", "wu0", "theta", "theta_min", "active",
        "delta_w", "dwl", "dzL", "dzU", "a_max", "a_z", "gd", "switch_ok"]
ACCEPT = ["active", "aug", "failed", "rest", "alpha", "a_z", "theta", "phi", "filt_t_in", "filt_p_in", "fcount_in",
          "w_new", "dy", "dzL", "dzU", "mu", "hasL", "hasU", "wl0", "wu0", "w", "y", "zL", "zU", "mu_state", "iters",
          "filt_t", "filt_p", "fcount"]
ROWS = ["mask", "src", "dst"]
OPTIONAL = {"judge": {"extra_mask"}, "accept": {"failed", "rest"}}


def _bufs(names, missing):
    """None for every buffer (missing = all), or host addresses with one buffer missing."""
    return [None if missing == "all" or n == missing else DUMMY for n in names]


def trial(batch=HUGE, n=3, nf=2, nw=3, missing="all"):
    return _abi.lib.cpl_ipm_trial_point(batch, n, nf, nw, *_bufs(TRIAL, missing), None)


def judge(batch=HUGE, nw=3, m=2, nf=2, nfilt=3, mode=0, missing="all"):
    return _abi.lib.cpl_ipm_judge_take(batch, nw, m, nf, nfilt, *_bufs(JUDGE, missing), mode, None)


def post(batch=HUGE, nw=3, missing="all"):
    return _abi.lib.cpl_ipm_post_step(batch, nw, *_bufs(POST, missing), None)


def accept(batch=HUGE, nw=3, m=2, nfilt=3, missing="all"):
    return _abi.lib.cpl_ipm_accept(batch, nw, m, nfilt, *_bufs(ACCEPT, missing), None)


def rows(batch=HUGE, row_len=1024, missing="all"):
    return _abi.lib.cpl_ipm_masked_rows(batch, row_len, *_bufs(ROWS, missing), None)


def _refused(rc, word):
    assert rc == INVALID
    assert word in _abi.lib.cpl_last_error().decode(), _abi.lib.cpl_last_error()


@pytest.mark.parametrize("call", [
    lambda: trial(batch=-1), lambda: trial(nw=0, nf=0), lambda: trial(nf=4, n=5, nw=3), lambda: trial(nf=3, n=2),
    lambda: trial(n=0, nf=0), lambda: trial(nf=-1),
    lambda: judge(batch=-1), lambda: judge(nw=0, nf=0), lambda: judge(nf=4), lambda: judge(nfilt=-1),
    lambda: judge(mode=1), lambda: judge(mode=-1), lambda: judge(m=-1), lambda: judge(nf=-1),
    lambda: post(batch=-1), lambda: post(nw=0), lambda: post(nw=-3),
    lambda: accept(batch=-1), lambda: accept(nw=0), lambda: accept(nfilt=0), lambda: accept(nfilt=-1),
    lambda: accept(m=-1),
    lambda: rows(batch=-1), lambda: rows(row_len=-1),
])
def test_bad_sizes_are_invalid_arguments(call):
    _refused(call(), "bad sizes")


@pytest.mark.parametrize("fn", [trial, judge, post, accept, rows])
def test_an_empty_batch_is_ok_without_buffers(fn):
    assert fn(batch=0) == 0
    assert fn is not rows or rows(batch=5, row_len=0) == 0


def _required(kind, names):
    return [n for n in names if n not in OPTIONAL.get(kind, ())]


@pytest.mark.parametrize("fn,kind,name", [(f, k, n) for f, k, names in (
    (trial, "trial", TRIAL), (judge, "judge", JUDGE), (post, "post", POST), (accept, "accept", ACCEPT),
    (rows, "rows", ROWS)) for n in _required(k, names)])
def test_each_missing_required_buffer_is_an_invalid_argument(fn, kind, name):
    _refused(fn(missing=name), "missing buffer")


def test_optional_buffers_are_not_required():
    """With every optional buffer absent and every required one present the call passes its argument checks
    (it ends at the grid limit, not at a missing buffer); the row buffers of m = 0, the filter of nfilt = 0
    and fixed_idx with n = nf are optional too."""
    for rc in (judge(missing="extra_mask"), judge(m=0, missing="row_slack"), judge(m=0, missing="st_g"),
               judge(nfilt=0, missing="filt_t"), accept(missing="failed"), accept(missing="rest"),
               accept(m=0, missing="dy"), trial(n=2, nf=2, missing="fixed_idx")):
        _refused(rc, "batch too large")
