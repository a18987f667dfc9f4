"""sga_optimize_batch (csrc/optimizer.hip): the lock-step host LM / GN over several pairs, on the CPU.

The contract under test: for every pair of a batch the sequence of linearize / error requests and the returned sga_result are EXACTLY
those of sga_optimize run on that pair alone with the same callbacks — np.array_equal on every field, the request poses in order.  The
reductions are the oracle's (as in test_abi.py::test_host_optimizer_reproduces_oracle) over the C1 clouds from different initial poses,
so that the pairs finish in different rounds.
"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib

FIELDS = ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error")


def same_result(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def _pose(rz, tx, ty):
    T = np.eye(4)
    c, s = np.cos(rz), np.sin(rz)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [tx, ty, 0.0]
    return T


# different distances from the optimum: the pairs need different numbers of outer iterations
INIT_POSES = [np.eye(4), _pose(0.02, 0.3, -0.2), _pose(-0.05, -0.6, 0.4), _pose(0.1, 1.0, 0.8), _pose(0.003, 0.01, 0.0)]


class Recorder:
    """oracle reductions of one pair that record the poses they are asked at"""

    def __init__(self, orc, tc, sc, setting):
        self.orc, self.tc, self.sc, self.s = orc, tc, sc, setting
        self.f = orc.Factors(len(sc))
        self.log = []

    def lin(self, T):
        self.log.append(("lin", T.copy()))
        return self.orc.linearize(self.tc, self.sc, self.s, T, self.f)

    def err(self, T):
        self.log.append(("err", T.copy()))
        return self.orc.error(self.tc, self.sc, self.s, T, self.f)


def same_log(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("optimizer", ["LM", "GN"])
@pytest.mark.parametrize("restrict", [False, True])
def test_batch_equals_lone_bit_for_bit(orc, c1_oracle_clouds, optimizer, restrict):
    tc, sc = c1_oracle_clouds
    os_ = orc.default_setting(factor_kind=orc.GICP, num_threads=1)
    kw = dict(restrict_dof_lambda=1e3, restrict_dof_mask=[1, 1, 0, 1, 0, 1]) if restrict else {}
    st = sga.make_setting("GICP", optimizer=optimizer, **kw)
    lone_recs = [Recorder(orc, tc, sc, os_) for _ in INIT_POSES]
    lone = [sga.optimize(st, T0, r.lin, r.err) for T0, r in zip(INIT_POSES, lone_recs)]
    recs = [Recorder(orc, tc, sc, os_) for _ in INIT_POSES]
    rounds = []  # the pairs served by each batched linearize request

    def lin(k, T):
        rounds.append(k)
        return recs[k].lin(T)

    res = sga.optimize_batch(st, INIT_POSES, lin, lambda k, T: recs[k].err(T))
    assert len(res) == len(INIT_POSES)
    for k in range(len(INIT_POSES)):
        assert same_result(res[k], lone[k]), (k, res[k], lone[k])
        assert same_log(recs[k].log, lone_recs[k].log), k
    iters = [r.iterations for r in lone]
    assert len(set(iters)) > 1, iters  # the pairs did finish in different rounds: the test exercises the shrinking active list
    # a pair that is done is never asked again: pair k was linearized exactly as often as alone
    for k in range(len(INIT_POSES)):
        assert rounds.count(k) == sum(1 for kind, _ in lone_recs[k].log if kind == "lin")


def test_lm_failure_of_one_pair_leaves_the_others_alone(orc, c1_oracle_clouds):
    """optimizer.hpp:141-143 for pair 1 of three (test_host_optimizer_lm_failure_path's construction): ten rejected trials end it with
    converged = False while its neighbours converge as they do alone."""
    tc, sc = c1_oracle_clouds
    os_ = orc.default_setting(factor_kind=orc.GICP, num_threads=1)
    st = sga.make_setting("GICP")
    calls = {"lin": 0, "err": 0}

    def bad_lin(T):
        calls["lin"] += 1
        return np.eye(6), np.ones(6), 1.0, 5

    def bad_err(T):
        calls["err"] += 1
        return 2.0  # never better

    lone_bad = sga.optimize(st, np.eye(4), bad_lin, bad_err)
    assert calls == {"lin": 1, "err": 10}
    inits = [INIT_POSES[1], np.eye(4), INIT_POSES[2]]
    lone_recs = {k: Recorder(orc, tc, sc, os_) for k in (0, 2)}
    lone = {k: sga.optimize(st, inits[k], lone_recs[k].lin, lone_recs[k].err) for k in (0, 2)}
    recs = {k: Recorder(orc, tc, sc, os_) for k in (0, 2)}
    calls.update(lin=0, err=0)
    res = sga.optimize_batch(st, inits, lambda k, T: bad_lin(T) if k == 1 else recs[k].lin(T), lambda k, T: bad_err(T) if k == 1 else recs[k].err(T))
    assert calls == {"lin": 1, "err": 10}
    assert same_result(res[1], lone_bad) and not res[1].converged and res[1].iterations == 0
    for k in (0, 2):
        assert same_result(res[k], lone[k]) and same_log(recs[k].log, lone_recs[k].log)
        assert res[k].converged


def test_callback_failure_count_zero_and_argument_checks():
    """SGA_ERR_CALLBACK from either callback; count == 0 is SGA_OK and calls nothing; null arguments give SGA_ERR_INVALID and the
    combinations a batch does not take give SGA_ERR_UNSUPPORTED — all before any device work, so also where there is no GPU."""
    lib = sga.load()
    OK, INVALID, UNSUPPORTED, CALLBACK = 0, 1, 4, 5
    st = sga.make_setting("GICP")
    res = (_lib.ResultC * 2)()
    T2 = np.ascontiguousarray(np.stack([np.eye(4).reshape(16)] * 2))
    Tp = T2.ctypes.data_as(C.POINTER(C.c_double))
    asked = []

    def lin_fail(user, count, active, T, H, b, e, n):
        asked.append("lin")
        return 1

    def lin_ok(user, count, active, T, H, b, e, n):
        for k in range(count):
            if active[k]:
                for i in range(36):
                    H[36 * k + i] = 1.0 if i % 7 == 0 else 0.0
                for i in range(6):
                    b[6 * k + i] = 1.0
                e[k], n[k] = 1.0, 5
        return 0

    def err_fail(user, count, active, T, e):
        asked.append("err")
        return 7

    LF, EF = _lib.BATCH_LINEARIZE_FN, _lib.BATCH_ERROR_FN
    assert lib.sga_optimize_batch(C.byref(st), 2, Tp, LF(lin_fail), EF(err_fail), None, res) == CALLBACK
    assert asked == ["lin"]
    assert lib.sga_optimize_batch(C.byref(st), 2, Tp, LF(lin_ok), EF(err_fail), None, res) == CALLBACK
    assert asked == ["lin", "err"]
    assert b"callback" in lib.sga_last_error()
    # count == 0: nothing is called, nothing is written
    del asked[:]
    assert lib.sga_optimize_batch(C.byref(st), 0, None, LF(lin_fail), EF(err_fail), None, None) == OK and asked == []
    # init_T == NULL: every pair starts from the identity
    gn = sga.make_setting("GICP", optimizer="GN", max_iterations=1)
    assert lib.sga_optimize_batch(C.byref(gn), 2, None, LF(lin_ok), EF(), None, res) == OK
    assert res[0].iterations == 0 and res[1].num_inliers == 5
    # null arguments
    assert lib.sga_optimize_batch(None, 2, Tp, LF(lin_ok), EF(err_fail), None, res) == INVALID
    assert lib.sga_optimize_batch(C.byref(st), 2, Tp, LF(), EF(err_fail), None, res) == INVALID
    assert lib.sga_optimize_batch(C.byref(st), 2, Tp, LF(lin_ok), EF(), None, res) == INVALID  # LM needs the error callback
    assert lib.sga_optimize_batch(C.byref(st), 2, Tp, LF(lin_ok), EF(err_fail), None, None) == INVALID
    out = C.c_void_p()
    n = C.c_size_t()
    d = (C.c_double * 96)()
    assert lib.sga_batch_create(None, None, 0, C.byref(out)) == INVALID
    assert lib.sga_batch_create(None, None, 1, None) == INVALID
    assert lib.sga_batch_size(None, C.byref(n)) == INVALID
    assert lib.sga_batch_destroy(None) == OK
    assert lib.sga_batch_linearize(None, None, C.byref(st.factor), d, None, d, d, d, None) == INVALID
    assert lib.sga_batch_linearize(None, None, None, d, None, d, d, d, None) == INVALID
    assert lib.sga_align_batch(None, None, None, C.byref(st), res) == INVALID
    assert lib.sga_align_batch(None, None, None, None, res) == INVALID
    # what a batch does not take is refused whatever it is asked of: fp64 arithmetic, robust kernels, the error model switched off
    for kw in (dict(math_mode="fp64"), dict(robust_kernel="HUBER"), dict(robust_kernel="CAUCHY")):
        bad = sga.make_setting("GICP", **kw)
        assert lib.sga_batch_linearize(None, None, C.byref(bad.factor), d, None, d, d, d, None) == UNSUPPORTED
        assert lib.sga_align_batch(None, None, None, C.byref(bad), res) == UNSUPPORTED
    sga.set_error_model(False)
    try:
        assert lib.sga_align_batch(None, None, None, C.byref(st), res) == UNSUPPORTED
        assert lib.sga_batch_linearize(None, None, C.byref(st.factor), d, None, d, d, d, None) == UNSUPPORTED
    finally:
        sga.set_error_model(True)
    bad = sga.make_setting("GICP")
    bad.factor.factor_kind = 7
    assert lib.sga_align_batch(None, None, None, C.byref(bad), res) == INVALID


def test_verbose_lines_carry_the_pair_number(capfd):
    st = sga.make_setting("GICP", optimizer="GN", max_iterations=2, verbose=True)
    sga.optimize_batch(st, [np.eye(4), np.eye(4)], lambda k, T: (np.eye(6), np.zeros(6), 1.0, 3), lambda k, T: 0.0)
    C.CDLL(None).fflush(None)  # the lines sit in the C library's buffer
    out = capfd.readouterr().out
    assert "pair=0 iter=0" in out and "pair=1 iter=0" in out
