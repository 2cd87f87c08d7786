"""State estimator, the parts that need no GPU: the C-ABI of include/scpqp_estimator.h
(exports, constants and the plant parameters by a gcc probe of the header, argument validation
without touching a device), the CPU mirror's anchors and known answers
(tests/estimator_mirror.py) and scpqp.estimator's host side.

Bounds.  F against expm(A T): the remainder of the exponential series after the quadratic
term, ||A T||^3 / 6 * e^||A T|| in the 2-norm.  The known answers of a diagonal problem: 1e-13
relative, a few dozen roundings of 2^-53 with no transcendental involved; the Joseph form of a
full P: the same times cond(S), the amplification of a solve with S, relative to
sqrt(P_ii P_jj).  The steering variance over n ticks: each tick is phi * P * phi + T q^2 and a
halving sum, at most four roundings, so 4 n 2^-53 relative.  The consistency bound is the
mirror's own (``consistency_verdict``): five standard deviations of the mean of 9000
chi-square(5) variables, 0.167."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg
import torch

import estimator_mirror as EM
from oracle import plant_reference as PR
from scpqp import _lib as LB
from scpqp import estimator as EST
from scpqp import plant as PL
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_estimator.h")
E_ARG, E_SIZE = -1, -4
LF = LR = 0.34
TICK = 0.01


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------------------
# 1. boundary
# ---------------------------------------------------------------------------
def test_estimator_header_declares_the_boundary():
    assert header_functions() == sorted(LB.EST_EXPORTS) == ["scpqp_est_step"]
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS) | set(LB.OBSTACLE_EXPORTS)
              | set(LB.SENSE_EXPORTS))
    assert not set(LB.EST_EXPORTS) & others
    txt = open(HEADER).read()
    for word in ("LAG", "BIAS_HEADING", "SCALE_SPEED", "not wrapped", "Off row", "Bad row"):
        assert word in txt, word


def test_library_exports_the_estimator_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.EST_EXPORTS:
        assert hasattr(lib, name)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_estimator.h"
int main(void) {
  printf("psize %zu\n", sizeof(scpqp_plant_params));
  printf("n_veh %zu\n", offsetof(scpqp_plant_params, n_veh));
  printf("lf %zu\n", offsetof(scpqp_plant_params, lf));
  printf("lr %zu\n", offsetof(scpqp_plant_params, lr));
  printf("ns %d\n", SCPQP_EST_NS);
  printf("np %d\n", SCPQP_EST_NP);
  printf("idx %d%d%d%d%d%d%d%d\n", SCPQP_EST_R_POS, SCPQP_EST_R_HEADING, SCPQP_EST_R_SPEED,
         SCPQP_EST_R_STEER, SCPQP_EST_Q_POS, SCPQP_EST_Q_HEADING, SCPQP_EST_Q_SPEED,
         SCPQP_EST_Q_STEER);
  printf("maxveh %d\n", SCPQP_MAX_VEH);
  return 0;
}
"""


def test_estimator_ctypes_layout_matches_header(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["psize"]) == C.sizeof(LB.PlantParams)
    for f in ("n_veh", "lf", "lr"):
        assert int(got[f]) == getattr(LB.PlantParams, f).offset, f
    assert int(got["ns"]) == LB.EST_NS == EM.NS == EST.NS == 5
    assert int(got["np"]) == LB.EST_NP == EM.NP == EST.NP == 8
    assert got["idx"] == "01234567"
    assert (LB.EST_R_POS, LB.EST_R_HEADING, LB.EST_R_SPEED, LB.EST_R_STEER, LB.EST_Q_POS,
            LB.EST_Q_HEADING, LB.EST_Q_SPEED, LB.EST_Q_STEER) == tuple(range(8)) \
        == (EM.R_POS, EM.R_HEADING, EM.R_SPEED, EM.R_STEER, EM.Q_POS, EM.Q_HEADING, EM.Q_SPEED,
            EM.Q_STEER)
    assert EST.FIELDS == LB.EST_FIELDS and len(EST.FIELDS) == 8
    assert int(got["maxveh"]) == LB.MAX_VEH
    # the declared argument list: 13 arguments, two of them doubles, in the header's order
    proto = re.search(r"int scpqp_est_step\((.*?)\);", open(HEADER).read(), re.S).group(1)
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    assert len(args) == len(lib.scpqp_est_step.argtypes) == 13
    for a, t in zip(args, lib.scpqp_est_step.argtypes):
        if a.startswith("double "):
            assert t is C.c_double, a
        elif a.startswith("int32_t "):
            assert t is C.c_int32, a
        else:
            assert "*" in a and t in (C.c_void_p, C.POINTER(LB.PlantParams)), a


def test_est_step_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    D = C.cast(buf, C.c_void_p)
    P = PL.plant_params([LF, 0.3], [LR, 0.3])

    def err():
        return lib.scpqp_last_error()

    def step(p=P, B=0, n_span=8, tick=TICK, h_max=PL.H_MAX, u=None, m=None, deliv=None, est=None,
             x=None, cov=None, nis=None):
        return lib.scpqp_est_step(None if p is None else C.byref(p), B, n_span, tick, h_max, u, m,
                                  deliv, est, x, cov, nis, None)

    assert step() == 0                                      # B = 0: a no-op, NULL arrays
    assert step(n_span=0) == 0
    assert step(p=None) == E_ARG and b"null plant" in err()
    for n in (0, -1, LB.MAX_VEH + 1):
        q = PL.plant_params([LF], [LR])
        q.n_veh = n
        assert step(p=q) == E_ARG and b"n_veh" in err()
    q = PL.plant_params([LF, 0.0], [LR, 0.0])
    assert step(p=q) == E_ARG and b"lf + lr" in err()
    assert step(B=-1) == E_ARG and b"batch" in err()
    assert step(n_span=-1) == E_ARG and b"n_span" in err()
    for t in (0.0, -0.01, math.nan, math.inf):
        assert step(tick=t) == E_ARG and b"tick" in err()
        assert step(h_max=t) == E_ARG and b"h_max" in err()
    full = dict(u=D, m=D, est=D, x=D, cov=D)
    for missing, word in (("u", b"u_span"), ("m", b"x_meas"), ("est", b"est"), ("x", b"x_est"),
                          ("cov", b"cov")):
        kw = dict(full)
        kw[missing] = None
        assert step(B=3, **kw) == E_ARG and word in err(), missing
    # sizes before the pointers: nothing is launched for a size error
    assert step(B=1 << 27, **full) == E_SIZE and b"25" in err()
    assert step(B=1 << 27) == E_SIZE
    assert step(B=1 << 20, n_span=1 << 11, **full) == E_SIZE and b"n_span" in err()


# ---------------------------------------------------------------------------
# 2. mirror anchors
# ---------------------------------------------------------------------------
STATES = [np.array([1.0, -2.0, 0.3, 4.0, 0.5, 0.02]), np.array([0.0, 0.0, -2.5, 9.0, -1.0, -0.25]),
          np.array([5.0, 5.0, 1.2, 0.5, 0.0, 0.4])]


@pytest.mark.parametrize("x", STATES)
def test_jacobian_has_nine_nonzeros_and_matches_the_right_hand_side(x):
    A = EM.jacobian5(x, LF, LR)
    assert np.count_nonzero(A) == 9 and A[4, 4] == -10.0
    # central differences of the flow's own right-hand side: O(h^2) truncation, h = 1e-6
    h = 1e-6
    for k, s in enumerate(EM.IDX):
        d = np.zeros(6)
        d[s] = h
        fd = (EM.rhs5(x + d, 0.1, LF, LR) - EM.rhs5(x - d, 0.1, LF, LR)) / (2 * h)
        assert np.abs(fd - A[:, k]).max() <= 1e-7 * max(1.0, np.abs(A).max()), k


@pytest.mark.parametrize("x", STATES)
def test_transition_against_the_matrix_exponential(x):
    A = EM.jacobian5(x, LF, LR)
    F = EM.transition(x, LF, LR, TICK)
    nrm = np.linalg.norm(A * TICK, 2)
    bound = nrm ** 3 / 6 * math.exp(nrm)
    diff = np.linalg.norm(F - scipy.linalg.expm(A * TICK), 2)
    print(f"||F - expm(AT)|| = {diff:.3e}, bound {bound:.3e} at ||AT|| = {nrm:.3f}")
    assert diff <= bound
    assert F[4, 4] == 1 - 10 * TICK + 50 * TICK ** 2 and (F[4, :4] == 0).all()


def _spd(seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((5, 5)) * np.array([0.05, 0.05, 0.01, 0.1, 0.002])[:, None]
    return G @ G.T + np.diag([1e-4, 1e-4, 1e-6, 1e-4, 1e-8])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_update_against_the_joseph_form(seed):
    P = _spd(seed)
    r = EM.r_diag([0.05, 0.01, 0.1, 0.002, 0, 0, 0, 0])
    x = STATES[0].copy()
    m = x + np.array([0.03, -0.02, 0.004, 0.05, 0.1, 0.001])
    x1, P1, nis = EM.update(x, P, m, r)
    K = P @ np.linalg.inv(P + np.diag(r))
    I = np.eye(5)
    joseph = (I - K) @ P @ (I - K).T + K @ np.diag(r) @ K.T
    scale = np.sqrt(np.outer(np.diag(P), np.diag(P)))
    assert (np.abs(P1 - joseph) <= 1e-13 * scale * np.linalg.cond(P + np.diag(r))).all()
    y = (m - x)[EM.IDX]
    assert abs(nis - y @ np.linalg.solve(P + np.diag(r), y)) <= 1e-12 * nis
    assert np.abs(x1[EM.IDX] - (x[EM.IDX] + K @ y)).max() <= 1e-13 and x1[4] == m[4]
    assert (P1 == P1.T).all() and np.linalg.eigvalsh(P1).min() > 0


# ---------------------------------------------------------------------------
# 3. known answers
# ---------------------------------------------------------------------------
ROW = np.array([0.05, 0.01, 0.1, 0.002, 0.02, 0.01, 0.05, 0.01])


def test_two_measurements_average():
    m1 = np.array([1.0, -2.0, 0.3, 4.0, 0.5, 0.02])
    m2 = m1 + np.array([0.07, -0.04, 0.012, 0.15, -0.2, 0.003])
    x, cov = np.full(6, np.nan), np.zeros((5, 5))
    x, cov, nis = EM.lane_step(ROW, LF, LR, TICK, (), m1, 1, x, cov)
    assert (x == m1).all() and (cov == np.diag(EM.r_diag(ROW))).all() and math.isnan(nis)
    x, cov, nis = EM.lane_step(ROW, LF, LR, TICK, (), m2, 1, x, cov)
    r = EM.r_diag(ROW)
    want = 0.5 * (m1 + m2)
    assert np.abs(x[EM.IDX] - want[EM.IDX]).max() <= 1e-13 * np.abs(want).max()
    assert x[4] == m2[4]
    assert (np.abs(np.diag(cov) - r / 2) <= 1e-13 * r / 2).all()
    assert (cov - np.diag(np.diag(cov)) == 0).all()
    want_nis = (((m2 - m1)[EM.IDX]) ** 2 / (2 * r)).sum()
    assert abs(nis - want_nis) <= 1e-13 * want_nis


@pytest.mark.parametrize("q_steer", [0.0, 0.01])
def test_steering_variance_over_a_predicted_span(q_steer):
    row = ROW.copy()
    row[EM.Q_STEER] = q_steer
    P = _spd(3)
    n = 8
    u = 0.03 * np.sin(0.2 * np.arange(n))
    _, P1 = EM.predict(STATES[0], P, u, LF, LR, TICK, EM.q_diag(row))
    phi = 1 - 10 * TICK + 50 * TICK ** 2
    p = P[4, 4]
    for _ in range(n):
        p = phi * phi * p + TICK * q_steer ** 2
    ulp = abs(P1[4, 4] - p) / np.spacing(p)
    print(f"steering variance off by {ulp:.1f} ulp after {n} ticks (Q_STEER = {q_steer})")
    assert abs(P1[4, 4] - p) <= 4 * n * 2.0 ** -53 * p


def test_a_lost_step_is_the_flow_of_the_previous_estimate():
    x0 = STATES[0]
    P = _spd(4)
    u = 0.03 * np.sin(0.2 * np.arange(8))
    m = x0 + 1.0                                             # never looked at
    for delivered, meas in ((0, m), (1, np.where(np.arange(6) == 2, np.nan, m))):
        x, cov, nis = EM.lane_step(ROW, LF, LR, TICK, u, meas, delivered, x0, P)
        want = x0.copy()
        for uj in u:
            want = PR._rk4_flow(want, TICK, float(uj), LF, LR, PR._rk4_steps(TICK))
        assert (x == want).all() and math.isnan(nis)
        assert (cov == cov.T).all() and np.linalg.eigvalsh(cov).min() > 0
    # not initialised and not measured: stays NaN; then initialises on the next measurement
    x, cov, nis = EM.lane_step(ROW, LF, LR, TICK, u, m, 0, np.full(6, np.nan), P)
    assert np.isnan(x).all() and (cov == P).all() and math.isnan(nis)
    x, cov, nis = EM.lane_step(ROW, LF, LR, TICK, u, m, 1, x, cov)
    assert (x == m).all() and (cov == np.diag(EM.r_diag(ROW))).all()


def test_off_and_bad_rows_of_the_mirror():
    m = STATES[1]
    P = _spd(5)
    x, cov, nis = EM.lane_step(np.zeros(8), LF, LR, TICK, (0.1,), m, 1, STATES[0], P)
    assert (x == m).all() and (cov == P).all() and math.isnan(nis)
    for f, val in ((0, -1e-3), (5, math.nan), (7, math.inf), (2, 0.0), (0, 0.0)):
        row = ROW.copy()
        row[f] = val
        assert EM.is_bad_row(row)
        x, cov, nis = EM.lane_step(row, LF, LR, TICK, (0.1,), m, 1, STATES[0], P)
        assert np.isnan(x).all() and np.isnan(cov).all() and math.isnan(nis)
    assert not EM.is_bad_row(ROW) and not EM.is_bad_row(np.zeros(8))
    # a pivot that is not positive: the lane turns NaN
    x, cov, nis = EM.lane_step(ROW, LF, LR, TICK, (), m, 1, STATES[0], -np.eye(5))
    assert np.isnan(x).all() and np.isnan(cov).all() and math.isnan(nis)


# ---------------------------------------------------------------------------
# 4. consistency (mirror alone): the condition the GPU statistical test also uses
# ---------------------------------------------------------------------------
def test_mirror_is_consistent_on_the_statistical_inputs():
    N = 1500
    truth, u, meas, rows = EM.consistency_inputs(N)
    x, cov = np.full((N, 1, 6), np.nan), np.zeros((N, 1, 5, 5))
    every = []
    for s in range(EM.CONS_STEPS + 1):
        us = None if s == 0 else np.broadcast_to(u[s - 1], (N, 1, EM.CONS_SPAN))
        nis = EM.step([EM.CONS_LF], [EM.CONS_LR], EM.CONS_TICK, us, meas[s][:, None], None,
                      rows[:, None], x, cov)
        assert np.isnan(nis).all() if s == 0 else np.isfinite(nis).all()
        if s:
            every.append(nis)
        # P stays symmetric with a positive smallest eigenvalue
        assert (cov == cov.transpose(0, 1, 3, 2)).all()
        assert np.linalg.eigvalsh(cov[:, 0]).min() > 0
    mean, bound, rms_est, rms_meas = EM.consistency_verdict(np.array(every), x[:, 0], truth[-1],
                                                             meas[-1])
    print(f"mean NIS {mean:.3f} (|mean - 5| <= {bound:.3f}); RMS position error {rms_est:.4f} m "
          f"of the estimate, {rms_meas:.4f} m of the measurement")
    assert np.array(every).size == 9000 and abs(bound - 0.167) < 5e-4
    assert abs(mean - 5.0) <= bound
    assert rms_est < rms_meas


# ---------------------------------------------------------------------------
# 5. scpqp.estimator's host side
# ---------------------------------------------------------------------------
def test_validate_names_the_row_and_the_field():
    good = EST.rows(3, 2, device="cpu").numpy()
    EST.validate(good)
    EST.validate(np.zeros((3, 2, 8)))
    assert EST.is_off(np.zeros((3, 2, 8))) and not EST.is_off(good)
    for (b, v, f), val, what in (((2, 1, 5), math.nan, "q_heading is not finite"),
                                 ((0, 1, 0), math.inf, "r_pos is not finite"),
                                 ((1, 0, 7), -1e-9, "q_steer must be >= 0"),
                                 ((2, 0, 3), 0.0, "r_steer must be > 0")):
        bad = good.copy()
        bad[b, v, f] = val
        with pytest.raises(ValueError, match=rf"rows\[{b}, {v}\]: {what}"):
            EST.validate(bad)
        with pytest.raises(ValueError):
            EST.validate(torch.as_tensor(bad))
        assert EM.is_bad_row(bad[b, v])
    for shape in ((3, 2, 7), (3, 8), (3, 2, 8, 1)):
        with pytest.raises(ValueError, match="rows must be"):
            EST.validate(np.zeros(shape))


def test_rows_broadcast_and_from_table():
    r = EST.rows(4, 3, r_pos=np.array([[0.01], [0.02], [0.05], [0.1]]), q_steer=0.0, device="cpu")
    assert tuple(r.shape) == (4, 3, 8) and r.dtype == torch.float64
    assert r[:, :, 0].tolist() == [[0.01] * 3, [0.02] * 3, [0.05] * 3, [0.1] * 3]
    assert (r[..., 7] == 0).all() and (r[..., 1] == 0.01).all()
    with pytest.raises(ValueError, match="r_speed does not broadcast"):
        EST.rows(4, 3, r_speed=np.ones(5), device="cpu")
    with pytest.raises(ValueError, match=r"rows\[0, 0\]: r_pos must be > 0"):
        EST.rows(4, 3, r_pos=0.0, device="cpu")
    table = torch.stack([EST.rows(1, 3, r_pos=s, device="cpu")[0] for s in (0.01, 0.1)])
    got = EST.from_table(table, [1, 0, 1], device="cpu")
    assert got[:, 0, 0].tolist() == [0.1, 0.01, 0.1]
    with pytest.raises(ValueError, match="outside the table"):
        EST.from_table(table, [2], device="cpu")
    off = EST.off(2, 3, device="cpu")
    assert EST.is_off(off) and tuple(off.shape) == (2, 3, 8)
    x, cov = EST.alloc(2, 3, device="cpu")
    assert torch.isnan(x).all() and tuple(x.shape) == (2, 3, 6)
    assert (cov == 0).all() and tuple(cov.shape) == (2, 3, 5, 5)


def test_matched_raises_the_sigmas_to_the_floors():
    s = np.zeros((2, 3, 8))
    s[..., 5] = 1.0
    s[0, :, 0] = 0.05                 # sig_pos above its floor
    s[1, :, 1] = 1e-5                 # sig_heading below its floor
    s[..., 4], s[..., 6], s[..., 7] = 0.2, 0.1, 3.0   # bias, drop, lag: not the filter's business
    r = EST.matched(s, floor=(1e-3, 2e-3, 3e-3, 4e-3), q=(0.1, 0.2, 0.3, 0.4), device="cpu").numpy()
    assert (r[0, :, 0] == 0.05).all() and (r[1, :, 0] == 1e-3).all()
    assert (r[..., 1] == 2e-3).all() and (r[..., 2] == 3e-3).all() and (r[..., 3] == 4e-3).all()
    assert (r[..., 4:] == np.array([0.1, 0.2, 0.3, 0.4])).all()
    EST.validate(r)
    d = EST.matched(torch.as_tensor(s)).numpy()      # lives where the sensing rows live
    assert (d[..., :4] >= np.array(EST.FLOOR)).all() and (d[..., 4:] == np.array(EST.Q_DEFAULT)).all()
    with pytest.raises(ValueError, match="floor"):
        EST.matched(s, floor=(0.0, 1e-3, 1e-3, 1e-3), device="cpu")
    with pytest.raises(ValueError, match="sensing rows"):
        EST.matched(np.zeros((2, 3, 5)), device="cpu")


def test_step_refuses_host_tensors():
    P = PL.plant_params([LF, LF], [LR, LR])
    B, V = 2, 2
    rows = EST.rows(B, V, device="cpu")
    x_est, cov = EST.alloc(B, V, device="cpu")
    m = torch.zeros((B, V, 6), dtype=torch.float64)
    with pytest.raises(ValueError, match="rows must be .* on the GPU"):
        EST.step(P, None, TICK, m, None, rows, x_est, cov)
    with pytest.raises(ValueError, match="rows must be"):
        EST.step(P, None, TICK, m, None, rows.numpy(), x_est, cov)
