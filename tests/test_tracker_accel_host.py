"""Obstacle tracker with an acceleration state, the parts that need no GPU: the C-ABI of
include/scpqp_tracker_accel.h (exports, constants by a gcc probe of the header, argument
validation without touching a device), the CPU mirror's anchors and known answers
(tests/tracker_accel_mirror.py), the derivation of the tolerance the GPU tests use, and
scpqp.tracker_accel's host side.

Bounds.
  p' and r' against an 80-bit evaluation (a 30-term series in ``numpy.longdouble``): twice the
  header's figures, 1e-15 relative for the series below the switch, 4e-13 for the closed form
  of p' on [0.3, 4] and 6e-14 for that of r' on [0.3, 2]; 4e-16 absolute for r' on [2, 4],
  where it has a zero.  Measured: 1.5e-16 and 3.7e-16 (series), 1.3e-13 (p'), 1.5e-14 (r'), 8e-17.
  The Jacobian against central differences of the mirror's flow: 1e-8 absolute, the bound of
  tests/test_tracker_host.py by its reasoning (entries of order s T + a T^2 <= 2, a step of
  1e-5: truncation 2e-11, rounding ulp(30) / h = 4e-10).  Measured: 7.4e-11 at most over the
  cases below.
  At a stop F holds T_e fixed.  The position rows still agree with the central differences of
  the flow (the speed at the stop is 0, so the dependence of the stop time on s and a does not
  move the position to first order); the heading row lacks w / (-a) and w s / a^2 in the
  columns of s and a, and the speed row keeps 1 and T_e where the flow has 0.  The test
  documents exactly that.
  Known answers of a diagonal problem: 1e-13 relative.
  The reduction to the five-state mirror: tracker_accel_cases.RED_TOL, 16 times the measured
  6.74e-14, rounded up to a power of two.
  The consistency bound is five standard deviations of the mean of 18000 chi-square(4)
  variables, 0.105.  Measured on the mirror: mean NIS 4.004 (the five-state tracker on the
  same measurements: 178); RMS position error 2.5 s ahead 0.193 m against 5.525 m of the
  five-state tracker.  The braking frog obstacles, on the mirrors: 329.6 m summed prediction
  error from step 3 on against 1514.8 m, a ratio of 0.218."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import manoeuvre_mirror as MNM
import obstacle_mirror as OM
import tracker_accel_cases as TC
import tracker_accel_mirror as AM
import tracker_mirror as TM
from scpqp import _lib as LB
from scpqp import tracker_accel as TRKA
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_tracker_accel.h")
E_ARG, E_SIZE = -1, -4
LD = np.longdouble


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
def test_header_declares_the_boundary():
    assert header_functions() == sorted(LB.TRKA_EXPORTS) == ["scpqp_obstacles_track_accel"]
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS) | set(LB.OBSTACLE_EXPORTS)
              | set(LB.SENSE_EXPORTS) | set(LB.EST_EXPORTS) | set(LB.TRK_EXPORTS)
              | set(LB.MAN_EXPORTS))
    assert not set(LB.TRKA_EXPORTS) & others
    assert LB.TRK_EXPORTS == ("scpqp_obstacles_track",)
    txt = open(HEADER).read()
    for word in ("A_HOLD", "W_HOLD", "P0_ACCEL", "A_CLAMP", "not wrapped", "not clamped", "Off row",
                 "Bad row", "0.3", "No new Philox site", "T_e held fixed", "never moves backwards"):
        assert word in txt, word


def test_library_exports_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.TRKA_EXPORTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_tracker_accel.h"
int main(void) {
  printf("ns %d\n", SCPQP_TRKA_NS);
  printf("nz %d\n", SCPQP_TRKA_NZ);
  printf("np %d\n", SCPQP_TRKA_NP);
  printf("idx %d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n", SCPQP_TRKA_R_POS,
         SCPQP_TRKA_R_HEADING, SCPQP_TRKA_R_SPEED, SCPQP_TRKA_Q_POS, SCPQP_TRKA_Q_HEADING,
         SCPQP_TRKA_Q_SPEED, SCPQP_TRKA_Q_YAW, SCPQP_TRKA_Q_ACCEL, SCPQP_TRKA_P0_YAW,
         SCPQP_TRKA_P0_ACCEL, SCPQP_TRKA_W_CLAMP, SCPQP_TRKA_A_CLAMP, SCPQP_TRKA_W_HOLD,
         SCPQP_TRKA_A_HOLD);
  printf("switch %.17g\n", SCPQP_TRKA_DPR_SWITCH);
  printf("dsinc %.17g\n", SCPQP_TRK_DSINC_SWITCH);
  printf("pr %.17g\n", SCPQP_MAN_PR_SWITCH);
  printf("maxobst %d\n", SCPQP_MAX_OBST);
  printf("ssize %zu\n", sizeof(scpqp_sense_stream));
  return 0;
}
"""


def test_ctypes_layout_matches_header(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["ns"]) == LB.TRKA_NS == AM.NS == TRKA.NS == 6
    assert int(got["nz"]) == LB.TRKA_NZ == AM.NZ == TRKA.NZ == 4
    assert int(got["np"]) == LB.TRKA_NP == AM.NP == TRKA.NP == 14
    assert got["idx"] == ",".join(str(i) for i in range(14))
    assert (LB.TRKA_R_POS, LB.TRKA_R_HEADING, LB.TRKA_R_SPEED, LB.TRKA_Q_POS, LB.TRKA_Q_HEADING,
            LB.TRKA_Q_SPEED, LB.TRKA_Q_YAW, LB.TRKA_Q_ACCEL, LB.TRKA_P0_YAW, LB.TRKA_P0_ACCEL,
            LB.TRKA_W_CLAMP, LB.TRKA_A_CLAMP, LB.TRKA_W_HOLD, LB.TRKA_A_HOLD) == tuple(range(14)) \
        == (AM.R_POS, AM.R_HEADING, AM.R_SPEED, AM.Q_POS, AM.Q_HEADING, AM.Q_SPEED, AM.Q_YAW,
            AM.Q_ACCEL, AM.P0_YAW, AM.P0_ACCEL, AM.W_CLAMP, AM.A_CLAMP, AM.W_HOLD, AM.A_HOLD)
    assert float(got["switch"]) == LB.TRKA_DPR_SWITCH == AM.DPR_SWITCH == 0.3
    assert float(got["dsinc"]) == AM.DSINC_SWITCH == LB.TRK_DSINC_SWITCH
    assert float(got["pr"]) == AM.PR_SWITCH == LB.MAN_PR_SWITCH
    assert TRKA.FIELDS == LB.TRKA_FIELDS and len(TRKA.FIELDS) == 14
    assert int(got["maxobst"]) == LB.MAX_OBST
    assert int(got["ssize"]) == C.sizeof(LB.SenseStream)
    # the declared argument list: that of scpqp_obstacles_track, 17 arguments in its order
    proto = re.search(r"int scpqp_obstacles_track_accel\((.*?)\);", open(HEADER).read(),
                      re.S).group(1)
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    assert len(args) == len(lib.scpqp_obstacles_track_accel.argtypes) == 17
    assert list(lib.scpqp_obstacles_track_accel.argtypes) == list(lib.scpqp_obstacles_track.argtypes)
    five = re.search(r"int scpqp_obstacles_track\((.*?)\);",
                     open(os.path.join(ROOT, "include", "scpqp_tracker.h")).read(), re.S).group(1)
    assert args == [a.strip() for a in five.replace("\n", " ").split(",")]
    for a, t in zip(args, lib.scpqp_obstacles_track_accel.argtypes):
        if a.startswith("double "):
            assert t is C.c_double, a
        elif a.startswith("int32_t "):
            assert t is C.c_int32, a
        else:
            assert "*" in a and t in (C.c_void_p, C.POINTER(LB.SenseStream)), a


def test_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    D = C.cast(buf, C.c_void_p)
    ST = LB.SenseStream(seed=1, epoch=0, b_offset=0)

    def err():
        return lib.scpqp_last_error()

    def track(B=0, n_obst=3, hp=5, rows=None, osense=None, st=None, trk=None, t_meas=0.0,
              t_since=0.4, lead=0.1, dt=0.4, x=None, cov=None, z=None, nis=None, out=None):
        return lib.scpqp_obstacles_track_accel(B, n_obst, hp, rows, osense,
                                               None if st is None else C.byref(st), trk, t_meas,
                                               t_since, lead, dt, x, cov, z, nis, out, None)

    assert track() == 0                                     # B = 0: a no-op, NULL arrays
    assert track(t_since=0.0) == 0
    assert track(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_OBST + 1):
        assert track(n_obst=n) == E_ARG and b"n_obst" in err()
    for h in (0, -1, LB.MAX_HP + 1):
        assert track(hp=h) == E_ARG and b"hp" in err()
    for t in (-1e-9, -0.4, math.nan, math.inf):
        assert track(t_since=t) == E_ARG and b"t_since" in err()
    for kw in (dict(t_meas=math.nan), dict(lead=math.inf), dict(dt=math.nan)):
        assert track(**kw) == E_ARG and b"finite" in err()
    full = dict(rows=D, trk=D, x=D, cov=D, out=D)
    for missing, word in (("rows", b"rows"), ("trk", b"trk"), ("x", b"x_trk"), ("cov", b"cov"),
                          ("out", b"output")):
        kw = dict(full)
        kw[missing] = None
        assert track(B=3, **kw) == E_ARG and word in err(), missing
    # an osense array needs its stream; without osense the stream may be NULL
    assert track(B=3, osense=D, **full) == E_ARG and b"stream" in err()
    # sizes before the pointers: nothing is launched for a size error.  2^26 * 36 > 2^31 - 1
    assert track(B=1 << 26, n_obst=1, **full) == E_SIZE and b"36" in err()
    assert track(B=1 << 26, n_obst=1) == E_SIZE
    assert track(B=1 << 22, n_obst=4, hp=64, osense=D, st=ST, **full) == E_SIZE and b"hp" in err()


# ---------------------------------------------------------------------------
# 2. mirror anchors: the piece, p' and r', the Jacobian
# ---------------------------------------------------------------------------
def test_the_generic_piece_is_the_manoeuvre_mirrors_in_float64():
    rng = np.random.default_rng(0)
    for _ in range(500):
        q = tuple(rng.uniform(-3, 3, 3)) + (rng.uniform(0, 4),)
        a = float(rng.choice([0.0, -1.5, 2.0, rng.uniform(-3, 3)]))
        w = float(rng.choice([0.0, 1e-5, 0.05, rng.uniform(-2, 2)]))
        tau = float(rng.uniform(0, 4))
        want = MNM.piece(q, a, w, tau)[:4]
        got = AM.piece(tuple(np.float64(v) for v in q), np.float64(a), np.float64(w),
                       np.float64(tau))
        assert all(float(g) == float(m) for g, m in zip(got, want))
    for th in (0.0, 0.05, 0.0999, 0.1, 0.7, -0.3):
        assert AM.p_of(np.float64(th)) == MNM.p_of(th) and AM.r_of(np.float64(th)) == MNM.r_of(th)
        assert AM.sinc(np.float64(th)) == OM.sinc(th)
        assert AM.dsinc(np.float64(th)) == TM.dsinc(th)


def _dp_ref(th):
    th, s = LD(th), LD(0)
    for k in range(30):
        s += (-1) ** k * th ** (2 * k + 1) / (LD(math.factorial(2 * k + 1)) * (2 * k + 4))
    return -s


def _dr_ref(th):
    th, s = LD(th), LD(0)
    for k in range(30):
        s += (-1) ** k * th ** (2 * k) / (LD(math.factorial(2 * k)) * (2 * k + 3))
    return s


def _rel(got, want):
    return abs(float((LD(got) - want) / want))


def test_both_branches_of_dp_and_dr_against_long_double():
    if np.finfo(LD).eps > 1e-18:
        pytest.fail("numpy's long double is not an 80-bit type on this machine")
    S = AM.DPR_SWITCH
    # next to the switch, both branches
    for factor in (0.999, 1.0, 1.001):
        for sign in (1.0, -1.0):
            th = np.float64(sign * factor * S)
            assert _rel(AM.dp_series(th), _dp_ref(th)) <= 1e-15
            assert _rel(AM.dr_series(th), _dr_ref(th)) <= 1e-15
            assert _rel(AM.dp_closed(th), _dp_ref(th)) <= 4e-13
            assert _rel(AM.dr_closed(th), _dr_ref(th)) <= 6e-14
    # over each branch's range
    worst = dict(dps=0.0, drs=0.0, dpc=0.0, drc=0.0, drc_abs=0.0)
    for th in np.linspace(1e-6, S * 0.9999, 1500):
        for t in (np.float64(th), np.float64(-th)):
            worst["dps"] = max(worst["dps"], _rel(AM.dp_series(t), _dp_ref(t)))
            worst["drs"] = max(worst["drs"], _rel(AM.dr_series(t), _dr_ref(t)))
    for th in np.linspace(S, 4.0, 3000):
        for t in (np.float64(th), np.float64(-th)):
            worst["dpc"] = max(worst["dpc"], _rel(AM.dp_closed(t), _dp_ref(t)))
            if th <= 2.0:
                worst["drc"] = max(worst["drc"], _rel(AM.dr_closed(t), _dr_ref(t)))
            else:
                worst["drc_abs"] = max(worst["drc_abs"],
                                       abs(float(LD(AM.dr_closed(t)) - _dr_ref(t))))
    print("p', r' against 80-bit:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["dps"] <= 1e-15 and worst["drs"] <= 1e-15
    assert worst["dpc"] <= 4e-13 and worst["drc"] <= 6e-14 and worst["drc_abs"] <= 4e-16
    # the switch selects the branches; the limits
    assert AM.dp_of(np.float64(0.0)) == 0.0 and AM.dr_of(np.float64(0.0)) == 1.0 / 3.0
    lo, hi = np.float64(0.999 * S), np.float64(S)
    assert AM.dp_of(lo) == AM.dp_series(lo) and AM.dr_of(lo) == AM.dr_series(lo)
    assert AM.dp_of(hi) == AM.dp_closed(hi) and AM.dr_of(-hi) == AM.dr_closed(-hi)
    # they are the derivatives of p and r
    for th in (0.05, 0.2, 0.29, 0.31, 1.0, -0.7):
        h = 1e-5
        dp = (MNM.p_of(th + h) - MNM.p_of(th - h)) / (2 * h)
        dr = (MNM.r_of(th + h) - MNM.r_of(th - h)) / (2 * h)
        assert abs(dp - AM.dp_of(np.float64(th))) < 1e-8 and abs(dr - AM.dr_of(np.float64(th))) < 1e-8


T_JAC = 0.4
# theta = w T on both sides of every switch: sinc (|theta / 2| = 1e-4), g' (0.02), p and r
# (0.1), p' and r' (0.3)
W_JAC = [0.0, 1e-9, 1.8e-4 / T_JAC, 2.2e-4 / T_JAC, 0.038 / T_JAC, 0.042 / T_JAC, 0.095 / T_JAC,
         0.105 / T_JAC, 0.29 / T_JAC, 0.31 / T_JAC, -1.2, 3.0]
NONZERO = ((0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (3, 5))


def _central(x, T, h=1e-5):
    num = np.empty((6, 6))
    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        num[:, j] = (AM.flow(x + d, np.float64(T)) - AM.flow(x - d, np.float64(T))) / (2 * h)
    return num


@pytest.mark.parametrize("w", W_JAC)
def test_jacobian_against_central_differences_of_the_flow(w):
    worst = 0.0
    for h0, s in ((0.3, 4.0), (-2.5, 1.5)):
        for a in (-1.0, 0.0, 0.8):                          # no stop within T_JAC
            x = np.array([1.0, -2.0, h0, s, w, a])
            F = AM.transition(x, np.float64(T_JAC))
            worst = max(worst, float(np.abs(F - _central(x, T_JAC)).max()))
            # twelve off-diagonal nonzeros (ten distinct values) on a unit diagonal
            off = F - np.eye(6)
            mask = np.zeros((6, 6), bool)
            for r, c in NONZERO:
                mask[r, c] = True
            assert (off[~mask] == 0.0).all() and F[2, 4] == T_JAC == F[3, 5]
    print(f"w = {w}: largest |F - central difference| {worst:.2e}")
    assert worst <= 1e-8


def test_at_a_stop_the_jacobian_holds_the_stop_time_fixed():
    h0, s, w, a = 0.3, 0.5, 0.6, -2.5                       # stops after 0.2 s < T_JAC
    x = np.array([1.0, -2.0, h0, s, w, a])
    F = AM.transition(x, np.float64(T_JAC))
    num = _central(x, T_JAC)
    Te = s / -a
    got = AM.flow(x, np.float64(T_JAC))
    assert got[3] == 0.0 and got[2] == h0 + w * Te and got[4] == w and got[5] == a
    assert F[2, 4] == Te == F[3, 5] and F[3, 3] == 1.0
    # the position rows agree: the speed at the stop is 0
    assert np.abs(F[:2] - num[:2]).max() <= 1e-8
    # the heading row lacks the dependence of the stop time on s and a ...
    assert F[2, 3] == 0.0 and abs(num[2, 3] - w / -a) <= 1e-8
    assert F[2, 5] == 0.0 and abs(num[2, 5] - w * s / (a * a)) <= 1e-8
    assert abs(F[2, 4] - num[2, 4]) <= 1e-8
    # ... and the speed row keeps 1 and T_e where the flow has 0
    assert (num[3] == 0.0).all()
    # s0 = max(s, 0): a negative speed estimate flows as a standing obstacle
    neg = np.array([1.0, -2.0, h0, -0.2, w, 0.0])
    got = AM.flow(neg, np.float64(T_JAC))
    assert (got[:3] == neg[:3]).all() and got[3] == 0.0
    assert (AM.transition(neg, np.float64(T_JAC)) == np.eye(6)).all()


# ---------------------------------------------------------------------------
# 3. known answers
# ---------------------------------------------------------------------------
ROW = np.array([0.05, 0.01, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.3, 3.0, 1.0, 6.0, 1e3, 1e3])
LEAD, DT, HP = 0.13, 0.4, 10


def _one(trk, z, T, x, cov, untracked=None, hp=HP, fm=AM.F64):
    return AM.lane_step(np.asarray(trk, float), np.asarray(z, float), fm.num(T), LEAD, DT, hp, x,
                        cov, np.zeros((2, hp)) if untracked is None else untracked, fm)


def test_two_measurements_average():
    z1 = np.array([1.0, -2.0, 0.3, 4.0])
    z2 = z1 + np.array([0.04, -0.03, 0.005, -0.08])
    x, P, nis, ob = _one(ROW, z1, 0.0, np.full(6, np.nan), np.zeros((6, 6)))
    r = AM.r_diag(ROW)
    assert (x == np.append(z1, [0.0, 0.0])).all() and math.isnan(nis)
    assert (P == np.diag(np.append(r, [0.3 ** 2, 3.0 ** 2]))).all()
    # the horizon of the initialised lane is the straight line of the measurement
    assert np.allclose(ob, TM.straight(z1, LEAD, DT, HP), rtol=0, atol=1e-13)
    x, P, nis, ob = _one(ROW, z2, 0.0, x, P)
    want = 0.5 * (z1 + z2)
    assert (np.abs(x[:4] - want) <= 1e-13 * np.maximum(1.0, np.abs(want))).all()
    assert x[4] == 0.0 and P[4, 4] == 0.3 ** 2 and x[5] == 0.0 and P[5, 5] == 3.0 ** 2
    assert (np.abs(np.diag(P)[:4] - r / 2) <= 1e-13 * r / 2).all()
    assert (P - np.diag(np.diag(P)) == 0).all()
    want_nis = ((z2 - z1) ** 2 / (2 * r)).sum()
    assert abs(nis - want_nis) <= 1e-13 * want_nis


def test_two_exact_measurements_of_a_braking_lane_recover_the_acceleration():
    a_true, s, h = -1.5, 4.0, 0.3
    trk = ROW.copy()
    trk[:3] = 1e-3
    x, P = np.full(6, np.nan), np.zeros((6, 6))
    for k in range(2):
        q = MNM.piece((1.0, -2.0, h, s), a_true, 0.0, 0.4 * k)
        x, P, nis, ob = _one(trk, q[:4], 0.0 if k == 0 else 0.4, x, P)
    sigma = math.sqrt(P[5, 5])
    print(f"a = {x[5]:.6f} after two measurements, posterior sigma {sigma:.2e}")
    assert abs(x[5] - a_true) <= sigma < 0.01
    # and the prediction from there follows the braking: 0.1 m after 4 s, where the straight
    # line at the measured speed is 12 m off
    true = np.array([MNM.piece((1.0, -2.0, h, s), a_true, 0.0, 0.4 + (k + 1) * DT + LEAD)[:2]
                     for k in range(HP)]).T
    line = TM.straight(np.asarray(q[:4], float), LEAD, DT, HP)
    assert np.abs(ob - true).max() < 0.1 < 5.0 < np.abs(line - true).max()


@pytest.mark.parametrize("w", [0.0, 0.2])
def test_a_horizon_that_crosses_the_stop_stands_and_never_reverses(w):
    # stops 2 s ahead; W_HOLD = 1: the stop lies in the second piece
    x = np.array([1.0, -2.0, 0.3, 2.0, w, -1.0])
    row = ROW.copy()
    row[AM.W_HOLD] = 1.0
    ob = AM.horizon(x, row, LEAD, DT, HP)
    tau = np.array([(k + 1) * DT + LEAD for k in range(HP)])
    stopped = tau >= 2.0
    assert stopped.sum() >= 5 and (~stopped).sum() >= 4
    first = np.argmax(stopped)
    assert (ob[:, first:] == ob[:, first:first + 1]).all()           # bitwise, from the stop on
    # along the heading of the moment the obstacle never moves backwards
    head = x[2] + w * np.minimum(tau, 1.0)
    step = np.diff(np.concatenate([x[:2, None], ob], axis=1), axis=1)
    along = step[0] * np.cos(head) + step[1] * np.sin(head)
    assert (along >= 0.0).all() and (along[:first] > 0.0).all()
    # the stopping distance s^2 / (2 |a|) = 2 m is not exceeded
    assert np.hypot(ob[0] - x[0], ob[1] - x[1]).max() <= 2.0 + 1e-12
    # a clamp of 0 on the acceleration: the constant-speed prediction, which does not stop
    row0 = row.copy()
    row0[AM.A_CLAMP] = 0.0
    ob0 = AM.horizon(x, row0, LEAD, DT, HP)
    assert np.hypot(ob0[0, -1] - x[0], ob0[1, -1] - x[1]) > 4.0


def test_both_holds_zero_is_the_straight_line_from_the_filtered_pose():
    x = np.array([1.0, -2.0, 0.3, 2.0, 0.4, -1.0])
    row = ROW.copy()
    row[AM.W_HOLD] = row[AM.A_HOLD] = 0.0
    ob = AM.horizon(x, row, LEAD, DT, HP)
    assert np.allclose(ob, TM.straight(x[:4], LEAD, DT, HP), rtol=0, atol=1e-12)
    # a negative speed estimate predicts a standing obstacle
    xn = x.copy()
    xn[3] = -0.3
    assert (AM.horizon(xn, ROW, LEAD, DT, HP) == xn[:2, None]).all()


@pytest.mark.parametrize("w_hold,a_hold", [(2.5, 1.0), (1.0, 2.5), (1.0, 1.0), (0.0, 2.5),
                                           (1.0, 1e3)])
def test_the_three_piece_walk_is_the_manoeuvre_of_the_equivalent_schedule(w_hold, a_hold):
    x = np.array([1.0, -2.0, 0.3, 2.0, 0.4, -0.5])
    row = ROW.copy()
    row[AM.W_HOLD], row[AM.A_HOLD] = w_hold, a_hold
    row[AM.W_CLAMP], row[AM.A_CLAMP] = 0.25, 0.4             # both clamps bite
    ob = AM.horizon(x, row, LEAD, DT, HP)
    wc, ac = 0.25, -0.4
    t1, t2 = min(w_hold, a_hold), max(w_hold, a_hold)
    second = (ac, 0.0) if a_hold > w_hold else (0.0, wc)
    man = np.zeros((4, 3))
    man[0] = (t1, ac, wc)
    man[1] = (t2 - t1, second[0], second[1])
    truth = np.array([1.0, -2.0, 0.3, 2.0, 4.0, 2.0, 0.0])  # a row that does not turn itself
    want = np.array([MNM.state_lane(truth, man, (k + 1) * DT + LEAD)[:2] for k in range(HP)]).T
    assert (ob == want).all()                                # the holds are exact in binary
    assert not np.allclose(ob, AM.horizon(x, ROW, LEAD, DT, HP), atol=1e-3)


# ---------------------------------------------------------------------------
# 4. the reduction to the five-state tracker
# ---------------------------------------------------------------------------
def test_without_an_acceleration_the_mirror_is_the_five_state_mirror():
    B, nO, hp = 12, 22, 10
    rows, osense, trk5, trk6 = TC.reduction_case(B, nO)
    assert (trk6[..., AM.P0_ACCEL] == 0).all() and (trk6[..., AM.Q_ACCEL] == 0).all()
    on = (trk5 != 0).any(axis=2)
    assert (trk6[on][:, (AM.W_HOLD, AM.A_HOLD)] == 1e3).all() and ((trk6 != 0).any(axis=2) == on).all()
    x6, c6 = AM.alloc(B, nO)
    x5, c5 = np.full((B, nO, 5), np.nan), np.zeros((B, nO, 5, 5))
    worst = 0.0
    for s, (t, since) in enumerate(TC.reduction_times()):
        o6, z6, n6 = AM.step(rows, osense, TC.SEED, s, 3, trk6, t, since, TC.LEAD, TC.DT, hp, x6, c6)
        o5, z5, n5 = TM.step(rows, osense, TC.SEED, s, 3, trk5, t, since, TC.LEAD, TC.DT, hp, x5, c5)
        assert np.array_equal(z6, z5, equal_nan=True)
        a = x6[..., 5]
        assert (a[~np.isnan(a)] == 0.0).all()                # the acceleration stays exactly 0
        worst = max(worst, TC.reduction_ratio(x6, c6, n6, o6, x5, c5, n5, o5))
    print(f"six-state mirror with P0_ACCEL = Q_ACCEL = 0 against the five-state mirror: "
          f"{worst:.3e} (RED_TOL {TC.RED_TOL:.3e})")
    assert worst <= TC.RED_TOL


# ---------------------------------------------------------------------------
# 5. rules
# ---------------------------------------------------------------------------
def test_off_bad_and_trouble_rows_of_the_mirror():
    z = np.array([1.0, -2.0, 0.3, 4.0])
    x0, P0 = np.arange(6.0), np.arange(36.0).reshape(6, 6)
    base = np.arange(2.0 * HP).reshape(2, HP)
    assert AM.is_off_row(np.zeros(14)) and not AM.is_bad_row(np.zeros(14))
    assert AM.is_off_row(-np.zeros(14))
    x, P, nis, ob = _one(np.zeros(14), z, 0.4, x0, P0, base)
    assert (x == x0).all() and (P == P0).all() and math.isnan(nis) and (ob == base).all()
    for f, val in ((0, math.nan), (7, math.inf), (1, -1e-3), (13, -1e-300), (11, -1.0), (2, 0.0),
                   (0, 0.0)):
        bad = ROW.copy()
        bad[f] = val
        assert AM.is_bad_row(bad), (f, val)
        x, P, nis, ob = _one(bad, z, 0.4, x0, P0, base)
        assert np.isnan(x).all() and np.isnan(P).all() and math.isnan(nis) and np.isnan(ob).all()
    for f in (AM.P0_YAW, AM.P0_ACCEL, AM.W_CLAMP, AM.A_CLAMP, AM.W_HOLD, AM.A_HOLD, AM.Q_POS,
              AM.Q_ACCEL):
        ok = ROW.copy()
        ok[f] = 0.0
        assert not AM.is_bad_row(ok)
    # a bad measurement (a bad obstacle or osense row) and a covariance without a Cholesky
    x, P, nis, ob = _one(ROW, np.full(4, np.nan), 0.4, x0, np.eye(6))
    assert np.isnan(x).all() and np.isnan(P).all() and np.isnan(ob).all()
    x, P, nis, ob = _one(ROW, z, 0.4, x0, -np.eye(6))
    assert np.isnan(x).all() and np.isnan(P).all() and math.isnan(nis) and np.isnan(ob).all()
    # ... after which the lane initialises itself again
    x, P, nis, ob = _one(ROW, z, 0.4, x, P)
    assert (x == np.append(z, [0.0, 0.0])).all() and math.isnan(nis) and np.isfinite(ob).all()
    # a non-finite estimate is trouble too
    xi = np.append(z, [0.0, 0.0])
    xi[3] = math.inf
    x, P, nis, ob = _one(ROW, z, 0.4, xi, np.eye(6))
    assert np.isnan(x).all() and np.isnan(ob).all()
    # only the upper triangle of cov is read
    Pu = np.diag(np.arange(1.0, 7.0)) * 1e-2
    Pu[0, 4] = 1e-3
    Pl = Pu.copy()
    Pl[4, 0] = 55.0
    xg = np.append(z, [0.1, -0.5])
    a, b = _one(ROW, z + 0.01, 0.4, xg, Pu), _one(ROW, z + 0.01, 0.4, xg, Pl)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert (a[1] == a[1].T).all()


def test_the_long_double_format_runs_the_same_code():
    if np.finfo(LD).eps > 1e-18:
        pytest.fail("numpy's long double is not an 80-bit type on this machine")
    z = np.array([1.0, -2.0, 0.3, 4.0])
    x64, P64 = np.full(6, np.nan), np.zeros((6, 6))
    x80, P80 = AM.F80.array(x64), AM.F80.array(P64)
    for k in range(3):
        zk = z + 0.05 * k
        x64, P64, n64, o64 = _one(ROW, zk, 0.4, x64, P64)
        x80, P80, n80, o80 = _one(ROW, zk, 0.4, x80, P80, fm=AM.F80)
        assert x80.dtype == P80.dtype == o80.dtype == LD and x64.dtype == np.float64
        assert np.abs(x64 - x80.astype(float)).max() < 1e-12
        assert np.abs(o64 - o80.astype(float)).max() < 1e-11
    assert abs(float(n80) - float(n64)) < 1e-9 * float(n64)
    L = AM.cholesky(AM.F80.array([[4, 2], [2, 3]]), AM.F80)
    assert L.dtype == LD and abs(float(L[1, 1]) - math.sqrt(2.0)) < 1e-18 * 4
    assert AM.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]])) is None


# ---------------------------------------------------------------------------
# 6. the tolerance of the GPU tests, from the reference alone
# ---------------------------------------------------------------------------
def test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies():
    if np.finfo(LD).eps > 1e-18:
        pytest.fail("numpy's long double is not an 80-bit type on this machine")
    figures = {}
    seen = dict(stop_in_step=0, stop_in_horizon=0, restart=0, a_zero=0, w_zero=0)
    sides = {k: [0, 0] for k in ("sinc", "dsinc", "pr", "dpr")}
    for B, nO, hp in TC.SHAPES:
        rows, man, osense, trk = TC.case(B, nO)
        r64, r80 = TC.run_mirror(B, nO, hp, AM.F64), TC.run_mirror(B, nO, hp, AM.F80)
        worst = 0.0
        for (s, since), a, b in zip(TC.times(), r64, r80):
            worst = max(worst, TC.ratio([(a[0], b[0]), (a[3], b[3])], a[1], b[1], a[2], b[2]))
            z = a[4]
            assert np.nanmax(np.abs(z[..., :2])) <= 16.0     # the conditioning limit
            # what the steps exercise, from the estimates the predictions started from
            xb = a[5].reshape(-1, 6)
            tr = trk.reshape(-1, 14)
            for g in range(len(xb)):
                if np.isnan(xb[g, 0]) or since == 0.0 or not tr[g].any():
                    continue
                s0, w, acc = max(xb[g, 3], 0.0), xb[g, 4], xb[g, 5]
                stop = AM.stop_time(np.float64(s0), np.float64(acc))
                Te = min(since, stop)
                seen["stop_in_step"] += Te < since
                seen["a_zero"] += acc == 0.0
                seen["w_zero"] += w == 0.0
                th = abs(w * Te)
                for key, lim, val in (("sinc", 1e-4, th / 2), ("dsinc", 0.02, th / 2),
                                      ("pr", 0.1, th), ("dpr", 0.3, th)):
                    if 0.5 * lim <= val < 2.0 * lim:
                        sides[key][int(val >= lim)] += 1
            xa = a[0].reshape(-1, 6)
            ob = a[3].reshape(len(xa), 2, hp)
            for g in range(len(xa)):
                if np.isnan(xa[g, 0]) or hp < 3:
                    continue
                stands = (ob[g, :, 1:] == ob[g, :, :-1]).all(axis=0)
                seen["stop_in_horizon"] += bool(stands[-1] and not stands[0])
        speed = np.array([MNM.state(rows, man, t)[..., OM.SPEED] for t, _ in TC.times()])
        seen["restart"] += int(((speed[:-1] == 0) & (speed[1:] > 0)).any(axis=0).sum())
        figures[(B, nO, hp)] = worst
        on = (trk != 0).any(axis=2)
        assert (on.sum() > 0) and ((~on).sum() > 0 or B * nO < 4)
    print("float64 against 80-bit mirror:", {k: f"{v:.3e}" for k, v in figures.items()})
    print("exercised:", seen, sides)
    assert all(v > 0 for v in seen.values()), seen
    assert all(lo > 0 and hi > 0 for lo, hi in sides.values()), sides
    worst = max(figures.values())
    assert abs(worst - TC.MIRROR_ROUNDING) <= 0.01 * TC.MIRROR_ROUNDING
    assert TC.TOL == TC.pow2_ceil(16.0 * worst) == 2.0 ** -39
    assert TC.RED_TOL == TC.pow2_ceil(16.0 * TC.REDUCTION_MEASURED)


# ---------------------------------------------------------------------------
# 7. consistency and the direction of the inequalities the GPU tests assert
# ---------------------------------------------------------------------------
def test_mirror_is_consistent_and_beats_the_five_state_mirror():
    rows, man, osense, trk, trk5 = TC.consistency_inputs()
    assert TC.no_lane_stops(rows, man)
    B, nO = rows.shape[:2]
    x, cov = AM.alloc(B, nO)
    x5, cov5 = np.full((B, nO, 5), np.nan), np.zeros((B, nO, 5, 5))
    every, every5 = [], []
    for s in range(TC.CONS_STEPS + 1):
        snap = MNM.state(rows, man, s * TC.CONS_T)
        since = 0.0 if s == 0 else TC.CONS_T
        obst, z, nis = AM.step(snap, osense, TC.CONS_SEED, s, 0, trk, 0.0, since, TC.CONS_LEAD,
                               TC.CONS_DT, TC.CONS_HP, x, cov)
        obst5, z5, nis5 = TM.step(snap, osense, TC.CONS_SEED, s, 0, trk5, 0.0, since, TC.CONS_LEAD,
                                  TC.CONS_DT, TC.CONS_HP, x5, cov5)
        assert np.array_equal(z, z5)                         # the same measurements
        assert np.isnan(nis).all() if s == 0 else np.isfinite(nis).all()
        if s:
            every.append(nis)
            every5.append(nis5)
        assert (cov == cov.transpose(0, 1, 3, 2)).all()
    assert np.linalg.eigvalsh(cov.reshape(-1, 6, 6)).min() > 0
    mean, bound, rms, rms5 = TC.consistency_verdict(np.array(every), obst, obst5, rows, man)
    print(f"mean NIS {mean:.3f} (|mean - 4| <= {bound:.3f}; the five-state tracker: "
          f"{float(np.mean(every5)):.1f}); RMS position error {TC.CONS_AHEAD:.1f} s ahead {rms:.4f} m, "
          f"of the five-state tracker {rms5:.4f} m")
    assert np.array(every).size == 18000 and abs(bound - 0.105) < 5e-4
    assert abs(mean - 4.0) <= bound
    assert rms < rms5


def test_against_braking_obstacles_the_prediction_beats_the_five_state_mirrors():
    """The inequality of the frog rollout of the GPU tests, on the mirrors: B = 4, 6 steps,
    every obstacle braking at 3 m/s^2, an exact sensor, `matched` rows; the summed error of
    the prediction against the manoeuvring truth at the predicted times, from step 3 on."""
    from oracle import scp_reference as R
    from scpqp import tracker as TRK
    sc = R.frog_scenario(Hp=10)
    rows, brake = TC.frog_inputs(sc, 4)
    zeros = np.zeros((4, sc.nObst, 3))
    trk6 = TRKA.matched(zeros, device="cpu").numpy()
    trk5 = TRK.matched(zeros, device="cpu").numpy()
    x6, c6 = AM.alloc(4, sc.nObst)
    x5, c5 = np.full((4, sc.nObst, 5), np.nan), np.zeros((4, sc.nObst, 5, 5))
    lead = sc.delay_x + sc.dt + sc.delay_u
    err6 = err5 = 0.0
    g0 = 0
    for i in range(TC.FROG_STEPS):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        t = g1 * sc.tick_length
        snap = MNM.state(rows, brake, t)
        since = (g1 - g0) * sc.tick_length
        g0 = g1
        o6, _, _ = AM.step(snap, None, 0, i, 0, trk6, 0.0, since, lead, sc.dt, sc.Hp, x6, c6)
        o5, _, _ = TM.step(snap, None, 0, i, 0, trk5, 0.0, since, lead, sc.dt, sc.Hp, x5, c5)
        if i >= 3:
            true = np.array([MNM.state(rows, brake, t + (k + 1) * sc.dt + lead)[..., :2]
                             for k in range(sc.Hp)]).transpose(1, 2, 3, 0)
            err6 += float(np.hypot(*(o6 - true).transpose(2, 0, 1, 3)).sum())
            err5 += float(np.hypot(*(o5 - true).transpose(2, 0, 1, 3)).sum())
    print(f"summed prediction error from step 3 on: {err6:.3f} m with the acceleration state, "
          f"{err5:.3f} m without, ratio {err6 / err5:.3e}")
    assert err6 < err5


# ---------------------------------------------------------------------------
# 8. scpqp.tracker_accel's host side
# ---------------------------------------------------------------------------
def test_validate_names_the_row_and_the_field():
    good = TRKA.rows(3, 2, device="cpu").numpy()
    TRKA.validate(good)
    TRKA.validate(np.zeros((3, 2, 14)))
    assert TRKA.is_off(np.zeros((3, 2, 14))) and not TRKA.is_off(good)
    for (b, o, f), val, what in (((2, 1, 4), math.nan, "q_heading is not finite"),
                                 ((0, 1, 0), math.inf, "r_pos is not finite"),
                                 ((1, 0, 7), -1e-9, "q_accel must be >= 0"),
                                 ((1, 1, 11), -1.0, "a_clamp must be >= 0"),
                                 ((0, 0, 13), -0.5, "a_hold must be >= 0"),
                                 ((2, 0, 2), 0.0, "r_speed must be > 0")):
        bad = good.copy()
        bad[b, o, f] = val
        with pytest.raises(ValueError, match=rf"rows\[{b}, {o}\]: {what}"):
            TRKA.validate(bad)
        with pytest.raises(ValueError):
            TRKA.validate(torch.as_tensor(bad))
        assert AM.is_bad_row(bad[b, o])
    legal = good.copy()
    legal[..., 8:] = 0.0                    # zeros in P0_*, *_CLAMP and *_HOLD are legal
    TRKA.validate(legal)
    for shape in ((3, 2, 9), (3, 14), (3, 2, 14, 1)):
        with pytest.raises(ValueError, match="rows must be"):
            TRKA.validate(np.zeros(shape))


def test_rows_broadcast_matched_and_from_table():
    r = TRKA.rows(4, 3, r_pos=np.array([[0.01], [0.02], [0.05], [0.1]]), q_accel=0.0, a_hold=0.0,
                  device="cpu")
    assert tuple(r.shape) == (4, 3, 14) and r.dtype == torch.float64
    assert r[:, :, 0].tolist() == [[0.01] * 3, [0.02] * 3, [0.05] * 3, [0.1] * 3]
    assert (r[..., 7] == 0).all() and (r[..., 13] == 0).all() and (r[..., 1] == 0.01).all()
    d = TRKA.rows(1, 1, device="cpu")[0, 0].tolist()
    assert d[7:] == [1.0, 0.5, 3.0, 1.0, 6.0, 1e3, 1e3]     # the choices of the docstring
    assert "choices, not tunings" in TRKA.__doc__
    with pytest.raises(ValueError, match="r_speed does not broadcast"):
        TRKA.rows(4, 3, r_speed=np.ones(5), device="cpu")
    with pytest.raises(ValueError, match=r"rows\[0, 0\]: r_pos must be > 0"):
        TRKA.rows(4, 3, r_pos=0.0, device="cpu")
    table = torch.stack([TRKA.rows(1, 3, r_pos=s, device="cpu")[0] for s in (0.01, 0.1)])
    got = TRKA.from_table(table, [1, 0, 1], device="cpu")
    assert got[:, 0, 0].tolist() == [0.1, 0.01, 0.1]
    with pytest.raises(ValueError, match="outside the table"):
        TRKA.from_table(table, [2], device="cpu")
    with pytest.raises(ValueError, match="rows must be"):
        TRKA.from_table(torch.zeros((2, 3, 9)), [0], device="cpu")
    off = TRKA.off(2, 3, device="cpu")
    assert TRKA.is_off(off) and tuple(off.shape) == (2, 3, 14)
    x, cov = TRKA.alloc(2, 3, device="cpu")
    assert torch.isnan(x).all() and tuple(x.shape) == (2, 3, 6)
    assert (cov == 0).all() and tuple(cov.shape) == (2, 3, 6, 6)
    # matched: an exact sensor still gives a legal row
    s = np.zeros((2, 3, 3))
    s[0, :, 0] = 0.05
    s[1, :, 1] = 1e-5
    m = TRKA.matched(s, floor=(1e-3, 2e-3, 3e-3), q=(0.1, 0.2, 0.3, 0.4, 0.5), p0_yaw=0.7,
                     p0_accel=0.8, w_clamp=0.9, a_clamp=1.1, w_hold=1.2, a_hold=1.3,
                     device="cpu").numpy()
    assert (m[0, :, 0] == 0.05).all() and (m[1, :, 0] == 1e-3).all()
    assert (m[..., 1] == 2e-3).all() and (m[..., 2] == 3e-3).all()
    assert (m[..., 3:] == np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 0.8, 0.9, 1.1, 1.2, 1.3])).all()
    d = TRKA.matched(torch.zeros((2, 3, 3), dtype=torch.float64)).numpy()
    assert (d[..., :3] == np.array(TRKA.FLOOR)).all() and (d[..., 3:8] == np.array(TRKA.Q_DEFAULT)).all()
    with pytest.raises(ValueError, match="floor"):
        TRKA.matched(s, floor=(0.0, 1e-3, 1e-3), device="cpu")
    with pytest.raises(ValueError, match="q five"):
        TRKA.matched(s, q=(0.1, 0.2, 0.3, 0.4), device="cpu")
    with pytest.raises(ValueError, match="obstacle sensing rows"):
        TRKA.matched(np.zeros((2, 3, 8)), device="cpu")


def test_step_refuses_host_tensors():
    B, nO = 2, 3
    trk = TRKA.rows(B, nO, device="cpu")
    x, cov = TRKA.alloc(B, nO, device="cpu")
    rows = torch.zeros((B, nO, 7), dtype=torch.float64)
    with pytest.raises(ValueError, match="rows must be .* on the GPU"):
        TRKA.step(rows, None, 0, 0, 0, trk, 0.0, 0.0, 0.1, 0.4, 5, x, cov)
