"""Obstacle tracker, the parts that need no GPU: the C-ABI of include/scpqp_tracker.h
(exports, constants by a gcc probe of the header, argument validation without touching a
device), the CPU mirror's anchors and known answers (tests/tracker_mirror.py) and
scpqp.tracker's host side.

Bounds.  The Jacobian against central differences of the mirror's flow: 1e-8 absolute on
entries of order c = s T <= 2 (the step 1e-5 leaves a truncation error of h^2 / 6 times a third
derivative of order one, 2e-11, and a rounding error of ulp(30) / h = 4e-10; a run shows 2e-10).
The two branches of g' against an 80-bit evaluation next to the switch: 1e-11 relative (the
series' next term is 4e-15 relative there, the closed form cancels to ulp / a^2 = 3e-13).  The
known answers of a diagonal problem: 1e-13 relative, a few dozen roundings of 2^-53 with no
transcendental involved.  The consistency bound is the mirror's own (``consistency_verdict``):
five standard deviations of the mean of 18000 chi-square(4) variables, 0.105."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import obstacle_mirror as OM
import tracker_mirror as TM
from scpqp import _lib as LB
from scpqp import tracker as TRK
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_tracker.h")
E_ARG, E_SIZE = -1, -4


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
def test_tracker_header_declares_the_boundary():
    assert header_functions() == sorted(LB.TRK_EXPORTS) == ["scpqp_obstacles_track"]
    others = (set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
              | set(LB.VARIANT_EXPORTS) | set(LB.TRUTH_EXPORTS) | set(LB.OBSTACLE_EXPORTS)
              | set(LB.SENSE_EXPORTS) | set(LB.EST_EXPORTS))
    assert not set(LB.TRK_EXPORTS) & others
    txt = open(HEADER).read()
    for word in ("W_CLAMP", "P0_YAW", "not wrapped", "Off row", "Bad row", "0.02",
                 "No new Philox site"):
        assert word in txt, word


def test_library_exports_the_tracker_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.TRK_EXPORTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_tracker.h"
int main(void) {
  printf("ns %d\n", SCPQP_TRK_NS);
  printf("nz %d\n", SCPQP_TRK_NZ);
  printf("np %d\n", SCPQP_TRK_NP);
  printf("idx %d%d%d%d%d%d%d%d%d\n", SCPQP_TRK_R_POS, SCPQP_TRK_R_HEADING, SCPQP_TRK_R_SPEED,
         SCPQP_TRK_Q_POS, SCPQP_TRK_Q_HEADING, SCPQP_TRK_Q_SPEED, SCPQP_TRK_Q_YAW,
         SCPQP_TRK_P0_YAW, SCPQP_TRK_W_CLAMP);
  printf("switch %.17g\n", SCPQP_TRK_DSINC_SWITCH);
  printf("maxobst %d\n", SCPQP_MAX_OBST);
  printf("ssize %zu\n", sizeof(scpqp_sense_stream));
  return 0;
}
"""


def test_tracker_ctypes_layout_matches_header(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["ns"]) == LB.TRK_NS == TM.NS == TRK.NS == 5
    assert int(got["nz"]) == LB.TRK_NZ == TM.NZ == TRK.NZ == 4
    assert int(got["np"]) == LB.TRK_NP == TM.NP == TRK.NP == 9
    assert got["idx"] == "012345678"
    assert (LB.TRK_R_POS, LB.TRK_R_HEADING, LB.TRK_R_SPEED, LB.TRK_Q_POS, LB.TRK_Q_HEADING,
            LB.TRK_Q_SPEED, LB.TRK_Q_YAW, LB.TRK_P0_YAW, LB.TRK_W_CLAMP) == tuple(range(9)) \
        == (TM.R_POS, TM.R_HEADING, TM.R_SPEED, TM.Q_POS, TM.Q_HEADING, TM.Q_SPEED, TM.Q_YAW,
            TM.P0_YAW, TM.W_CLAMP)
    assert float(got["switch"]) == LB.TRK_DSINC_SWITCH == TM.DSINC_SWITCH == 0.02
    assert TRK.FIELDS == LB.TRK_FIELDS and len(TRK.FIELDS) == 9
    assert int(got["maxobst"]) == LB.MAX_OBST
    assert int(got["ssize"]) == C.sizeof(LB.SenseStream)
    # the declared argument list: 17 arguments, in the header's order
    proto = re.search(r"int scpqp_obstacles_track\((.*?)\);", open(HEADER).read(), re.S).group(1)
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    assert len(args) == len(lib.scpqp_obstacles_track.argtypes) == 17
    for a, t in zip(args, lib.scpqp_obstacles_track.argtypes):
        if a.startswith("double "):
            assert t is C.c_double, a
        elif a.startswith("int32_t "):
            assert t is C.c_int32, a
        else:
            assert "*" in a and t in (C.c_void_p, C.POINTER(LB.SenseStream)), a


def test_track_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    D = C.cast(buf, C.c_void_p)
    ST = LB.SenseStream(seed=1, epoch=0, b_offset=0)

    def err():
        return lib.scpqp_last_error()

    def track(B=0, n_obst=3, hp=5, rows=None, osense=None, st=None, trk=None, t_meas=0.0,
              t_since=0.4, lead=0.1, dt=0.4, x=None, cov=None, z=None, nis=None, out=None):
        return lib.scpqp_obstacles_track(B, n_obst, hp, rows, osense,
                                         None if st is None else C.byref(st), trk, t_meas, t_since,
                                         lead, dt, x, cov, z, nis, out, None)

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
    # sizes before the pointers: nothing is launched for a size error
    assert track(B=1 << 27, n_obst=1, **full) == E_SIZE and b"25" in err()
    assert track(B=1 << 27, n_obst=1) == E_SIZE
    assert track(B=1 << 22, n_obst=4, hp=64, osense=D, st=ST, **full) == E_SIZE and b"hp" in err()


# ---------------------------------------------------------------------------
# 2. mirror anchors: the Jacobian and g'
# ---------------------------------------------------------------------------
T_JAC = 0.4
W_JAC = [0.0, 1e-9, 1e-3, 0.019 * 2 / T_JAC, 0.021 * 2 / T_JAC, 0.3, -1.2, 3.0]


@pytest.mark.parametrize("w", W_JAC)
def test_jacobian_against_central_differences_of_the_flow(w):
    worst = 0.0
    for h0, s in ((0.3, 4.0), (-2.5, 1.5), (1.2, 0.0)):
        x = np.array([1.0, -2.0, h0, s, w])
        F = TM.transition(x, T_JAC)
        num = np.empty((5, 5))
        for j in range(5):
            d = np.zeros(5)
            d[j] = 1e-5
            num[:, j] = (TM.flow(x + d, T_JAC) - TM.flow(x - d, T_JAC)) / 2e-5
        worst = max(worst, float(np.abs(F - num).max()))
        # seven off-diagonal nonzeros on a unit diagonal
        off = F - np.eye(5)
        mask = np.zeros((5, 5), bool)
        for r, c in ((0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4), (2, 4)):
            mask[r, c] = True
        assert (off[~mask] == 0.0).all()
    print(f"w = {w}: largest |F - central difference| {worst:.2e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("factor", [0.999, 1.001])
def test_both_dsinc_branches_against_long_double_at_the_switch(factor):
    if np.finfo(np.longdouble).eps > 1e-18:
        pytest.fail("numpy's long double is not an 80-bit type on this machine")
    for sign in (1.0, -1.0):
        a = sign * factor * TM.DSINC_SWITCH
        al = np.longdouble(a)
        want = (al * np.cos(al) - np.sin(al)) / (al * al)
        for got in (TM.dsinc_series(a), TM.dsinc_closed(a), TM.dsinc(a)):
            assert abs(float((np.longdouble(got) - want) / want)) <= 1e-11
    assert TM.dsinc(0.0) == 0.0
    assert TM.dsinc(0.999 * TM.DSINC_SWITCH) == TM.dsinc_series(0.999 * TM.DSINC_SWITCH)
    assert TM.dsinc(TM.DSINC_SWITCH) == TM.dsinc_closed(TM.DSINC_SWITCH)


# ---------------------------------------------------------------------------
# 3. known answers
# ---------------------------------------------------------------------------
ROW = np.array([0.05, 0.01, 0.1, 0.0, 0.0, 0.0, 0.0, 0.3, 1.0])
LEAD, DT, HP = 0.1, 0.4, 5


def _one(trk, z, T, x, cov, untracked=None):
    return TM.lane_step(np.asarray(trk, float), np.asarray(z, float), T, LEAD, DT, HP, x, cov,
                        np.zeros((2, HP)) if untracked is None else untracked)


def test_two_measurements_average():
    z1 = np.array([1.0, -2.0, 0.3, 4.0])
    z2 = z1 + np.array([0.04, -0.03, 0.005, -0.08])
    x, P, nis, ob = _one(ROW, z1, 0.0, np.full(5, np.nan), np.zeros((5, 5)))
    r = TM.r_diag(ROW)
    assert (x == np.append(z1, 0.0)).all() and math.isnan(nis)
    assert (P == np.diag(np.append(r, 0.3 ** 2))).all()
    # the horizon of the initialised lane is the straight line of the measurement
    assert np.allclose(ob, TM.straight(z1, LEAD, DT, HP), rtol=0, atol=1e-13)
    x, P, nis, ob = _one(ROW, z2, 0.0, x, P)
    want = 0.5 * (z1 + z2)
    assert (np.abs(x[:4] - want) <= 1e-13 * np.maximum(1.0, np.abs(want))).all()
    assert x[4] == 0.0 and P[4, 4] == 0.3 ** 2            # the turn rate and its variance stay
    assert (np.abs(np.diag(P)[:4] - r / 2) <= 1e-13 * r / 2).all()
    assert (P - np.diag(np.diag(P)) == 0).all()
    want_nis = ((z2 - z1) ** 2 / (2 * r)).sum()
    assert abs(nis - want_nis) <= 1e-13 * want_nis


def test_the_turn_rate_is_learnt_from_the_heading():
    row = np.array([1.0, -2.0, 0.3, 4.0, 4.0, 2.0, 0.25])
    trk = ROW.copy()
    trk[:3] = 1e-3
    x, P = np.full(5, np.nan), np.zeros((5, 5))
    for s in range(4):
        px, py, ph = OM.pose(row, s * 0.4)
        x, P, nis, ob = _one(trk, [px, py, ph, 4.0], 0.0 if s == 0 else 0.4, x, P)
    assert abs(x[4] - 0.25) < 1e-3
    true = np.array([OM.pose(row, 3 * 0.4 + (k + 1) * DT + LEAD)[:2] for k in range(HP)]).T
    line = TM.straight([px, py, ph, 4.0], LEAD, DT, HP)
    assert np.abs(ob - true).max() < 0.02 < np.abs(line - true).max()
    # W_CLAMP = 0: a straight prediction from the filtered pose
    trk0 = trk.copy()
    trk0[TM.W_CLAMP] = 0.0
    ob0 = TM.horizon(x, 0.0, LEAD, DT, HP)
    assert np.allclose(ob0, TM.straight(x[:4], LEAD, DT, HP), rtol=0, atol=1e-12)
    # and a clamp below the estimate is used as it is
    assert np.array_equal(TM.horizon(x, 0.1, LEAD, DT, HP),
                          TM.horizon(np.append(x[:4], 0.1), 10.0, LEAD, DT, HP))


def test_off_bad_and_trouble_rows_of_the_mirror():
    z = np.array([1.0, -2.0, 0.3, 4.0])
    x0, P0 = np.arange(5.0), np.arange(25.0).reshape(5, 5)
    base = np.arange(2.0 * HP).reshape(2, HP)
    assert TM.is_off_row(np.zeros(9)) and not TM.is_bad_row(np.zeros(9))
    assert TM.is_off_row(-np.zeros(9))
    x, P, nis, ob = _one(np.zeros(9), z, 0.4, x0, P0, base)
    assert (x == x0).all() and (P == P0).all() and math.isnan(nis) and (ob == base).all()
    for f, val in ((0, math.nan), (6, math.inf), (1, -1e-3), (8, -1e-300), (2, 0.0), (0, 0.0)):
        bad = ROW.copy()
        bad[f] = val
        assert TM.is_bad_row(bad), (f, val)
        x, P, nis, ob = _one(bad, z, 0.4, x0, P0, base)
        assert np.isnan(x).all() and np.isnan(P).all() and math.isnan(nis) and np.isnan(ob).all()
    for f in (TM.P0_YAW, TM.W_CLAMP, TM.Q_POS, TM.Q_YAW):
        ok = ROW.copy()
        ok[f] = 0.0
        assert not TM.is_bad_row(ok)
    # a bad measurement (a bad obstacle or osense row) and a covariance without a Cholesky
    x, P, nis, ob = _one(ROW, np.full(4, np.nan), 0.4, x0, np.eye(5))
    assert np.isnan(x).all() and np.isnan(P).all() and np.isnan(ob).all()
    x, P, nis, ob = _one(ROW, z, 0.4, x0, -np.eye(5))
    assert np.isnan(x).all() and np.isnan(P).all() and math.isnan(nis) and np.isnan(ob).all()
    # ... after which the lane initialises itself again
    x, P, nis, ob = _one(ROW, z, 0.4, x, P)
    assert (x == np.append(z, 0.0)).all() and math.isnan(nis) and np.isfinite(ob).all()
    # the measurement of a bad obstacle row or a bad osense row is NaN
    good = np.array([1.0, -2.0, 0.3, 4.0, 4.0, 2.0, 0.1])
    assert np.isfinite(TM.measurement(good, np.array([0.1, 0.0, 0.0]), 1, 0, 0, 0, 0.4)).all()
    assert np.isnan(TM.measurement(good, np.array([-0.1, 0.0, 0.0]), 1, 0, 0, 0, 0.4)).all()
    bad_ob = good.copy()
    bad_ob[OM.LENGTH] = -1.0
    assert np.isnan(TM.measurement(bad_ob, None, 1, 0, 0, 0, 0.4)).all()
    # the exact sensor draws nothing: NULL and an all-zero row are the same
    assert np.array_equal(TM.measurement(good, None, 1, 0, 0, 0, 0.4),
                          TM.measurement(good, np.zeros(3), 7, 3, 2, 5, 0.4))


# ---------------------------------------------------------------------------
# 4. consistency (mirror alone): the condition the GPU statistical test also uses
# ---------------------------------------------------------------------------
def test_mirror_is_consistent_on_the_statistical_inputs():
    rows, osense, trk = TM.consistency_inputs()
    B, nO = rows.shape[:2]
    x, cov = np.full((B, nO, 5), np.nan), np.zeros((B, nO, 5, 5))
    every = []
    for s in range(TM.CONS_STEPS + 1):
        obst, z, nis = TM.step(rows, osense, TM.CONS_SEED, s, 0, trk, s * TM.CONS_T,
                               0.0 if s == 0 else TM.CONS_T, TM.CONS_LEAD, TM.CONS_DT, TM.CONS_HP,
                               x, cov)
        assert np.isnan(nis).all() if s == 0 else np.isfinite(nis).all()
        if s:
            every.append(nis)
        assert (cov == cov.transpose(0, 1, 3, 2)).all()
        assert np.linalg.eigvalsh(cov.reshape(-1, 5, 5)).min() > 0
    mean, bound, rms_trk, rms_line = TM.consistency_verdict(
        np.array(every), obst, z, rows, TM.CONS_STEPS * TM.CONS_T)
    print(f"mean NIS {mean:.3f} (|mean - 4| <= {bound:.3f}); RMS error 2.5 s ahead {rms_trk:.4f} m "
          f"of the tracked prediction, {rms_line:.4f} m of the straight extrapolation")
    assert np.array(every).size == 18000 and abs(bound - 0.105) < 5e-4
    assert abs(mean - 4.0) <= bound
    assert rms_trk < rms_line


# ---------------------------------------------------------------------------
# 5. scpqp.tracker's host side
# ---------------------------------------------------------------------------
def test_validate_names_the_row_and_the_field():
    good = TRK.rows(3, 2, device="cpu").numpy()
    TRK.validate(good)
    TRK.validate(np.zeros((3, 2, 9)))
    assert TRK.is_off(np.zeros((3, 2, 9))) and not TRK.is_off(good)
    for (b, o, f), val, what in (((2, 1, 4), math.nan, "q_heading is not finite"),
                                 ((0, 1, 0), math.inf, "r_pos is not finite"),
                                 ((1, 0, 6), -1e-9, "q_yaw must be >= 0"),
                                 ((1, 1, 8), -1.0, "w_clamp must be >= 0"),
                                 ((2, 0, 2), 0.0, "r_speed must be > 0")):
        bad = good.copy()
        bad[b, o, f] = val
        with pytest.raises(ValueError, match=rf"rows\[{b}, {o}\]: {what}"):
            TRK.validate(bad)
        with pytest.raises(ValueError):
            TRK.validate(torch.as_tensor(bad))
        assert TM.is_bad_row(bad[b, o])
    legal = good.copy()
    legal[..., 7] = legal[..., 8] = 0.0                    # P0_YAW = 0 and W_CLAMP = 0 are legal
    TRK.validate(legal)
    for shape in ((3, 2, 8), (3, 9), (3, 2, 9, 1)):
        with pytest.raises(ValueError, match="rows must be"):
            TRK.validate(np.zeros(shape))


def test_rows_broadcast_matched_and_from_table():
    r = TRK.rows(4, 3, r_pos=np.array([[0.01], [0.02], [0.05], [0.1]]), q_yaw=0.0, w_clamp=0.0,
                 device="cpu")
    assert tuple(r.shape) == (4, 3, 9) and r.dtype == torch.float64
    assert r[:, :, 0].tolist() == [[0.01] * 3, [0.02] * 3, [0.05] * 3, [0.1] * 3]
    assert (r[..., 6] == 0).all() and (r[..., 8] == 0).all() and (r[..., 1] == 0.01).all()
    with pytest.raises(ValueError, match="r_speed does not broadcast"):
        TRK.rows(4, 3, r_speed=np.ones(5), device="cpu")
    with pytest.raises(ValueError, match=r"rows\[0, 0\]: r_pos must be > 0"):
        TRK.rows(4, 3, r_pos=0.0, device="cpu")
    table = torch.stack([TRK.rows(1, 3, r_pos=s, device="cpu")[0] for s in (0.01, 0.1)])
    got = TRK.from_table(table, [1, 0, 1], device="cpu")
    assert got[:, 0, 0].tolist() == [0.1, 0.01, 0.1]
    with pytest.raises(ValueError, match="outside the table"):
        TRK.from_table(table, [2], device="cpu")
    off = TRK.off(2, 3, device="cpu")
    assert TRK.is_off(off) and tuple(off.shape) == (2, 3, 9)
    x, cov = TRK.alloc(2, 3, device="cpu")
    assert torch.isnan(x).all() and tuple(x.shape) == (2, 3, 5)
    assert (cov == 0).all() and tuple(cov.shape) == (2, 3, 5, 5)
    # matched: an exact sensor still gives a legal row
    s = np.zeros((2, 3, 3))
    s[0, :, 0] = 0.05
    s[1, :, 1] = 1e-5
    m = TRK.matched(s, floor=(1e-3, 2e-3, 3e-3), q=(0.1, 0.2, 0.3, 0.4), p0_yaw=0.7, w_clamp=0.9,
                    device="cpu").numpy()
    assert (m[0, :, 0] == 0.05).all() and (m[1, :, 0] == 1e-3).all()
    assert (m[..., 1] == 2e-3).all() and (m[..., 2] == 3e-3).all()
    assert (m[..., 3:] == np.array([0.1, 0.2, 0.3, 0.4, 0.7, 0.9])).all()
    d = TRK.matched(torch.zeros((2, 3, 3), dtype=torch.float64)).numpy()
    assert (d[..., :3] == np.array(TRK.FLOOR)).all() and (d[..., 3:7] == np.array(TRK.Q_DEFAULT)).all()
    with pytest.raises(ValueError, match="floor"):
        TRK.matched(s, floor=(0.0, 1e-3, 1e-3), device="cpu")
    with pytest.raises(ValueError, match="obstacle sensing rows"):
        TRK.matched(np.zeros((2, 3, 8)), device="cpu")


def test_step_refuses_host_tensors():
    B, nO = 2, 3
    trk = TRK.rows(B, nO, device="cpu")
    x, cov = TRK.alloc(B, nO, device="cpu")
    rows = torch.zeros((B, nO, 7), dtype=torch.float64)
    with pytest.raises(ValueError, match="rows must be .* on the GPU"):
        TRK.step(rows, None, 0, 0, 0, trk, 0.0, 0.0, 0.1, 0.4, 5, x, cov)
