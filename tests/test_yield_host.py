"""Right of way and graded braking without a GPU (include/scpqp_yield.h):

1. the boundary: the header's constants and its one function (a gcc probe of the header), the
   export, the ctypes binding, argument validation before any HIP call;
2. the mirror (tests/yield_mirror.py): against its 80-bit self, known answers, the off row and
   every kind of bad row, and the bitwise reduction to ``governor_mirror``;
3. two properties of the definition, over the table and a seeded random batch;
4. the case table (tests/yield_cases.py): its conditions with none left out, what it covers,
   the derivation of the GPU tolerance, and the geometry of the crossing scene;
5. the Python side: ``validate``, ``rows`` and ``from_governor``.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import governor_cases as GC
import governor_mirror as GM
import yield_cases as YC
import yield_mirror as YM
from scpqp import _lib as LB
from scpqp import governor as GOV
from scpqp import yielding as YLD
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "scpqp_yield.h")
E_ARG, E_SIZE = -1, -4
INF = math.inf
TH, TB = YC.T_HOLD, YC.T_BACK


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


# ---------------------------------------------------------------------------
# 1. boundary
# ---------------------------------------------------------------------------
PROBE = r"""
#include <stdio.h>
#include "scpqp_yield.h"
/* the prototype, restated: a mismatch with the header's is a compile error */
int scpqp_yield_step(int32_t n_veh, int32_t n_obst, int32_t hp_max, int32_t B, double t_hold,
                     double t_back, const double* x0, const double* traj, const double* obst,
                     const double* obst_margin, const int32_t* hp, const double* dreq_obs,
                     const double* dreq_veh, const double* yld, double* a_cmd, int32_t* k_conf,
                     int32_t* k_any, int32_t* who, double* clear, double* d_stop, void* stream);
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", SCPQP_YLD_NP, SCPQP_GOV_V_REF,
         SCPQP_GOV_A_ACC, SCPQP_GOV_A_BRAKE, SCPQP_GOV_K_V, SCPQP_GOV_J_MAX, SCPQP_GOV_LOOK,
         SCPQP_GOV_BAND, SCPQP_YLD_PRIO, SCPQP_YLD_A_EASE, SCPQP_YLD_S_STAND, SCPQP_YLD_PRIO_MAX,
         SCPQP_MAX_VEH);
  return 0;
}
"""


def test_header_constants_and_ctypes_layout(tmp_path, lib):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{INCLUDE}", str(src), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == [LB.YLD_NP, LB.GOV_V_REF, LB.GOV_A_ACC, LB.GOV_A_BRAKE, LB.GOV_K_V, LB.GOV_J_MAX,
                   LB.GOV_LOOK, LB.GOV_BAND, LB.YLD_PRIO, LB.YLD_A_EASE, LB.YLD_S_STAND,
                   LB.YLD_PRIO_MAX, LB.MAX_VEH] == [10, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 2 ** 20, 16]
    assert (YM.NP, YM.V_REF, YM.A_ACC, YM.A_BRAKE, YM.K_V, YM.J_MAX, YM.LOOK, YM.BAND, YM.PRIO,
            YM.A_EASE, YM.S_STAND, YM.PRIO_MAX) == tuple(got[:12])
    assert len(LB.YLD_FIELDS) == YLD.NP == 10 and LB.YLD_FIELDS[:7] == LB.GOV_FIELDS
    I, D, V = C.c_int32, C.c_double, C.c_void_p
    assert lib.scpqp_yield_step.argtypes == [I] * 4 + [D] * 2 + [V] * 15
    assert lib.scpqp_yield_step.restype is C.c_int
    assert YLD.required is GOV.required


def test_header_declares_the_boundary_and_the_definition():
    txt = open(HEADER).read()
    assert sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M))) == sorted(LB.YLD_EXPORTS) \
        == ["scpqp_yield_step"]
    txt = " ".join(txt.replace("\n *", " ").split())        # the comment as running text
    for word in ("PRIO", "A_EASE", "S_STAND", "the larger rank has right of way", "Who counts",
                 "never yields, so it is yielded to", "PRIO_v > PRIO_w",
                 "a speed that is not a number stands", "k_any", "who is the smallest j",
                 "counts whatever the ranks", "p_v(-1) = (x0[0], x0[1])",
                 "a_need = max(s, 0)^2 / (2 d_stop)", "-min(A_BRAKE, max(A_EASE, a_need))",
                 "d_stop = +inf", "Off row", "bit for bit", "Bad lane", "k_conf = k_any = who = -2",
                 "A_EASE > A_BRAKE", "What it does not know", "static", "no first-come rule",
                 "negotiation", "not told to hurry", "no hysteresis", "not to the conflict itself",
                 "footprints", "time to collision", "no rows per variant", "SCPQP_E_SIZE",
                 "validated on the", "B = 0 is a no-op"):
        assert word in txt, word


def test_library_exports_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert set(LB.YLD_EXPORTS) <= set(re.findall(r"\sT\s(scpqp_\w+)", out))


def test_argument_validation_without_gpu(lib):
    buf = (C.c_double * 256)()
    P = C.cast(buf, C.c_void_p)

    def err():
        return lib.scpqp_last_error()

    def call(n_veh=2, n_obst=1, hp_max=10, B=0, t_hold=0.4, t_back=0.03, x0=None, traj=None,
             obst=None, margin=None, hp=None, dreq_obs=None, dreq_veh=None, yld=None, a_cmd=None):
        return lib.scpqp_yield_step(n_veh, n_obst, hp_max, B, t_hold, t_back, x0, traj, obst,
                                    margin, hp, dreq_obs, dreq_veh, yld, a_cmd, None, None, None,
                                    None, None, None)

    assert call() == 0                                       # B = 0: a no-op, NULL arrays
    assert call(n_obst=0, t_back=0.0) == 0
    assert call(B=-1) == E_ARG and b"batch" in err()
    for n in (0, -1, LB.MAX_VEH + 1):
        assert call(n_veh=n) == E_ARG and b"n_veh" in err()
    for n in (-1, LB.MAX_OBST + 1):
        assert call(n_obst=n) == E_ARG and b"n_obst" in err()
    for h in (0, -1, LB.MAX_HP + 1):
        assert call(hp_max=h) == E_ARG and b"hp_max" in err()
    for v in (0.0, -0.4, math.nan, INF):
        assert call(t_hold=v) == E_ARG and b"t_hold" in err()
    for v in (-1e-9, math.nan, INF):
        assert call(t_back=v) == E_ARG and b"t_back" in err()
    full = dict(x0=P, traj=P, obst=P, dreq_obs=P, dreq_veh=P, yld=P, a_cmd=P)
    for missing, word in (("x0", b"x0"), ("traj", b"traj"), ("obst", b"null obst"),
                          ("dreq_obs", b"dreq_obs"), ("dreq_veh", b"dreq_veh"), ("yld", b"yld"),
                          ("a_cmd", b"a_cmd")):
        kw = dict(full)
        kw[missing] = None
        assert call(B=3, **kw) == E_ARG and word in err(), missing
    # sizes before the pointers: nothing is launched for a size error
    assert call(n_veh=16, hp_max=64, B=1 << 21, **full) == E_SIZE and b"n_veh * 2 * hp_max" in err()
    assert call(n_veh=1, n_obst=32, hp_max=64, B=1 << 20) == E_SIZE and b"n_obst" in err()
    assert call(n_veh=16, n_obst=0, hp_max=1, B=1 << 24, **full) == E_SIZE and b"row width" in err()
    # the row is ten wide: one vehicle, no obstacle, B * 10 past int32
    assert call(n_veh=1, n_obst=0, hp_max=1, B=215_000_000, **full) == E_SIZE and b"row width" in err()


# ---------------------------------------------------------------------------
# 2. the mirror
# ---------------------------------------------------------------------------
def row(v_ref=4.0, a_acc=1.5, a_brake=3.0, k_v=0.8, j_max=INF, look=6, band=0.25, prio=0,
        a_ease=None, s_stand=0.0):
    return np.array([v_ref, a_acc, a_brake, k_v, j_max, look, band, prio,
                     a_brake if a_ease is None else a_ease, s_stand], float)


def crossing(at=3, hb=6):
    """Two vehicles at 1.6 m a step: vehicle 0 along y = 0 from x = 0, vehicle 1 along x =
    1.6 (at + 1) from below, so that both plans hold the same point at step ``at``.  The
    required distance is 2 m.  -> (x0 [2, 6] at 4 m/s, traj [hb, 2, 2], dreq_veh [2, 2])."""
    k = np.arange(hb) + 1.0
    traj = np.zeros((hb, 2, 2))
    traj[:, 0, 0] = 1.6 * k
    traj[:, 0, 1] = 1.6 * (at + 1)
    traj[:, 1, 1] = 1.6 * (k - at - 1)
    x0 = np.zeros((2, 6))
    x0[1, 0:2] = (1.6 * (at + 1), -1.6 * (at + 1))
    x0[:, 3] = 4.0
    return x0, traj, np.full((2, 2), 2.0)


def run(rows, x0, traj, dv, v, fm=YM.F64, obst=None, do=None, hb=None, detail=None):
    return YM.lane(np.asarray(rows), x0, v, traj.shape[0] if hb is None else hb, traj, obst, None,
                   do, dv[v], TH, TB, fm, detail)


@pytest.mark.parametrize("cid", YC.IDS)
def test_mirror_against_its_eighty_bit_self(cid):
    a, b = YC.mirror(cid, YM.F64), YC.mirror(cid, YM.F80)
    assert b[0].dtype == np.longdouble and np.finfo(np.longdouble).eps < 2e-19
    for i in (1, 3, 4):                                      # k_conf, k_any, who: the same branches
        assert np.array_equal(a[i], b[i]), i
    assert YC.ratio(a, b, cid) <= YC.MIRROR_ROUNDING


def test_known_answers_right_of_way():
    x0, traj, dv = crossing(at=3)
    # the plans are 2.25 m apart or less at steps 2 (1.6 sqrt 2 = 2.26 > 2.25: not yet), 3
    # (0) and 4: the first conflict is at step 3 ... and at step 2 with a band of 0.3
    # a clear road: the other vehicle far away
    far = traj.copy()
    far[:, 0, 1] += 100.0
    for v in (0, 1):
        a, k, c, ka, wh, ds = run([row(prio=0), row(prio=0)], x0, far, dv, v)
        assert (a, k, ka, wh, ds) == (0.0, -1, -1, -1, INF) and c > 90
    # a tie: both brake, as the governor has it
    for v in (0, 1):
        a, k, c, ka, wh, ds = run([row(prio=5), row(prio=5)], x0, traj, dv, v)
        assert (a, k, ka, wh) == (-3.0, 3, 3, 1 - v) and c == -2.25
        assert abs(ds - 3 * 1.6) < 1e-14
    # distinct ranks: the outranked vehicle brakes and the other does not, whichever it is
    for hi in (0, 1):
        rows = [row(prio=7 if v == hi else 2) for v in (0, 1)]
        a, k, c, ka, wh, ds = run(rows, x0, traj, dv, hi)
        assert (a, k, ka, wh, ds) == (0.0, -1, 3, -1, INF) and c == -2.25
        a, k, c, ka, wh, ds = run(rows, x0, traj, dv, 1 - hi)
        assert (a, k, ka, wh) == (-3.0, 3, 3, hi) and c == -2.25
    # who carries n_obst: with two obstacles far away the vehicle w is 2 + w
    obst = np.full((2, 2, 6), 500.0)
    a, k, c, ka, wh, ds = run([row(prio=1), row(prio=2)], x0, traj, dv, 0, obst=obst,
                              do=np.full(2, 2.0))
    assert (k, wh) == (3, 3)
    # ... and an obstacle on the plan at step 1 is yielded to whatever the rank; it comes first
    obst[1, :, 1] = traj[1, :, 0]
    a, k, c, ka, wh, ds = run([row(prio=9), row(prio=2)], x0, traj, dv, 0, obst=obst,
                              do=np.full(2, 2.0))
    assert (a, k, ka, wh) == (-3.0, 1, 1, 1) and abs(ds - 1.6) < 1e-15
    # an obstacle and a counted vehicle at the same step: the smallest j, the obstacle
    obst[1, :, 3] = traj[3, :, 0]
    obst[1, :, 1] = 500.0
    assert run([row(prio=1), row(prio=2)], x0, traj, dv, 0, obst=obst, do=np.full(2, 2.0))[4] == 1


def test_known_answers_standing_off_and_bad_others_are_yielded_to():
    x0, traj, dv = crossing(at=3)
    top = row(prio=9, s_stand=0.5)
    # vehicle 0 outranks vehicle 1 and does not yield ...
    assert run([top, row(prio=1)], x0, traj, dv, 0)[1] == -1
    # ... unless vehicle 1 stands: at or below S_STAND, or a speed that is not a number
    for s1, stands in ((0.6, False), (0.5, True), (0.0, True), (-1.0, True), (math.nan, True),
                       (INF, False)):
        x = x0.copy()
        x[1, 3] = s1
        a, k, c, ka, wh, ds = run([top, row(prio=1)], x, traj, dv, 0)
        assert (k, wh) == ((3, 1) if stands else (-1, -1)), s1
    # S_STAND = 0: the rule is off, a vehicle at speed 0 keeps its rank
    x = x0.copy()
    x[1, 3] = 0.0
    assert run([row(prio=9), row(prio=1)], x, traj, dv, 0)[1] == -1
    # it is the yielding side's S_STAND that is asked, not the other's
    assert run([row(prio=9), row(prio=1, s_stand=5.0)], x, traj, dv, 0)[1] == -1
    # a vehicle without a governor, or with a bad row, never yields: it is yielded to
    for other in (np.zeros(10), row(prio=1, a_ease=3.5), row(prio=1.5), row(prio=1, k_v=-1.0),
                  row(prio=2.0 ** 20 + 1), row(prio=1, s_stand=math.nan)):
        a, k, c, ka, wh, ds = run([row(prio=9), other], x0, traj, dv, 0)
        assert (a, k, wh) == (-3.0, 3, 1)
    # ... by its fields alone: a bad state of the other vehicle does not make its row bad
    x = x0.copy()
    x[1, 4] = math.nan
    assert run([row(prio=9), row(prio=1)], x, traj, dv, 0)[1] == -1
    # a plan that is not a number counts whatever the ranks
    t = traj.copy()
    t[2, 1, 1] = math.nan
    a, k, c, ka, wh, ds = run([row(prio=9), row(prio=1)], x0, t, dv, 0)
    assert (a, k, ka, wh, c) == (-3.0, 2, 2, 1, -INF)


def test_known_answers_graded_braking():
    # k_conf = 0: nothing of the plan lies before the conflict, full braking
    x0, traj, dv = crossing(at=0)
    a, k, c, ka, wh, ds = run([row(a_ease=0.0), row()], x0, traj, dv, 0)
    assert (a, k, ds) == (-3.0, 0, 0.0)
    # s^2 / 2d by hand: 4 m/s, the conflict at step 5 with a band of 0 (step 4 is 2.26 m
    # away), five segments of 1.6 m -> 16 / 16 = 1 m/s^2
    x0, traj, dv = crossing(at=5, hb=8)
    lo = [row(a_ease=0.0, band=0.0, look=8), row(prio=1)]
    a, k, c, ka, wh, ds = run(lo, x0, traj, dv, 0)
    assert k == 5 and abs(ds - 8.0) < 1e-14 and abs(a + 1.0) < 1e-14
    for fm in (YM.F64, YM.F80):
        a, k, c, ka, wh, ds = run(lo, x0, traj, dv, 0, fm)
        assert a == -(fm.num(4.0) * fm.num(4.0)) / (fm.num(2.0) * ds)
    # A_EASE is the gentlest: 1.2 > 1; A_BRAKE the largest: one segment asks for 5
    lo[0][YM.A_EASE] = 1.2
    assert run(lo, x0, traj, dv, 0)[0] == -1.2
    x1, t1, _ = crossing(at=1)
    a, k, c, ka, wh, ds = run([row(a_ease=0.0, band=0.0), row(prio=1)], x1, t1, dv, 0)
    assert (a, k) == (-3.0, 1) and abs(ds - 1.6) < 1e-15
    # a speed of zero or below needs nothing; A_EASE still holds, and the stop rule has the
    # last word
    x = x0.copy()
    x[0, 3] = 0.0
    det = {}
    a = run([row(a_ease=0.5, band=0.0, look=8), row(prio=1)], x, traj, dv, 0, detail=det)[0]
    assert det["a_need"] == 0.0 and det["a_des"] == -0.5 and a == 0.0
    # a plan start that is not a number: d_stop is not finite, full braking
    x = x0.copy()
    x[0, 0] = math.nan
    a, k, c, ka, wh, ds = run(lo, x, traj, dv, 0)
    assert a == -3.0 and k == 5 and math.isnan(ds)
    # the slew limit and the stop rule are the governor's
    x = x0.copy()
    x[0, 4] = 0.5
    lo[0][YM.J_MAX] = 2.0
    assert run(lo, x, traj, dv, 0)[0] == 0.5 - 2.0 * TH


def test_off_row_and_every_kind_of_bad_row():
    x0, traj, dv = crossing(at=3)
    off = np.zeros(10)
    off[8] = -0.0
    for a_now in (1.25, -0.0, math.nan):
        x = x0.copy() * math.nan
        x[0, 4] = a_now
        a, k, c, ka, wh, ds = run([off, row()], x, traj * math.nan, dv, 0)
        assert np.array(a).tobytes() == np.array(a_now).tobytes() and (k, ka, wh) == (-1, -1, -1)
        assert math.isnan(c) and math.isnan(ds)
    bad = {f"{f}_{v}": (f, v) for f in range(10) for v in (-1e-300, math.nan, -INF)}
    bad.update({f"inf_{f}": (f, INF) for f in range(10) if f != YM.J_MAX})
    bad.update(look_fraction=(YM.LOOK, 2.5), look_above=(YM.LOOK, 65.0),
               prio_fraction=(YM.PRIO, 0.5), prio_above=(YM.PRIO, 2.0 ** 20 + 1),
               ease_above_brake=(YM.A_EASE, 3.0 + 1e-12))
    assert len(bad) == 44
    for kind, (f, v) in bad.items():
        r = row()
        r[f] = v
        assert YM.is_bad_row(r), kind
        a, k, c, ka, wh, ds = run([r, row()], x0, traj, dv, 0)
        assert math.isnan(a) and (k, ka, wh) == (-2, -2, -2) and math.isnan(c) and math.isnan(ds), kind
        with pytest.raises(ValueError, match=LB.YLD_FIELDS[f]):
            YLD.validate(r[None, None])
    for s, a_now in ((math.nan, 0.0), (INF, 0.0), (4.0, math.nan), (4.0, -INF)):
        x = x0.copy()
        x[0, 3:5] = (s, a_now)
        a, k, c, ka, wh, ds = run([row(), row()], x, traj, dv, 0)
        assert math.isnan(a) and (k, ka, wh) == (-2, -2, -2)
    a, k, *_ = YM.lane([row(), row()], x0, 0, None, None, None, None, None, dv[0], TH, TB)
    assert math.isnan(a) and k == -2                        # a horizon outside its slot
    # what is not bad: rank 0 and 2^20, A_EASE = 0 and = A_BRAKE, S_STAND = 0, a -0.0
    for r in (row(prio=0), row(prio=2.0 ** 20), row(a_ease=0.0), row(a_ease=3.0),
              row(s_stand=-0.0), row(j_max=INF), row(look=0), row(look=64)):
        assert not YM.is_bad_row(r)
        YLD.validate(r[None, None])
    assert not YM.is_bad_row(off)


@pytest.mark.parametrize("cid", YC.IDS)
def test_reduction_to_the_governor_is_bitwise(cid):
    """Equal ranks, A_EASE = A_BRAKE, S_STAND = 0: a_cmd, k_conf and clear of governor_mirror,
    bit for bit, in both number formats; and k_any = k_conf."""
    c, d = YC.by_id(cid), YC.inputs(cid)
    rows, grows = YC.reducing(cid)
    assert np.array_equal(rows[..., :7], grows) and (rows[..., YM.S_STAND] == 0).all()
    for fm in (YM.F64, YM.F80):
        arg = (d["x0"], d["traj"], d["obst"], d["margin"], d["hp"], d["dreq_obs"], d["dreq_veh"],
               TH, TB, c.hp_max, fm)
        y = YM.step(rows, *arg)
        g = GM.step(grows, *arg)
        for i in range(3):
            # value, NaN pattern and sign of zero: the 80-bit format has padding bytes
            assert np.array_equal(y[i], g[i], equal_nan=True), i
            assert np.array_equal(np.signbit(y[i]), np.signbit(g[i])), i
            if fm is YM.F64:
                assert y[i].tobytes() == g[i].tobytes(), i
        assert np.array_equal(y[3], y[1])


# ---------------------------------------------------------------------------
# 3. two properties
# ---------------------------------------------------------------------------
def random_batch(seed=4711, B=24, nV=5, hb=8):
    """Plans that wander over a 12 m square, so that many pairs conflict; distinct ranks (a
    permutation per realisation), S_STAND = 0, no obstacle."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, nV, 6))
    x0[..., 0:2] = rng.uniform(0, 12, (B, nV, 2))
    x0[..., 3] = rng.uniform(0, 5, (B, nV))
    x0[..., 4] = rng.uniform(-1, 1, (B, nV))
    steps = rng.uniform(-1.5, 1.5, (B, hb, 2, nV))
    traj = x0[..., 0:2].transpose(0, 2, 1)[:, None] + np.cumsum(steps, axis=1)
    rows = np.zeros((B, nV, 10))
    for b in range(B):
        for v in range(nV):
            rows[b, v] = row(look=rng.integers(1, hb + 1), band=rng.uniform(0, 0.5),
                             a_ease=rng.uniform(0, 3))
        rows[b, :, YM.PRIO] = rng.permutation(nV) * 3
    dv = 2.0 + rng.uniform(0, 1, (B, nV, nV))
    return dict(rows=rows, x0=x0, traj=traj, obst=None, margin=None, hp=None, dreq_obs=None,
                dreq_veh=dv), hb


def _sets():
    for cid in YC.IDS:
        yield cid, YC.inputs(cid), YC.by_id(cid).hp_max, YC.mirror(cid), \
            YC.mirror(cid, details=True)
    d, hb = random_batch()
    det = {}
    out = YM.step(d["rows"], d["x0"], d["traj"], None, None, None, None, d["dreq_veh"], TH, TB, hb,
                  details=det)
    yield "random", d, hb, out, det


def test_the_top_ranked_vehicle_never_yields_to_a_vehicle():
    """Valid rows of distinct ranks, finite entries, no obstacle conflict, S_STAND = 0: the
    top-ranked vehicle has k_conf = -1."""
    n = 0
    for name, d, hp_max, out, det in _sets():
        rows = d["rows"]
        B, nV = rows.shape[:2]
        for b in range(B):
            r = rows[b]
            if any(YM.is_off_row(x) or YM.is_bad_row(x) for x in r) or (r[:, YM.S_STAND] != 0).any():
                continue
            if len(set(r[:, YM.PRIO])) != nV or not np.isfinite(d["x0"][b]).all():
                continue
            top = int(np.argmax(r[:, YM.PRIO]))
            cs = det[(b, top)]["clearances"]
            if any(not np.isfinite(c) or (w[0] == "o" and c < 0) for k, c, w, _ in cs):
                continue
            assert out[1][b, top] == -1 and out[4][b, top] == -1, (name, b)
            n += out[3][b, top] >= 0
    assert n >= 10                      # ... while somebody was in its way


def test_of_two_vehicles_in_conflict_at_least_one_yields():
    """Every pair with c < 0 in both lanes' own examination has a lane with k_conf >= 0."""
    n = 0
    for name, d, hp_max, out, det in _sets():
        B, nV = d["rows"].shape[:2]
        for b in range(B):
            neg = {v: {(k, w[1]) for k, c, w, _ in det[(b, v)].get("clearances", ())
                       if w[0] == "v" and c < 0} for v in range(nV)}
            for v in range(nV):
                for k, w in neg[v]:
                    if (k, v) in neg[w]:
                        assert out[1][b, v] >= 0 or out[1][b, w] >= 0, (name, b, v, w, k)
                        n += 1
    assert n >= 100


# ---------------------------------------------------------------------------
# 4. the case table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", YC.IDS)
def test_case_conditions(cid):
    """The governor's separations, a_need against A_EASE and A_BRAKE, and the speeds against
    S_STAND, in float64 and in 80-bit: none is left out."""
    c, d = YC.by_id(cid), YC.inputs(cid)
    SEP = YC.SEP
    for fm in (YM.F64, YM.F80):
        det = YC.mirror(cid, fm, details=True)
        assert len(det) == c.B * c.n_veh
        for (b, v), e in det.items():
            r = d["rows"][b, v]
            if YM.is_off_row(r) or YM.is_bad_row(r):
                assert "clearances" not in e and d["pattern"][b] in ("off", "bad") and v == 1
                continue
            for k, cc, which, _ in e["clearances"]:
                assert abs(cc) >= SEP, (b, v, k, which)
            if not e["conflict"]:
                assert abs(e["wish"] + r[YM.A_BRAKE]) >= SEP and abs(e["wish"] - r[YM.A_ACC]) >= SEP
            else:
                assert abs(e["a_need"] - r[YM.A_EASE]) >= SEP, (b, v)
                assert abs(e["a_need"] - r[YM.A_BRAKE]) >= SEP, (b, v)
            if e["lo"] is not None:
                assert abs(e["a_des"] - e["lo"]) >= SEP and abs(e["a_des"] - e["hi"]) >= SEP
            assert abs(e["s_raw"]) >= SEP
            assert abs(e["a_slew"] - e["floor"]) >= SEP
            assert r[YM.A_ACC] > 0 and r[YM.A_BRAKE] > 0
            if r[YM.S_STAND] > 0:
                for w in range(c.n_veh):
                    assert abs(d["x0"][b, w, 3] - r[YM.S_STAND]) >= SEP


def test_what_the_table_covers():
    seen = set()
    for cid in YC.IDS:
        c, d = YC.by_id(cid), YC.inputs(cid)
        a, kc, cl, ka, wh, ds = YC.mirror(cid)
        det = YC.mirror(cid, details=True)
        nO = c.n_obst
        for b in range(c.B):
            seen.add(("pattern", d["pattern"][b]))
        for (b, v), e in det.items():
            r = d["rows"][b, v]
            if "clearances" not in e:
                seen.add("off_lane" if YM.is_off_row(r) else "bad_lane")
                continue
            seen.add(("ease", "brake" if r[YM.A_EASE] == r[YM.A_BRAKE] else
                      "zero" if r[YM.A_EASE] == 0 else "between"))
            pat = d["pattern"][b]
            if ka[b, v] >= 0 and kc[b, v] == -1:
                seen.add("has_right_of_way")
            if ka[b, v] >= 0 and kc[b, v] > ka[b, v]:
                seen.add("yields_later_than_the_first_conflict")
            if kc[b, v] >= 0:
                seen.add("who_obstacle" if wh[b, v] < nO else "who_vehicle")
                seen.add(("d_stop", "0" if kc[b, v] == 0 else "one" if kc[b, v] == 1 else "many"))
                an, ae, ab = float(e["a_need"]), r[YM.A_EASE], r[YM.A_BRAKE]
                seen.add(("a_need", "inf" if an == INF else "above" if an > ab else
                          "graded" if an > ae else "below_ease"))
                w = wh[b, v] - nO
                if w >= 0 and r[YM.PRIO] > d["rows"][b, w, YM.PRIO]:
                    seen.add(("outranks_but_yields", pat))
                if w >= 0 and r[YM.PRIO] == d["rows"][b, w, YM.PRIO]:
                    seen.add("tie_yields")
            if pat == "standing" and v == 0 and c.n_veh > 1:
                seen.add(("stands", bool(d["x0"][b, 1, 3] < YC.STAND), bool(e["counts"][1])))
            if pat == "zero" and v == 0 and c.n_veh > 1:
                assert d["x0"][b, 1, 3] == 0.0 and not e["counts"][1]
                seen.add("speed_zero_keeps_its_rank")
    want = {("pattern", p) for p in YC.PATTERNS} | {("ease", k) for k in ("brake", "zero", "between")} \
        | {("d_stop", k) for k in ("0", "one", "many")} \
        | {("a_need", k) for k in ("inf", "above", "graded", "below_ease")} \
        | {("outranks_but_yields", p) for p in ("off", "bad", "standing")} \
        | {("stands", True, True), ("stands", False, False)} \
        | {"off_lane", "bad_lane", "has_right_of_way", "who_obstacle", "who_vehicle", "tie_yields",
           "speed_zero_keeps_its_rank"}
    assert want <= seen, want - seen


def test_tolerance_is_sixteen_times_the_rounding_of_the_definition():
    worst = {cid: YC.ratio(YC.mirror(cid, YM.F64), YC.mirror(cid, YM.F80), cid) for cid in YC.IDS}
    print("yield mirror float64 against 80-bit:", {k: f"{v:.3g}" for k, v in worst.items()})
    big = max(worst.values())
    assert 0.5 * YC.MIRROR_ROUNDING <= big <= YC.MIRROR_ROUNDING
    assert YC.TOL == YC.pow2_ceil(16 * YC.MIRROR_ROUNDING)


# ---------------------------------------------------------------------------
# 5. the Python side
# ---------------------------------------------------------------------------
def test_rows_from_governor_off_from_table_and_validate():
    import torch
    kw = dict(v_ref=[4.0, 3.0], a_acc=1.0, a_brake=3.0, k_v=0.5, look=5, device="cpu")
    y = YLD.rows(3, 2, prio=[1, 0], **kw)
    assert tuple(y.shape) == (3, 2, 10)
    assert y[1, 1].tolist() == [3.0, 1.0, 3.0, 0.5, INF, 5.0, 0.0, 0.0, 3.0, 0.0]   # a_ease = a_brake
    y2 = YLD.rows(3, 2, prio=7, a_ease=0.5, s_stand=0.2, **kw)
    assert y2[0, 0, 7:].tolist() == [7.0, 0.5, 0.2]
    g = GOV.rows(3, 2, **kw)
    assert torch.equal(YLD.from_governor(g, [1, 0]), y)
    assert torch.equal(YLD.from_governor(g, 7, a_ease=0.5, s_stand=0.2), y2)
    # an off governor row stays off, whatever rank is asked
    g0 = g.clone()
    g0[1, 0] = 0.0
    f = YLD.from_governor(g0, 5)
    assert (f[1, 0] == 0).all() and f[1, 1, 7] == 5 and not YLD.is_off(f)
    assert YLD.is_off(YLD.off(3, 2, device="cpu")) and YLD.is_off(YLD.from_governor(GOV.off(3, 2, device="cpu"), 4))
    t = YLD.from_table(torch.stack([YLD.off(1, 2, device="cpu")[0], y[0]]), [1, 0, 1], device="cpu")
    assert tuple(t.shape) == (3, 2, 10) and YLD.is_off(t[1:2]) and (t[2] == y[0]).all()
    with pytest.raises(ValueError, match="index"):
        YLD.from_table(y, [3], device="cpu")
    with pytest.raises(ValueError, match=r"\[K, nVeh, 10\]"):
        YLD.from_table(g, [0], device="cpu")
    with pytest.raises(ValueError, match="a_brake"):
        YLD.rows(3, 2, prio=0, **dict(kw, a_brake=-3.0))
    with pytest.raises(ValueError, match="prio"):
        YLD.rows(3, 2, prio=0.5, **kw)
    with pytest.raises(ValueError, match="prio"):
        YLD.from_governor(g, 2 ** 20 + 1)
    with pytest.raises(ValueError, match="a_ease must be <= a_brake"):
        YLD.rows(3, 2, prio=0, a_ease=3.5, **kw)
    with pytest.raises(ValueError, match="s_stand"):
        YLD.rows(3, 2, prio=0, s_stand=-1.0, **kw)
    with pytest.raises(ValueError, match="broadcast"):
        YLD.rows(3, 2, prio=[1, 2, 3], **kw)
    with pytest.raises(ValueError, match=r"\[B, nVeh, 7\]"):
        YLD.from_governor(y, 0)
    with pytest.raises(ValueError, match=r"\[B, nVeh, 10\]"):
        YLD.validate(np.zeros((3, 2, 7)))
    with pytest.raises(ValueError, match=r"rows\[1, 0\]: a_ease"):
        bad = y.numpy().copy()
        bad[1, 0, YM.A_EASE] = math.nan
        YLD.validate(bad)


def test_crossing_scene_geometry():
    """The rollout scene of yield_cases.crossing_scene, fixed before any ranked run: on straight
    plans the mirror finds the conflict at step 5 in both lanes with equal ranks, and in the
    outranked lane only with distinct ranks."""
    scs, variant_of, x_init, ranks = YC.crossing_scene()
    assert len(scs) == 2 and x_init.shape == (YC.CROSS_B, 2, 6) and variant_of.tolist() == [0, 1, 0, 1]
    for sc in scs:
        assert sc.nVeh == 2 and sc.nObst == 0 and sc.Hp == YC.CROSS_HP
        for v in range(2):                                   # equal distance to the crossing
            assert math.hypot(*np.asarray(sc.x0[v])[:2]) == YC.CROSS_D
        radius = (sc.Lf[0] + sc.Lr[0]) / math.tan(sc.mechanicalSteeringLimit)
        assert radius > YC.CROSS_D
    dv = np.stack([np.asarray(scs[k].dsafeVehicles, float).reshape(2, 2) for k in variant_of])
    assert np.array_equal(dv[:, 0, 1], dv[:, 1, 0])
    x0, traj = YC.straight_plans(scs, variant_of, x_init)
    gap = np.hypot(*(traj[:, :, :, 0] - traj[:, :, :, 1]).transpose(2, 0, 1))     # [B, Hp]
    assert np.allclose(gap[:, 6], math.sqrt(2) * abs(YC.CROSS_D - 0.12 - 1.6 * 7))
    need = dv[:, 0, 1] + YC.CROSS_KW["band"]
    assert YC.CROSS_KW["band"] > scs[0].dsafeExtra          # more than the planner keeps
    assert (gap[:, 5] < need).all() and (gap[:, 4] > need).all()
    g = GOV.rows(YC.CROSS_B, 2, device="cpu", **YC.CROSS_KW)
    rows = YLD.from_governor(g, ranks).numpy()
    a, kc, cl, ka, wh, ds = YM.step(rows, x0, traj, None, None, None, None, dv, scs[0].dt,
                                    scs[0].delay_u, YC.CROSS_HP)
    assert (ka == 5).all()
    assert kc.tolist() == [[5, 5], [5, 5], [-1, 5], [5, -1]]
    assert wh.tolist() == [[1, 0], [1, 0], [-1, 0], [1, -1]]
    assert np.allclose(ds[kc >= 0], 4.0 * 0.4 * 5) and (a[kc >= 0] == -3.0).all() and (a[kc < 0] == 0).all()
