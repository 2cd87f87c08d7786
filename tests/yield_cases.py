"""The inputs of the right-of-way tests, shared by the CPU tests (tests/test_yield_host.py: the
conditions on the table and the tolerance are pinned there, on the mirror alone) and the GPU
tests (tests/test_gpu_yield.py), so that both see exactly the same numbers.

The nine shapes, plans, obstacles and planted kinds are those of ``governor_cases.inputs``.  On
top of them, per realisation b:

  - ``x0[:, :, 0:2]`` lies one step (1.6 m) behind each plan's first point, so d_stop counts a
    whole segment per step;
  - where there are two vehicles, vehicle 1's plan meets vehicle 0's at step ``(last examined,
    0, 1)[b % 3]`` (d_stop many segments, 0 and one), and vehicle 1 looks over its whole
    horizon, so both see it;
  - the ranks follow ``PATTERNS[(b + b // 8) % 8]``:
      equal       every vehicle rank 3
      ascending   rank v
      descending  rank n_veh - 1 - v
      ties        rank v // 2
      off         descending, vehicle 1 without a governor (an off row)
      bad         descending, vehicle 1 with a bad row (its rank, its A_EASE or its K_V in turn)
      standing    descending, S_STAND = 1 m/s, vehicle 1 at 0.5 m/s or at its cruise speed in
                  turn: both sides of S_STAND
      zero        descending, S_STAND = 0, vehicle 1 at speed 0 exactly
  - A_EASE cycles over A_BRAKE, 0 and 0.4 A_BRAKE with b + v.

Conditions, checked by test_yield_host.py with none left out: the governor's separations (every
examined clearance has |c| >= 1e-9 m, every clamp argument that decides a branch differs from its
bound by >= 1e-9); a_need keeps 1e-9 m/s^2 from A_EASE and from A_BRAKE; every x0[w][3] keeps
1e-9 m/s from every S_STAND > 0 of its realisation.  Under them every integer output and every
branch is the same in any correct float64 evaluation."""
from __future__ import annotations

import functools
import math

import numpy as np

import governor_cases as GC
import governor_mirror as GM
import yield_mirror as YM
from governor_cases import CASES, IDS, SEP, T_BACK, T_HOLD, by_id, pow2_ceil  # noqa: F401

PATTERNS = ("equal", "ascending", "descending", "ties", "off", "bad", "standing", "zero")
EASE = (1.0, 0.0, 0.4)            # A_EASE as a share of A_BRAKE
STAND = 1.0                       # m/s: S_STAND of the "standing" pattern
STEP_LEN = 1.6                    # metres between the plan points of governor_cases


def pattern_of(b):
    return PATTERNS[(b + b // 8) % 8]


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """The dict of ``governor_cases.inputs`` with rows [B, nV, 10], and ``pattern`` [B]."""
    c = by_id(cid)
    g = GC.inputs(cid)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    nV, B, Hm = c.n_veh, c.B, c.hp_max
    rows = np.zeros((B, nV, YM.NP))
    rows[..., :GM.NP] = g["rows"]
    x0, traj = d["x0"], d["traj"].reshape(B, -1)
    patterns = []
    for b in range(B):
        hb = Hm if d["hp"] is None else int(d["hp"][b])
        t = traj[b, :hb * 2 * nV].reshape(hb, 2, nV)       # a view: edits land in the slot
        pat = pattern_of(b)
        patterns.append(pat)
        if nV > 1:
            K = min(int(rows[b, 0, YM.LOOK]), hb)
            at = ((K if K > 0 else hb) - 1, 0, min(1, hb - 1))[b % 3]
            t[at, :, 1] = t[at, :, 0] + (0.3, 0.2)
            rows[b, 1, YM.LOOK] = hb
        v = np.arange(nV)
        rows[b, :, YM.PRIO] = {"equal": 3 + 0 * v, "ascending": v, "ties": v // 2}.get(
            pat, nV - 1 - v)
        for w in range(nV):
            rows[b, w, YM.A_EASE] = EASE[(b + w) % 3] * rows[b, w, YM.A_BRAKE]
        if pat == "standing":
            rows[b, :, YM.S_STAND] = STAND
        if nV > 1:
            if pat == "off":
                rows[b, 1] = 0.0
            elif pat == "bad":
                f, val = ((YM.PRIO, 2.5), (YM.A_EASE, rows[b, 1, YM.A_BRAKE] + 0.5),
                          (YM.K_V, -1.0))[(b // 8) % 3]
                rows[b, 1, f] = val
            elif pat == "standing" and (b // 8) % 2 == 0:
                x0[b, 1, 3] = 0.5
            elif pat == "zero":
                x0[b, 1, 3] = 0.0
                rows[b, 1, YM.A_EASE] = 0.4 * rows[b, 1, YM.A_BRAKE]   # a_need = 0 keeps off it
        x0[b, :, 0] = t[0, 0, :] - STEP_LEN
        x0[b, :, 1] = t[0, 1, :]
    d["rows"], d["pattern"] = rows, patterns
    d["traj"] = traj.reshape(B, Hm, 2, nV)
    return d


@functools.lru_cache(maxsize=None)
def reducing(cid):
    """The case with equal ranks, A_EASE = A_BRAKE and S_STAND = 0 in every row that is not off:
    (rows [B, nV, 10], the governor rows [B, nV, 7] they reduce to)."""
    rows = inputs(cid)["rows"].copy()
    on = ~(rows == 0.0).all(axis=2)
    rows[..., YM.PRIO] = np.where(on, 3.0, 0.0)
    rows[..., YM.A_EASE] = np.where(on, rows[..., YM.A_BRAKE], 0.0)
    rows[..., YM.S_STAND] = 0.0
    return rows, rows[..., :GM.NP].copy()


_mirror_cache = {}


def mirror(cid, fm=YM.F64, details=False):
    """(a_cmd, k_conf, clear, k_any, who, d_stop) of the case on the mirror, computed once per
    number format and shared; with ``details`` the per-lane dict of ``yield_mirror.step``."""
    key = (cid, fm.dtype)
    if key not in _mirror_cache:
        c, d, det = by_id(cid), inputs(cid), {}
        out = YM.step(d["rows"], d["x0"], d["traj"], d["obst"], d["margin"], d["hp"],
                      d["dreq_obs"], d["dreq_veh"], T_HOLD, T_BACK, c.hp_max, fm, det)
        _mirror_cache[key] = (out, det)
    return _mirror_cache[key][1 if details else 0]


# ---------------------------------------------------------------------------
# The comparison and its tolerance
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def yardsticks(cid):
    """(Y_a, Y_c, Y_d) [B, nV]: the sums of the absolute terms of the three expressions, from
    the 80-bit mirror.  a_cmd: the governor's (``governor_cases.yardsticks``; it holds A_BRAKE,
    which bounds the graded deceleration).  clear: the distance of the pair that gives the
    minimum plus its required distance, margin and band.  d_stop: the sum itself, every term of
    which is a length (1 where it is 0 or not finite)."""
    d = inputs(cid)
    det = mirror(cid, YM.F80, details=True)
    out = mirror(cid, YM.F80)
    rows, x0 = d["rows"], d["x0"]
    B, nV = rows.shape[:2]
    Ya, Yc, Yd = np.ones((B, nV)), np.ones((B, nV)), np.ones((B, nV))
    for (b, v), e in det.items():
        r, s, a = rows[b, v], abs(x0[b, v, 3]), abs(x0[b, v, 4])
        if "clearances" not in e:
            continue
        j = r[YM.J_MAX] * T_HOLD if math.isfinite(r[YM.J_MAX]) else 0.0
        Ya[b, v] = r[YM.K_V] * (r[YM.V_REF] + s) + r[YM.A_BRAKE] + r[YM.A_ACC] + a + j \
            + (s + a * T_BACK) / T_HOLD
        if e["clearances"]:
            Yc[b, v] = float(min(e["clearances"], key=lambda t: t[1])[3])
        ds = float(out[5][b, v])
        if math.isfinite(ds) and ds > 0:
            Yd[b, v] = ds
    return Ya, Yc, Yd


def ratio(dev, mir, cid):
    """The one figure of the comparison: |d a_cmd| / Y_a, |d clear| / Y_c and |d d_stop| / Y_d
    over the lanes, with ``mir`` the reference (both in the order of ``yield_mirror.step``);
    NaN patterns and infinities must be identical."""
    f = lambda a: np.asarray(a, dtype=np.longdouble)
    worst = 0.0
    for i, Y in zip((0, 2, 5), yardsticks(cid)):
        x, m = f(dev[i]), f(mir[i])
        assert (np.isnan(x) == np.isnan(m)).all(), i
        assert (np.isinf(x) == np.isinf(m)).all() and (x[np.isinf(m)] == m[np.isinf(m)]).all(), i
        ok = np.isfinite(m)
        if ok.any():
            x, m = np.where(ok, x, 0), np.where(ok, m, 0)
            worst = max(worst, float((np.abs(x - m)[ok] / Y[ok]).max()))
    return worst


# Tolerance of the device against the float64 mirror, in the figure of ``ratio``, by the
# governor's method.  It is derived on the CPU from the reference alone (tests/test_yield_host.py,
# test_tolerance_is_sixteen_times_the_rounding_of_the_definition): the largest figure between the
# mirror in float64 and the mirror in 80-bit over the table is MIRROR_ROUNDING.  The device
# contracts multiply-adds, has its own sqrt and division and adds the segments of d_stop in
# another order: 16 times the figure, rounded up to a power of two.
# Per case: 1x0x3 2.4e-18, 1x1x1 1.984e-16, 1x3x10 1.58e-16 (1.08e-16 without margins), 4x0x20
# 1.93e-16, 5x2x10 1.44e-16 (1.17e-16), 16x32x64 2.902e-16 (d_stop over 63 segments),
# 3x2x30_mixed 1.91e-16.
MIRROR_ROUNDING = 2.91e-16
TOL = 2.0 ** -47                  # 16 * 2.91e-16 = 4.66e-15 <= 2^-47 = 7.11e-15


# ---------------------------------------------------------------------------
# The rollout scene in which two references cross at equal distance
# ---------------------------------------------------------------------------
# Two vehicles at 4 m/s, CROSS_D = 12 m from the point where their reference polylines cross at
# a right angle: vehicle 0 drives east along y = 0; vehicle 1 drives north along x = 0 in variant
# 0 and south in variant 1 (the variants' per-problem polylines and start states).  Undisturbed,
# both reach the crossing after 3 s, 7.5 MPC steps.  The plan's point k lies 1.6 (k + 1) m on plus
# the 0.12 m of the transport delay, so two straight plans are sqrt(2) |12 - 0.12 - 1.6 (k + 1)|
# apart: 5.49 m at k = 4, 3.22 m at k = 5, 0.96 m at k = 6.  The required centre distance of two
# vehicles is 2.07 m (Scenarios.py:229-252) and the planner keeps dsafeExtra = 1 m on top of it
# where it can, so the rows ask for BAND = 1.5 m, more than the planner keeps: a plan that steers
# apart as far as its own constraint demands is still a conflict here, and straight plans conflict
# first at k = 5 of a horizon of 10.  B = 4 realisations (both variants, equal and distinct ranks)
# and Hp = 10 are the smallest that show it.  The geometry is checked on the CPU
# (tests/test_yield_host.py) with straight plans and the mirror.
CROSS_D, CROSS_HP, CROSS_STEPS, CROSS_B = 12.0, 10, 9, 4
CROSS_KW = dict(v_ref=4.0, a_acc=1.0, a_brake=3.0, k_v=0.5, look=CROSS_HP, band=1.5)
# realisation b: (variant, rank of vehicle 0, rank of vehicle 1)
CROSS_RUNS = ((0, 1, 1), (1, 1, 1), (0, 2, 1), (1, 1, 2))


def crossing_scene():
    """(variants [2 scenarios], variant_of [B], x_init [B, 2, 6], ranks [B, 2])."""
    GC._paths()
    from oracle import scp_reference as R
    scs = []
    for sign in (1.0, -1.0):
        sc = R.OracleScenario(Hp=CROSS_HP, Hu=CROSS_HP)
        sc.add_vehicle(-CROSS_D, 0.0, 0.0, [[-100.0, 0.0], [100.0, 0.0]])
        sc.add_vehicle(0.0, -sign * CROSS_D, sign * math.pi / 2,
                       [[0.0, -sign * 100.0], [0.0, sign * 100.0]])
        scs.append(sc.complete())
    variant_of = np.array([r[0] for r in CROSS_RUNS], np.int32)
    x_init = np.stack([np.array(scs[k].x0, float) for k in variant_of])
    ranks = np.array([r[1:] for r in CROSS_RUNS], float)
    return scs, variant_of, x_init, ranks


def straight_plans(scs, variant_of, x_init):
    """The plans of vehicles that hold their speed and heading: traj [B, Hp, 2, 2] with point k
    (k + 1) dt + delay_u on from x_init, the start of the plan x0 [B, 2, 6] at delay_u on."""
    sc = scs[0]
    B = len(variant_of)
    x0 = x_init.copy()
    traj = np.zeros((B, CROSS_HP, 2, 2))
    for b in range(B):
        for v in range(2):
            x, y, h, s = x_init[b, v, :4]
            x0[b, v, 0:2] = (x + s * sc.delay_u * math.cos(h), y + s * sc.delay_u * math.sin(h))
            for k in range(CROSS_HP):
                t = (k + 1) * sc.dt + sc.delay_u
                traj[b, k, :, v] = (x + s * t * math.cos(h), y + s * t * math.sin(h))
    return x0, traj
