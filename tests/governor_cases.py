"""The inputs of the speed-governor tests, shared by the CPU tests (tests/test_governor_host.py:
the conditions on the table and the tolerance are pinned there, on the mirror alone) and the GPU
tests (tests/test_gpu_governor.py), so that both see exactly the same numbers.

A case is a shape ``(n_veh, n_obst, hp)`` with B realisations.  Vehicle v of every realisation
plans along its own lane y = 6 v at 1.6 m a step; the obstacles stand in lanes of their own on
the other side (y = -9 (o + 1)), so a plain lane is clear by metres.  Conflicts are planted per
realisation, ``KINDS[b % 8]``, by moving one told point onto vehicle 0's plan:

  clear      nothing planted
  k0         an obstacle point (a vehicle's where there is no obstacle) at step 0
  last       the same at the last step vehicle 0 examines
  at_look    the same at step LOOK exactly, which vehicle 0 does not examine
  pair       vehicle 1's plan meets vehicle 0's at step 1 (both brake); obstacle shapes with
             one vehicle plant an obstacle there
  stop       k0 with vehicle 0 slow (s = 0.3 m/s): the stop rule binds
  clamp      clear, with s = 0.02 m/s below a_now t_back: s_app clamps at 0
  still      k0 at s = 0 exactly with a_now = -1 m/s^2

LOOK cycles over 0, 1, hp and above hp_b per lane (per realisation for vehicle 0, so that every
kind meets every LOOK that can show it), J_MAX alternates between 2 m/s^3 and +inf, the margins
are given (0 .. 0.3 m) or NULL, and the lanes that are not vehicle 0 take their row and state
from a seeded generator.  Conditions, checked by test_governor_host.py with none left out: every
examined clearance has |c| >= 1e-9 m and every clamp argument of steps 2 to 4 that decides a
branch differs from its bound by >= 1e-9, so k_conf and the branches are the same in any correct
float64 evaluation.

The rollout scene (``stop_scene``) is the smallest in which stopping is the only way out."""
from __future__ import annotations

import functools
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

import governor_mirror as GM

T_HOLD, T_BACK = 0.4, 0.03
SEP = 1e-9                    # metres, and m/s^2 for the clamp arguments
KINDS = ("clear", "k0", "last", "at_look", "pair", "stop", "clamp", "still")
SEED = 7301


def _paths():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (here, root, os.path.join(root, "senquential-convex-programming-for-trajectory-planning_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


@dataclass(frozen=True)
class Case:
    n_veh: int
    n_obst: int
    hp_max: int
    B: int
    hps: tuple = None         # the mixed-horizon batch: realisation b at hps[b % len(hps)]
    margin: bool = True       # obst_margin given (False: NULL)

    @property
    def id(self):
        return f"{self.n_veh}x{self.n_obst}x{self.hp_max}" + ("_mixed" if self.hps else "") \
            + ("" if self.margin or not self.n_obst else "_nomargin")


CASES = (
    Case(1, 0, 3, 16),
    Case(1, 1, 1, 16),
    Case(1, 3, 10, 16),
    Case(1, 3, 10, 16, margin=False),
    Case(4, 0, 20, 16),
    Case(5, 2, 10, 16),
    Case(5, 2, 10, 16, margin=False),
    Case(16, 32, 64, 8),
    Case(3, 2, 30, 24, hps=(10, 20, 30)),
)
IDS = [c.id for c in CASES]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def look_of(c, b, hb):
    """LOOK of vehicle 0 of realisation b: 0, 1, hp, above hp_b in turn over the rounds of
    KINDS, shifted by the kind so that the table does not pair a kind with one LOOK only."""
    above = min(hb + 5, GM.MAX_HP)
    return (hb, above, 1, 0)[(b // len(KINDS) + b) % 4]


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """dict of float64 / int32 numpy arrays: rows [B, nV, 7], x0 [B, nV, 6], traj
    [B, hp_max, 2, nV] (slots: problem b's [hp_b][2][nV] packed as the prefix), obst
    [B, nO, 2, hp_max] and margin [B, nO, hp_max] (slots likewise; None without obstacles or
    with margin NULL), hp [B] or None, dreq_obs [B, nV, nO], dreq_veh [B, nV, nV], kind [B]."""
    c = by_id(cid)
    nV, nO, Hm, B = c.n_veh, c.n_obst, c.hp_max, c.B
    rng = np.random.default_rng(SEED + 17 * nV + 3 * nO + Hm + (0 if c.margin else 1))
    hp = None if c.hps is None else np.array([c.hps[b % len(c.hps)] for b in range(B)], np.int32)
    rows = np.zeros((B, nV, GM.NP))
    x0 = np.zeros((B, nV, 6))
    traj = np.zeros((B, Hm * 2 * nV))
    obst = np.zeros((B, nO * 2 * Hm)) if nO else None
    margin = np.zeros((B, nO * Hm)) if nO and c.margin else None
    dreq_obs = 1.5 + rng.uniform(0, 1, (B, nV, nO))
    dreq_veh = 2.0 + rng.uniform(0, 1, (B, nV, nV))
    kinds = []
    for b in range(B):
        hb = Hm if hp is None else int(hp[b])
        kind = KINDS[b % len(KINDS)]
        kinds.append(kind)
        # the plain lanes
        t = np.zeros((hb, 2, nV))
        for v in range(nV):
            sv = 4.0 + rng.uniform(-0.5, 0.5)
            x0[b, v] = (rng.uniform(-1, 1), 6.0 * v, 0.0, sv, rng.uniform(-1, 1), 0.0)
            t[:, 0, v] = x0[b, v, 0] + 1.6 * (np.arange(hb) + 1) + rng.uniform(-0.1, 0.1, hb)
            t[:, 1, v] = 6.0 * v + rng.uniform(-0.1, 0.1, hb)
            rows[b, v] = (4.0 + rng.uniform(-1, 1), rng.uniform(0.5, 2.0), rng.uniform(2.0, 4.0),
                          rng.uniform(0.3, 1.5), (2.0, np.inf)[(b + v) % 2],
                          (0, 1, hb, min(hb + 5, GM.MAX_HP))[(b + v) % 4], rng.uniform(0, 0.5))
        o_ = np.zeros((nO, 2, hb))
        for o in range(nO):
            o_[o, 0] = 3.0 * o + rng.uniform(-0.1, 0.1, hb)
            o_[o, 1] = -9.0 * (o + 1) + rng.uniform(-0.1, 0.1, hb)
        m_ = rng.uniform(0, 0.3, (nO, hb))
        # vehicle 0: the planted kind
        look = look_of(c, b, hb)
        if kind == "at_look":
            look = max(1, hb // 2)          # a step LOOK exists wherever hp_b >= 2
        if kind == "last" and look == 0:
            look = hb
        rows[b, 0, GM.LOOK] = look
        rows[b, 0, GM.J_MAX] = (2.0, np.inf)[(b // len(KINDS)) % 2]
        K = min(look, hb)
        if kind == "stop":
            x0[b, 0, 3], x0[b, 0, 4] = 0.3, -0.5
        elif kind == "clamp":
            x0[b, 0, 3], x0[b, 0, 4] = 0.02, 1.0
        elif kind == "still":
            x0[b, 0, 3], x0[b, 0, 4] = 0.0, -1.0
        at = {"k0": 0, "stop": 0, "still": 0, "last": K - 1, "at_look": look, "pair": 1}.get(kind)
        if at is not None and 0 <= at < hb:
            spot = t[at, :, 0] + (0.3, 0.2)
            if kind == "pair" and nV > 1:
                t[at, :, 1] = spot
                rows[b, 1, GM.LOOK] = hb       # vehicle 1 sees it too
            elif nO:
                o_[nO - 1, :, at] = spot
            elif nV > 1:
                t[at, :, nV - 1] = spot
        traj[b, :t.size] = t.reshape(-1)
        if nO:
            obst[b, :o_.size] = o_.reshape(-1)
            if margin is not None:
                margin[b, :m_.size] = m_.reshape(-1)
    return dict(rows=rows, x0=x0, traj=traj.reshape(B, Hm, 2, nV),
                obst=None if obst is None else obst.reshape(B, nO, 2, Hm),
                margin=None if margin is None else margin.reshape(B, nO, Hm), hp=hp,
                dreq_obs=dreq_obs, dreq_veh=dreq_veh, kind=kinds)


_mirror_cache = {}


def mirror(cid, fm=GM.F64, details=False):
    """(a_cmd, k_conf, clear) of the case on the mirror, computed once per number format and
    shared; with ``details`` the per-lane dict of ``governor_mirror.step`` instead."""
    key = (cid, fm.dtype)
    if key not in _mirror_cache:
        c, d, det = by_id(cid), inputs(cid), {}
        out = GM.step(d["rows"], d["x0"], d["traj"], d["obst"], d["margin"], d["hp"],
                      d["dreq_obs"], d["dreq_veh"], T_HOLD, T_BACK, c.hp_max, fm, det)
        _mirror_cache[key] = (out, det)
    return _mirror_cache[key][1 if details else 0]


# ---------------------------------------------------------------------------
# The comparison and its tolerance
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def yardsticks(cid):
    """(Y_a [B, nV], Y_c [B, nV]): the sums of the absolute terms of the two expressions, from
    the 80-bit mirror.  a_cmd: K_V (|V_REF| + |s|) + A_BRAKE + A_ACC + |a_now| + J_MAX t_hold
    (a finite J_MAX) + (|s| + |a_now| t_back) / t_hold.  clear: the distance of the pair that
    gives the minimum plus its required distance, margin and band (1 where nothing was
    examined or the minimum is -inf: ``governor_mirror.clearances``)."""
    d = inputs(cid)
    det = mirror(cid, GM.F80, details=True)
    rows, x0 = d["rows"], d["x0"]
    B, nV = rows.shape[:2]
    Ya, Yc = np.ones((B, nV)), np.ones((B, nV))
    for (b, v), e in det.items():
        r, s, a = rows[b, v], abs(x0[b, v, 3]), abs(x0[b, v, 4])
        if "clearances" not in e:
            continue
        j = r[GM.J_MAX] * T_HOLD if math.isfinite(r[GM.J_MAX]) else 0.0
        Ya[b, v] = r[GM.K_V] * (r[GM.V_REF] + s) + r[GM.A_BRAKE] + r[GM.A_ACC] + a + j \
            + (s + a * T_BACK) / T_HOLD
        if e["clearances"]:
            Yc[b, v] = float(min(e["clearances"], key=lambda t: t[1])[3])
    return Ya, Yc


def ratio(dev, mir, cid):
    """The one figure of the comparison: |d a_cmd| / Y_a and |d clear| / Y_c over the lanes,
    with ``mir`` the reference; NaN patterns and infinities must be identical."""
    f = lambda a: np.asarray(a, dtype=np.longdouble)
    Ya, Yc = yardsticks(cid)
    worst = 0.0
    for x, m, Y in ((f(dev[0]), f(mir[0]), Ya), (f(dev[2]), f(mir[2]), Yc)):
        assert (np.isnan(x) == np.isnan(m)).all()
        assert (np.isinf(x) == np.isinf(m)).all() and (x[np.isinf(m)] == m[np.isinf(m)]).all()
        ok = np.isfinite(m)
        if ok.any():
            x, m = np.where(ok, x, 0), np.where(ok, m, 0)
            worst = max(worst, float((np.abs(x - m)[ok] / Y[ok]).max()))
    return worst


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


# Tolerance of the device against the float64 mirror, in the figure of ``ratio``.  It is derived
# on the CPU from the reference alone (tests/test_governor_host.py,
# test_tolerance_is_sixteen_times_the_rounding_of_the_definition): the largest figure between
# the mirror in float64 and the mirror in 80-bit over the table is MIRROR_ROUNDING.  The device
# contracts multiply-adds and has its own sqrt and division: 16 times the figure, rounded up to
# a power of two.
# Per case: 1x0x3 2.4e-18, 1x1x1 1.984e-16, 1x3x10 1.58e-16 (1.08e-16 without margins), 4x0x20
# 1.15e-16, 5x2x10 1.80e-16 (1.17e-16), 16x32x64 1.10e-16, 3x2x30_mixed 1.18e-16.
MIRROR_ROUNDING = 1.99e-16
TOL = 2.0 ** -48                  # 16 * 1.99e-16 = 3.18e-15 <= 2^-48 = 3.55e-15


# ---------------------------------------------------------------------------
# The rollout scene in which stopping is the only way out
# ---------------------------------------------------------------------------
# One vehicle on the lane y = 0 from x = -18 m at 4 m/s, and one obstacle that stands still
# across the lane: 12 m long across it, 2 m wide along it, its centre STOP_AHEAD = 10 m ahead of
# the start.
#   - Wide enough: at the 3 degree steering limit the vehicle (wheelbase 0.68 m) turns on a
#     radius of 0.68 / tan(3 deg) = 12.97 m at best.  Its near face is 9 m ahead, the vehicle's
#     nose 0.49 m ahead of its centre: when the nose reaches the face, 8.51 m on, the tightest
#     circle has moved the centre 12.97 (1 - cos(asin(8.51 / 12.97))) = 3.2 m sideways, and the
#     obstacle reaches 6 m to either side (6.44 m with the vehicle's half width).  No plan
#     within the limit clears it, and at 4 m/s the nose is there after 2.1 s: six MPC steps.
#   - Far enough: the first command takes effect one MPC step after the start, 1.6 m on.  From
#     4 m/s at A_BRAKE = 3 m/s^2 the vehicle stops within 16 / 6 = 2.67 m plus the last, partial
#     step of the stop rule: 4.3 m in all, half of the 8.51 m there are.  The required centre
#     distance of this obstacle is 6.8 m (Scenarios.py:229-252), so the first plan's first point,
#     3.3 m on and 6.7 m from the centre, is already a conflict: LOOK = 3 sees it at step 0.
STOP_AHEAD = 10.0
STOP_LENGTH, STOP_WIDTH = 12.0, 2.0
STOP_A_BRAKE, STOP_LOOK = 3.0, 3
STOP_B, STOP_STEPS = 4, 9


def stop_scene(delay_x=0.0):
    """(scenario, x_init [B, 1, 6], governor rows as keywords of ``governor.rows``);
    ``delay_x``: the scene with a measurement delay."""
    _paths()
    from oracle import scp_reference as R
    sc = R.OracleScenario(Hp=10, Hu=10, delay_x=delay_x)
    sc.add_vehicle(-18.0, 0.0, 0.0, [[-100.0, 0.0], [100.0, 0.0]])
    sc.obstacles.append(np.array([-18.0 + STOP_AHEAD, 0.0, math.pi / 2, 0.0, STOP_LENGTH,
                                  STOP_WIDTH]))
    sc.complete()
    rng = np.random.default_rng(12)
    x_init = np.array(sc.x0, float)[None] + rng.standard_normal((STOP_B, 1, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])
    kw = dict(v_ref=4.0, a_acc=1.0, a_brake=STOP_A_BRAKE, k_v=0.5, look=STOP_LOOK)
    return sc, x_init, kw
