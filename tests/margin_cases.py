"""The inputs of the obstacle-margin tests, shared by the CPU tests (tests/test_margin_host.py:
the input conditions and the tolerance are pinned there, on the mirrors alone) and the GPU
tests (tests/test_gpu_margin.py), so that both see exactly the same numbers.

Solver input (scpqp_solve_margin, scpqp_evaluate_margin).  8 problems ``BT.make_batch(sc, 8, base_seed=303)``
per shape, with the margin

    m[b][o][k] = 0.6 * ((o + b) % 3) / 2 * sqrt((k + 1) / hp_b)     (0, 0.3 or 0.6 m at the end)

The four frog shapes are the four obstacle-reaching rows of tests/dispatch_cases.py (one solve
kernel each); frog 1 x 10 starts 8 m further along its lane, since from the stock start no
obstacle row is active within ten steps and any margin passes.  parallel 5 x 10 has obstacle rows
next to pair rows and the obstacle quirk's repetitions.  The mixed run is frog 1 x 29 at the
horizons (29, 15, 5).  On the mirror alone (tests/margin_solver_mirror.py; pinned by
test_margin_host.py::test_solver_case_conditions): every QP certified, no problem at the
20-iteration cap; on the frog shapes n_scp >= 4, the last QP has >= 2 active rows
(|b - A z| < 1e-7) and the margin moves every problem's u by more than 1e-3 rad.

Margin step (scpqp_obstacles_margin).  The lanes of tests/imm_cases.py after its eight steps on
the float64 mirror, M = 1 .. 4, three shapes."""
from __future__ import annotations

import functools
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

N_PROBLEMS = 8
BASE_SEED = 303
ACTIVE_TOL = 1e-7
MOVE_MIN = 1e-3            # rad: the margin must move every frog problem's u by more


def _paths():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (here, root, os.path.join(root, "senquential-convex-programming-for-trajectory-planning_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


@dataclass(frozen=True)
class Case:
    scenario: str            # "frog" or "parallel"
    n_veh: int
    hp_max: int
    kernel: tuple            # (HG, VG, RM, OCC, SH) of the shape (tests/dispatch_cases.py)
    shift: float = 0.0       # added to every start x
    hps: tuple = None        # the mixed-horizon run: problem g at hps[g % len(hps)]

    @property
    def id(self):
        return f"{self.scenario}{self.n_veh}x{self.hp_max}" + ("_mixed" if self.hps else "")

    @property
    def frog(self):
        return self.scenario == "frog"


CASES = (
    Case("frog", 1, 10, (0, 0, 1, 3, 0), shift=8.0),
    Case("frog", 1, 20, (0, 1, 1, 3, 0)),
    Case("frog", 1, 22, (0, 0, 1, 2, 0)),
    Case("frog", 1, 29, (0, 1, 1, 2, 0)),
    Case("parallel", 5, 10, (0, 1, 1, 3, 0)),
    Case("frog", 1, 29, (0, 1, 1, 2, 0), hps=(29, 15, 5)),
)
IDS = [c.id for c in CASES]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def scenario(c):
    _paths()
    from oracle import scp_reference as R
    return R.frog_scenario(Hp=c.hp_max) if c.frog else R.parallel_scenario(c.n_veh, Hp=c.hp_max)


def margin_of(nO, hp, b):
    """m [nO, hp] of problem b at horizon hp."""
    o, k = np.arange(nO)[:, None], np.arange(hp)[None, :]
    return 0.6 * ((o + b) % 3) / 2 * np.sqrt((k + 1) / hp)


def inputs(c):
    """(scenario, batch, margin slots [B, nO, hp_max]: problem b's [nO][hp_b] packed as the
    prefix of its slot, zeros behind it)."""
    _paths()
    from scpqp import batch as BT
    sc = scenario(c)
    bt = BT.make_batch(sc, N_PROBLEMS, base_seed=BASE_SEED, mixed_hp=c.hps)
    assert bt.hp_max == c.hp_max
    bt.x0[:, :, 0] += c.shift
    mg = np.zeros((N_PROBLEMS, sc.nObst * c.hp_max))
    for b in range(N_PROBLEMS):
        m = margin_of(sc.nObst, int(bt.hp[b]), b).reshape(-1)
        mg[b, :m.size] = m
    return sc, bt, mg.reshape(N_PROBLEMS, sc.nObst, c.hp_max)


def problem(sc, bt, b):
    _paths()
    from oracle import scp_reference as R
    H = int(bt.hp[b])
    obst = bt.obst[b].reshape(-1)[:sc.nObst * 2 * H].reshape(sc.nObst, 2, H)
    return R.make_problem(sc, bt.x0[b], bt.u0[b], bt.ec_noise[b], Hp=H, obst=obst)


def mirror_job(args):
    """One problem on the margin-aware mirror, for a spawn pool: (cid, b, with_margin) ->
    the SCPResult with its history (the row matrices replaced by the count of active rows of
    the last QP) and the evaluation's c_obs of the returned u."""
    _paths()
    import margin_solver_mirror as MS
    import scp_parity as SP
    SP.single_thread_blas()
    cid, b, with_margin = args
    c = by_id(cid)
    sc, bt, mg = inputs(c)
    p = problem(sc, bt, b)
    m = margin_of(sc.nObst, int(bt.hp[b]), b) if with_margin else None
    r = MS.scp_solve(p, m)
    last = r.history[-1]
    r.active = int(np.sum(np.abs(last["b"] - last["A"] @ last["z"]) < ACTIVE_TOL))
    for h in r.history:
        del h["A"], h["b"], h["u_lin"]
    r.c_obs = r.evaluation.c_obs
    r.lin = r.evaluation = None
    return r


def mirror_jobs(cid, with_margin=True):
    return [(cid, b, with_margin) for b in range(N_PROBLEMS)]


# ---------------------------------------------------------------------------
# The margin step
# ---------------------------------------------------------------------------
SHAPES = [(12, 22, 10), (2, 3, 5), (1, 1, 1)]          # (B, n_obst, hp): tests/imm_cases.py
MODES = (1, 2, 3, 4)
P_MISS = 0.05
M_MAX = 1e3                # metres: far above every margin of the cases, so nothing is capped


@functools.lru_cache(maxsize=None)
def states(B, nO, hp, M):
    """(trk [B, nO, M, 14], x [B, nO, M, 6], cov [B, nO, M, 6, 6], mu [B, nO, M]) float64: the
    bank of ``imm_cases.case`` and its state after the eight steps on the float64 mirror.  The
    off lanes were never initialised (x NaN), the bad lanes are NaN throughout."""
    _paths()
    import imm_cases as IC
    import imm_mirror as IM
    trk = IC.case(B, nO, M)[3]
    x, cov, mu = IC.run_mirror(B, nO, hp, M, IM.F64)[-1][:3]
    return (np.asarray(trk, float), np.asarray(x, float), np.asarray(cov, float),
            np.asarray(mu, float))


def lead_dt():
    _paths()
    import imm_cases as IC
    return IC.LEAD, IC.DT


def ratio(dev, mir):
    """The one figure of the comparison: |d margin| / max(1, margin) and |d Sigma_ij| /
    max(1, Sxx + Syy) over (margin, Sigma); NaN patterns must be identical.  ``mir`` is the
    reference."""
    f = lambda a: np.asarray(a, dtype=np.longdouble)
    (dm, ds), (mm, ms) = (f(dev[0]), f(dev[1])), (f(mir[0]), f(mir[1]))
    assert (np.isnan(dm) == np.isnan(mm)).all() and (np.isnan(ds) == np.isnan(ms)).all()
    worst = 0.0
    ok = ~np.isnan(mm)
    if ok.any():
        worst = float((np.abs(dm - mm)[ok] / np.maximum(1.0, np.abs(mm[ok]))).max())
    tr = np.maximum(1.0, ms[..., 0] + ms[..., 2])[..., None] * np.ones(3)
    ok = ~np.isnan(ms)
    if ok.any():
        worst = max(worst, float((np.abs(ds - ms)[ok] / tr[ok]).max()))
    return worst


# Tolerance of the device against the mirror, in the figure of ``ratio``.  It is derived on the
# CPU from the reference alone (tests/test_margin_host.py,
# test_tolerance_is_sixteen_times_the_rounding_the_definition_amplifies): the largest figure
# between the mirror in float64 and the mirror in 80-bit on ``states``, over the three shapes
# and M = 1 .. 4, with kappa = kappa_for(P_MISS) and m_max = M_MAX, is MIRROR_ROUNDING.  The
# device contracts multiply-adds, has its own sincos, sqrt and hypot and sums in another order:
# 16 times the figure, rounded up to a power of two.
# Per shape, the largest over M: (12, 22, 10) 3.52e-14 (at M = 3), (2, 3, 5) 1.68e-14,
# (1, 1, 1) 2.3e-16.
MIRROR_ROUNDING = 3.52e-14
TOL = 2.0 ** -40                  # 16 * 3.52e-14 = 5.63e-13 <= 2^-40 = 9.09e-13


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


# ---------------------------------------------------------------------------
# Calibration: 100 filtered lanes of ``tracker_accel_cases.consistency_inputs`` (20 x 5, twelve
# steps on the float64 mirror), 200 states drawn from N(x, P) of each and pushed through the
# mirror horizon: 20 000 points per horizon step.
# ---------------------------------------------------------------------------
CAL_B, CAL_NO, CAL_DRAWS = 20, 5, 200
CAL_SEED = 2041
# the share of the 20 000 points of a horizon step farther from c[k] than the margin at
# kappa_for(0.05): at most 0.05 plus three standard deviations of a share of 0.05 over 20 000
CAL_BOUND = 0.05 + 3.0 * math.sqrt(0.05 * 0.95 / 20000)
# the covariances of the filtered lanes are used as they are (scale 1): see the host test
CAL_P_SCALE = 1.0
