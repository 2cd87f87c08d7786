"""Closed-loop Monte-Carlo rollouts on the GPU (main.py:98-206).

``ClosedLoopBatch`` runs ``Simulation.runsimulation`` with the SCP controller
for B independent realisations of one scenario at once.  Per MPC step i:

1. measurement, steering limits and the held command (main.py:101-117, 105-108)
2. delay compensation, ``IterClass`` (MPC_Iter.py:24-33)   -> scpqp_delay_compensate
3. the SCP solve, warm-started from the previous step's u  -> scpqp_solve
   (SCP_controller.py:42-43)
4. steering-limit enforcement (main.py:164-174)            -> scpqp_clip_controls
5. actuator-delayed control path and the plant over one step (main.py:176-191)
                                                            -> scpqp_plant_step
6. evaluateInOriginalProblem of the step (main.py:201-202, SCP_controller.py:343-400)
                                                            -> device tensor ops
7. with ``metrics=True``: footprint gaps, collisions, margins to dsafe and cross-track
   errors along the step's realised path, merged into a per-realisation accumulator
   (scpqp/metrics.py)                                       -> scpqp_metrics_accumulate

All state lives on the device (torch-ROCm tensors); the per-step index
bookkeeping (which tick is measured, which control tick each plant output
reads) is the same for every realisation and is computed on the host once
per step, exactly as main.py computes it.  Realisations differ by their
initial state and, with ``reset(..., seed=)``, by the reference's model noise
(Model.py:84-86): drawn on the device per right-hand-side evaluation from a
counter-based generator (include/scpqp_noise.h), reproducible from the seed and
independent of how the realisations are sharded.  ``noise=`` instead holds a
caller-made constant pair per vehicle over the whole rollout.  ``reset(..., truth=)``
gives the plant of every (realisation, vehicle) its own geometry, steering lag, gain and
offset (include/scpqp_truth.h), unknown to the controller.  ``reset(..., obstacles=)``
gives every (realisation, obstacle) its own start pose, speed, footprint and turn rate
(include/scpqp_obstacles.h); the controller extrapolates what it measures on a straight line.
``reset(..., sensing=, obstacle_sensing=)`` makes what the controller measures of the vehicles
and the obstacles noisy, biased, late or lost (include/scpqp_sensing.h).
``reset(..., estimator=)`` puts an extended Kalman filter per (realisation, vehicle) between
that measurement and the delay compensation (include/scpqp_estimator.h).
``reset(..., tracker=)`` puts one per (realisation, obstacle) between the obstacle measurement
and the obstacle prediction (include/scpqp_tracker.h).
``reset(..., manoeuvres=)`` makes the obstacles brake, accelerate and turn in pieces on top of
their rows (include/scpqp_manoeuvres.h); the controller measures them as before and knows
nothing of the schedule.
``reset(..., tracker_accel=)`` puts the filter that also estimates the acceleration in the
tracker's place (include/scpqp_tracker_accel.h): it runs on one manoeuvre piece and predicts a
horizon that brakes to a stop.
``reset(..., governor=)`` commands the acceleration state of every (realisation, vehicle) from
the step's own plan (include/scpqp_governor.h): brake on a predicted conflict, else return to
the cruise speed.
``reset(..., right_of_way=)`` puts the governor with ranks and graded braking in its place
(include/scpqp_yield.h): in a conflict between two vehicles only the outranked one yields, with
a deceleration sized to stop before the conflict.
``reset(..., drive=)`` puts a longitudinal actuator per (realisation, vehicle) between that
command and the plant (include/scpqp_drive.h): gain, offset, limits, a lag and the hold rule,
none of which the controller or the governor knows.
"""
from __future__ import annotations

import json
import math
import time

import numpy as np
import torch

from . import plant as PL
from .solver import ScpQpSolver

LATERAL_ACC_LIMIT = 9.81 / 2      # Scenarios.py:48
CONSTRAINT_TOL = 2 * 2.1 * 1e-3   # Config.py:18


def evaluate_in_original_problem(scenario, U, traj, ref_points, obst_future=None,
                                 tol=CONSTRAINT_TOL, variants=None, variant_of=None,
                                 obst_margin=None):
    """SCPcontroller.evaluateInOriginalProblem (SCP_controller.py:343-400) for a
    batch, on the device: U [B, Hp, nVeh] (the clipped controller output),
    traj [B, Hp, 2, nVeh] (trajectory prediction), ref_points [B, Hp, 2, nVeh],
    obst_future [B, nObst, 2, Hp] or None.  Returns tensors: the objective terms
    [B], constraint values [B, nVeh, nVeh, Hp] / [B, nVeh, nObst, Hp] and
    predictionFeasible [B] (from the predicted trajectory, as the reference).
    With ``variants`` (a list of scenarios) and ``variant_of`` (an integer device tensor
    [B]), realisation b is weighed with the Q, Q_final, R and dsafe tables of
    ``variants[variant_of[b]]`` instead of ``scenario``'s.  ``obst_margin`` [B, nObst, Hp]
    (scpqp/margin.py): metres added to the obstacle safety distances, as the solve adds them."""
    dev = U.device
    f = dict(dtype=torch.float64, device=dev)
    nV = U.shape[2]
    scs = [scenario] if variants is None else list(variants)

    def table(get):
        # [1, ...] of the scenario, or [B, ...] gathered per realisation
        t = torch.as_tensor(np.stack([np.asarray(get(sc), float) for sc in scs]), **f)
        return t if variants is None else t[variant_of.long()]

    Q = table(lambda sc: [float(q) for q in sc.Q])
    Qf = table(lambda sc: [float(q) for q in sc.Q_final])
    Rw = table(lambda sc: [float(r) for r in sc.R])
    err2 = (ref_points - traj) ** 2                                  # [B, Hp, 2, nV]
    objx = (err2[:, :-1].sum(dim=(1, 2)) * Q).sum(-1) + (err2[:, -1].sum(dim=1) * Qf).sum(-1)
    obju = ((U ** 2).sum(dim=1) * Rw).sum(-1)
    ds2 = table(lambda sc: np.asarray(sc.dsafeVehicles, float) ** 2)   # [1 | B, nV, nV]
    p = traj.permute(0, 3, 2, 1)                                     # [B, nV, 2, Hp]
    d2 = ((p[:, :, None] - p[:, None, :]) ** 2).sum(3)               # [B, nV, nV, Hp]
    cv = ds2[:, :, :, None] - d2
    eye = torch.eye(nV, dtype=torch.bool, device=dev)[None, :, :, None]
    cv = torch.where(eye, torch.zeros_like(cv), cv)                  # diagonal stays 0
    viol = (cv > tol).flatten(1).any(1)
    out = dict(predictionObjectiveValueX=objx, predictionObjectiveValueU=obju,
               predictionObjectiveValue=objx + obju, constraintValuesVehicle=cv)
    if obst_future is not None and obst_future.shape[1] > 0:
        dso = table(lambda sc: np.asarray(sc.dsafeObstacles, float).reshape(nV, -1) ** 2)
        d2o = ((p[:, :, None] - obst_future[:, None]) ** 2).sum(3)   # [B, nV, nO, Hp]
        if obst_margin is not None:
            dsm = table(lambda sc: np.asarray(sc.dsafeObstacles, float).reshape(nV, -1))
            co = (dsm[:, :, :, None] + obst_margin[:, None]) ** 2 - d2o
        else:
            co = dso[:, :, :, None] - d2o
        viol = viol | (co > tol).flatten(1).any(1)
        out["constraintValuesObstacle"] = co
    out["predictionFeasible"] = ~viol
    return out


def held_command_tick(tick_now, tdx, tdu, tps, ticks_total):
    """u_path[:, -1] of main.py:101-117 (the command IterClass holds over the
    delay, MPC_Iter.py:29-32): the controlPathFullRes tick it copies, or None
    when the slice is truncated at the end of the simulation and u_path[:, -1]
    keeps its zero initialisation."""
    tick_meas = max(0, tick_now - tdx)
    tick_act = min(ticks_total + 1, tick_now + 1 + tdu + tps)
    n_path = tdx + tps + tdu
    lo = max(tdx - tick_now, 0)
    hi = lo + tick_act - 1 - tick_meas
    if hi < n_path:
        return None
    return tick_meas + 1 + (n_path - 1 - lo)


# what every variant of a rollout shares with its scenario: the plant kernels, the held
# command and the per-step tick bookkeeping are computed once for the whole batch
SHARED_ATTRS = ("Lf", "Lr", "u0", "mechanicalSteeringLimit", "Hp", "dt", "tick_length", "delay_x",
                "delay_u", "ticks_delay_x", "ticks_delay_u", "ticks_per_sim", "ticks_total", "Nsim")


def check_shared(scenario, variants):
    """ValueError naming the first attribute of SHARED_ATTRS in which a variant differs."""
    for k, sc in enumerate(variants):
        for name in SHARED_ATTRS:
            a, b = getattr(scenario, name), getattr(sc, name)
            if not np.array_equal(np.asarray(a, float).reshape(-1), np.asarray(b, float).reshape(-1)):
                raise ValueError(f"variant {k} differs from the scenario in {name}: every "
                                 f"realisation of a rollout shares it")


class ClosedLoopBatch:
    def __init__(self, scenario, B, device=None, h_max=PL.H_MAX, keep_path=False, evaluate=True,
                 timing=False, trace=False, metrics=False, variants=None, variant_of=None,
                 **solver_kw):
        """``variants`` (a list of scenarios) with ``variant_of`` [B]: realisation b runs
        scenario ``variants[variant_of[b]]``: its solve and metrics parameters, its obstacle
        set and its evaluation weights.  ``scenario`` supplies what all of them share
        (SHARED_ATTRS); a variant that differs there is rejected."""
        self.sc = scenario
        self.B = int(B)
        self.device = torch.device(device or "cuda")
        self.variants = None if variants is None else list(variants)
        self.variant_of = None
        if self.variants is None:
            if variant_of is not None:
                raise ValueError("variant_of needs variants")
        else:
            if variant_of is None:
                raise ValueError("variants needs variant_of [B]")
            vo = np.asarray(variant_of.cpu() if isinstance(variant_of, torch.Tensor)
                            else variant_of).reshape(-1)
            if vo.shape[0] != self.B:
                raise ValueError("variant_of must hold B entries")
            if vo.min() < 0 or vo.max() >= len(self.variants):
                raise ValueError("variant_of indexes outside variants")
            check_shared(scenario, self.variants)
            for k, sc in enumerate(self.variants):
                if int(sc.nVeh) != int(scenario.nVeh) or int(sc.nObst) != int(scenario.nObst):
                    raise ValueError(f"variant {k} differs from the scenario in nVeh / nObst")
            self.variant_of = torch.as_tensor(vo.astype(np.int32), device=self.device)
        self.nV, self.Hp = int(scenario.nVeh), int(scenario.Hp)
        self.tps = int(scenario.ticks_per_sim)
        self.ticks_total = int(scenario.ticks_total)
        self.tdx, self.tdu = int(scenario.ticks_delay_x), int(scenario.ticks_delay_u)
        if self.tdx > self.tps:
            raise ValueError("measurement delay longer than one MPC step is not supported")
        self.h_max = h_max
        self.keep_path = keep_path
        self.evaluate = evaluate
        self.timing = timing
        self.nO = int(scenario.nObst)
        self.obstacles = np.asarray(scenario.obstacles, float).reshape(self.nO, -1) if self.nO \
            else np.zeros((0, 6))
        # per variant its own obstacle set (result_for_plot draws self.obstacles: variant-free)
        self.var_obstacles = None
        if self.variants is not None and self.nO:
            self.var_obstacles = [np.asarray(sc.obstacles, float).reshape(self.nO, -1)
                                  for sc in self.variants]
        self.params = PL.plant_params(scenario.Lf, scenario.Lr)
        self.solver = ScpQpSolver(scenario, max_batch=self.B, device=self.device,
                                  variants=self.variants, **solver_kw)
        self.du_lim = float(scenario.mechanicalSteeringLimit) * 2          # Scenarios.py:50
        f = dict(dtype=torch.float64, device=self.device)
        self.L = torch.tensor([float(a) + float(b) for a, b in zip(scenario.Lf, scenario.Lr)], **f)
        self.control = torch.full((self.B, self.nV, self.ticks_total + 1), float("nan"), **f)
        self.state = torch.zeros((self.B, self.nV, 6), **f)
        self.last_path = None          # [B, nV, tps + 1, 6] of the previous step
        self.u_prev = None
        self.obst_rows = None          # the obstacle truth of reset(..., obstacles=)
        self.sense_rows = None         # the sensing truth of reset(..., sensing=)
        self.osense_rows = None        # and of reset(..., obstacle_sensing=)
        self.x_held = None
        self.est_rows = None           # the estimator tuning of reset(..., estimator=)
        self.trk_rows = None           # the tracker tuning of reset(..., tracker=)
        self.man_rows = None           # the manoeuvre schedule of reset(..., manoeuvres=)
        self.trka_rows = None          # the tracker tuning of reset(..., tracker_accel=)
        self.imm_rows = None           # the bank (trk, sw) of reset(..., imm=)
        self.margin = None             # (kappa, m_max) of reset(..., margin=)
        self.obst_margin = None
        self.gov_rows = None           # the governor tuning of reset(..., governor=)
        self.yld_rows = None           # the tuning of reset(..., right_of_way=)
        self.drive_rows = None         # the drive truth of reset(..., drive=)
        self.a_cmd = None              # with it: the acceleration command in force [B, nVeh]
        self.trace = trace     # keep every step's solve inputs and per-SCP-iteration trace
        self.out = self.solver.alloc_out(self.B, trace=trace)
        self.history = []
        # realised-path metrics (scpqp/metrics.py); off: nothing is allocated or launched
        self.path_metrics = None
        if metrics:
            from .metrics import PathMetrics
            self.path_metrics = PathMetrics(scenario, self.B, self.device, variants=self.variants)

    def reset(self, x_init, noise=None, seed=None, sigma=PL.SIGMA_NOISE, b_offset=0, truth=None,
              obstacles=None, sensing=None, obstacle_sensing=None, sense_seed=None,
              estimator=None, tracker=None, manoeuvres=None, tracker_accel=None, imm=None,
              margin=None, governor=None, right_of_way=None, drive=None):
        """main.py:73-75: vehiclePathFullRes[:, v, 0] = x0; the control path holds
        scenario.u0 for the first ticks_delay_u + ticks_per_sim + 1 ticks.

        ``seed``: run with the reference's model noise (Simulation(..., isNoise);
        Model.py:84-86), drawn on the device per right-hand-side evaluation: step i uses
        epoch i for its delay compensation, its plant step and the ec_noise of its solve.
        Realisation b draws as global realisation ``b_offset + b``, so a batch sharded
        over ranks (b_offset = rank * per_rank) computes what one large batch would.

        ``truth`` [B, nVeh, 5] (scpqp/truth.py; include/scpqp_truth.h): the plant that
        realises the path has these parameters per (realisation, vehicle).  Only the plant
        step reads them: the delay compensation, the solve, the steering limit and the
        evaluation keep the scenario's nominal model (main.py:121-123).  Validated here,
        before anything is launched; None: nothing is allocated and the nominal kernels run.

        ``obstacles`` [B, nObst, 7] (scpqp/obstacles.py; include/scpqp_obstacles.h): every
        (realisation, obstacle) moves by its own row: start pose, speed, footprint and a
        constant turn rate.  The controller measures the true pose and extrapolates it on a
        straight line, on the device (scpqp_obstacles_predict); the metrics and
        ``result_for_plot`` follow the row.  With ``variants`` the rows replace the variants'
        obstacle sets and the dsafe tables stay per variant.  Validated here, before anything
        is launched: a refused reset changes nothing.  None: the scenario's constant
        obstacles, predicted on the host as before.

        ``sensing`` [B, nVeh, 8] (scpqp/sensing.py; include/scpqp_sensing.h): what the
        controller measures of every (realisation, vehicle) is noisy, biased, scaled, late or
        lost, drawn per step on the device from ``sense_seed`` (epoch i, realisation
        ``b_offset + b``).  Only the measurement changes: the steering limit keeps reading the
        realised speed, and the delay compensation, the solve, the plant and the metrics are
        what they were.  ``obstacle_sensing`` [B, nObst, 3]: noise on the obstacle pose and
        speed the controller extrapolates; it needs ``obstacles=`` rows, which stay the truth
        of the world.  Both are validated here, before anything is launched; None: the lines
        of the exact sensor run, and nothing is allocated.

        ``estimator`` [B, nVeh, 8] (scpqp/estimator.py; include/scpqp_estimator.h): an extended
        Kalman filter per (realisation, vehicle) takes the step's measurement, exact or of
        ``sensing=``, and its estimate replaces the measurement as the input of the delay
        compensation.  It predicts over the ticks since the previous measurement with the
        nominal model and the commands this controller issued.  The steering limit keeps
        reading the realised speed; the solve, the plant, the metrics and the evaluation are
        what they were.  Validated here, before anything is launched; None: nothing is
        allocated and the measurement goes to the delay compensation as before.

        ``tracker`` [B, nObst, 9] (scpqp/tracker.py; include/scpqp_tracker.h): an extended
        Kalman filter per (realisation, obstacle) takes the step's obstacle measurement, exact
        or of ``obstacle_sensing=``, estimates the turn rate, and its prediction on the arc of
        the estimate replaces the straight extrapolation as the solve's ``obst``.  It needs
        ``obstacles=`` rows.  The world (metrics, plotted paths) keeps the true rows.
        Validated here, before anything is launched; None: nothing is allocated or launched
        and the prediction is what it was.

        ``manoeuvres`` [B, nObst, 4, 3] (scpqp/manoeuvres.py; include/scpqp_manoeuvres.h): every
        (realisation, obstacle) accelerates and turns in up to four pieces on top of its row.
        It needs ``obstacles=`` rows.  The controller measures the true pose and the true
        current speed at the measurement tick (the snapshot row, recorded as ``obst_state``)
        and predicts from them as before: exact, sensed or tracked.  The metrics and
        ``result_for_plot`` follow the schedule.  Validated here, before anything is launched;
        None, or a schedule in which no piece does anything: nothing is allocated or launched
        and the rollout is what it was.

        ``tracker_accel`` [B, nObst, 14] (scpqp/tracker_accel.py;
        include/scpqp_tracker_accel.h): the six-state filter per (realisation, obstacle) that
        also estimates the acceleration, runs on one manoeuvre piece and predicts a horizon
        that brakes to a stop.  It takes the place of ``tracker=`` (the two together are
        refused), needs ``obstacles=`` rows, sees the same measurement and the same draws,
        and records the same keys (``obst_est`` is six wide).  Validated here, before
        anything is launched; None, or a tuning in which every row is off: nothing is
        allocated or launched and the rollout is what it was.

        ``imm`` = (trk [B, nObst, M, 14], sw [B, nObst, M + 1, M]) (scpqp/imm.py;
        include/scpqp_imm.h): a bank of M six-state filters per (realisation, obstacle) whose
        probability-weighted prediction becomes the solve's ``obst``.  It takes the place of
        ``tracker=`` and ``tracker_accel=`` (together with either it is refused), needs
        ``obstacles=`` rows, and sees the same measurement and the same draws.  The record
        gains ``obst_est`` (the combined estimate, six wide), ``obst_mu`` and ``obst_nis``
        ([B, nObst, M]) and ``obst_meas``.  Validated here, before anything is launched; None,
        or a bank in which every row is off: nothing is allocated or launched and the rollout
        is what it was.

        ``margin`` = (kappa, m_max) (scpqp/margin.py; include/scpqp_margin.h): after every
        tracker step the tracker's covariances become a safety margin per (realisation,
        obstacle, horizon step), ``min(kappa sigma, m_max)`` metres, which the solve (and the
        evaluation of ``evaluate=True``) adds to its obstacle safety distances.  It needs
        ``tracker_accel=`` or ``imm=`` (the five-state ``tracker=`` has no acceleration row).
        The record gains ``obst_margin`` [B, nObst, Hp].  The realised-path metrics stay what
        they are: they measure the truth, not the inflated distance.  None: the rollout is
        what it was; ``(0, m_max)`` gives the same rollout bitwise.

        ``governor`` [B, nVeh, 7] (scpqp/governor.py; include/scpqp_governor.h): after the solve
        of step i the governor looks at that step's plan (``x0``, ``traj``, the ``obst`` and the
        margins the solve was given, the required distances of each realisation's variant,
        ``t_hold = dt``, ``t_back = delay_u``) and commands an acceleration, which becomes the
        plant's ``x[4]`` at the start of step i + 1: the one-step compute delay the steering has,
        and no transport delay of its own.  Column 4 of the delay compensation's input is the
        acceleration in force at the step's first tick, after the sensor and the estimator: the
        controller issued that command and knows it.  The record gains ``accel_cmd``,
        ``gov_k_conf`` and ``gov_clear`` [B, nVeh].  The steering limit keeps reading the
        realised speed (at speed 0 it is the mechanical limit).  Validated here, before
        anything is launched; None, or a tuning in which every row is off: nothing is allocated
        or launched and the rollout is what it was.

        ``right_of_way`` [B, nVeh, 10] (scpqp/yielding.py; include/scpqp_yield.h) takes the
        governor's place in the step: the same inputs, ``t_hold`` and ``t_back``, the same write
        of ``state[:, :, 4]`` and the same column-4 rule for the delay compensation, with a rank
        per vehicle and a deceleration sized to stop before the conflict.  Passing it together
        with ``governor`` is refused.  The record gains ``accel_cmd``, ``gov_k_conf``,
        ``gov_clear``, ``gov_k_any``, ``gov_who`` and ``gov_d_stop`` [B, nVeh].  Validated here,
        before anything is launched; None, or every row off: nothing is allocated or launched
        and the rollout is what it was.

        ``drive`` [B, nVeh, 6] (scpqp/drive.py; include/scpqp_drive.h): the longitudinal
        actuator of every (realisation, vehicle).  It needs ``governor=`` or ``right_of_way=``:
        without one nothing commands the acceleration.  The command then lives in its own
        tensor ``a_cmd`` [B, nVeh], initialised from ``x_init[:, :, 4]`` and replaced by the
        governor's output at the end of each step, and ``state[:, :, 4]`` is the realised
        acceleration, which the governor no longer writes.  The controller side never sees the
        realised acceleration: column 4 of what the sensor, the estimator and the delay
        compensation are handed is the command in force from the measured tick on (the new
        command at the step's first tick, the previous step's inside the previous step),
        which is what those columns hold without a drive.  The steering limit keeps reading the
        realised speed.  The record gains ``accel_real`` [B, nVeh], the realised acceleration
        at the step's end.  Validated here, before anything is launched; None, or every row
        ideal: nothing is allocated or launched and the rollout is what it was."""
        if drive is not None:
            from . import drive as DRV
            if governor is None and right_of_way is None:
                raise ValueError("drive needs governor= or right_of_way=: without one nothing "
                                 "commands the acceleration")
            dv = drive.detach().cpu().numpy() if isinstance(drive, torch.Tensor) \
                else np.asarray(drive, float)
            if tuple(dv.shape) != (self.B, self.nV, DRV.NP):
                raise ValueError(f"drive must be [B, nVeh, 6] = [{self.B}, {self.nV}, 6]")
            DRV.validate(dv, self.h_max)
            if DRV.is_ideal(dv):
                drive = None
        if right_of_way is not None:
            from . import yielding as YLD
            if governor is not None:
                raise ValueError("right_of_way takes the governor's place: pass one of "
                                 "governor= and right_of_way=")
            yv = right_of_way.detach().cpu().numpy() if isinstance(right_of_way, torch.Tensor) \
                else np.asarray(right_of_way, float)
            if tuple(yv.shape) != (self.B, self.nV, YLD.NP):
                raise ValueError(f"right_of_way must be [B, nVeh, 10] = [{self.B}, {self.nV}, 10]")
            YLD.validate(yv)
            if YLD.is_off(yv):
                right_of_way = None
        if governor is not None:
            from . import governor as GOV
            gv = governor.detach().cpu().numpy() if isinstance(governor, torch.Tensor) \
                else np.asarray(governor, float)
            if tuple(gv.shape) != (self.B, self.nV, GOV.NP):
                raise ValueError(f"governor must be [B, nVeh, 7] = [{self.B}, {self.nV}, 7]")
            GOV.validate(gv)
            if GOV.is_off(gv):
                governor = None
        if margin is not None:
            from . import margin as MG
            if tracker_accel is None and imm is None:
                raise ValueError("margin needs tracker_accel= or imm=: the margin is taken from "
                                 "a six-state tracker's covariance")
            try:
                kappa, m_max = margin
            except (TypeError, ValueError):
                raise ValueError("margin must be a pair (kappa, m_max)") from None
            margin = MG.validate(kappa, m_max)
        if imm is not None:
            from . import imm as IMM
            if tracker is not None or tracker_accel is not None:
                raise ValueError("pass one of tracker=, tracker_accel= and imm=, not several")
            if obstacles is None:
                raise ValueError("imm needs obstacles= rows: pass "
                                 "obstacles.nominal(scenario, B) for the scenario's own")
            try:
                imm_trk, imm_sw = imm
            except (TypeError, ValueError):
                raise ValueError("imm must be a pair (trk, sw)") from None
            it, isw = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor)
                       else np.asarray(a, float) for a in (imm_trk, imm_sw))
            if it.ndim != 4 or tuple(it.shape[:2]) != (self.B, self.nO) or it.shape[3] != IMM.NP:
                raise ValueError(f"imm trk must be [B, nObst, M, 14] = [{self.B}, {self.nO}, M, 14]")
            IMM.validate(it, isw)
            if IMM.is_off(it):
                imm = None
        if tracker_accel is not None:
            from . import tracker_accel as TRKA
            if tracker is not None:
                raise ValueError("pass either tracker= or tracker_accel=, not both")
            if obstacles is None:
                raise ValueError("tracker_accel needs obstacles= rows: pass "
                                 "obstacles.nominal(scenario, B) for the scenario's own")
            ta = tracker_accel.detach().cpu().numpy() if isinstance(tracker_accel, torch.Tensor) \
                else np.asarray(tracker_accel, float)
            if tuple(ta.shape) != (self.B, self.nO, TRKA.NP):
                raise ValueError(f"tracker_accel must be [B, nObst, 14] = [{self.B}, {self.nO}, 14]")
            TRKA.validate(ta)
            if TRKA.is_off(ta):
                tracker_accel = None
        if manoeuvres is not None:
            from . import manoeuvres as MAN
            if obstacles is None:
                raise ValueError("manoeuvres needs obstacles= rows: pass "
                                 "obstacles.nominal(scenario, B) for the scenario's own")
            mn = manoeuvres.detach().cpu().numpy() if isinstance(manoeuvres, torch.Tensor) \
                else np.asarray(manoeuvres, float)
            if tuple(mn.shape) != (self.B, self.nO, MAN.NSEG, MAN.NF):
                raise ValueError(f"manoeuvres must be [B, nObst, 4, 3] = [{self.B}, {self.nO}, 4, 3]")
            ob = obstacles.detach().cpu().numpy() if isinstance(obstacles, torch.Tensor) \
                else np.asarray(obstacles, float)
            MAN.validate(mn, ob if tuple(ob.shape) == (self.B, self.nO, 7) else None)
            if MAN.is_off(mn):
                manoeuvres = None
        if tracker is not None:
            from . import tracker as TRK
            if obstacles is None:
                raise ValueError("tracker needs obstacles= rows: pass "
                                 "obstacles.nominal(scenario, B) for the scenario's own")
            tk = tracker.detach().cpu().numpy() if isinstance(tracker, torch.Tensor) \
                else np.asarray(tracker, float)
            if tuple(tk.shape) != (self.B, self.nO, TRK.NP):
                raise ValueError(f"tracker must be [B, nObst, 9] = [{self.B}, {self.nO}, 9]")
            TRK.validate(tk)
        if estimator is not None:
            from . import estimator as EST
            e = estimator.detach().cpu().numpy() if isinstance(estimator, torch.Tensor) \
                else np.asarray(estimator, float)
            if tuple(e.shape) != (self.B, self.nV, EST.NP):
                raise ValueError(f"estimator must be [B, nVeh, 8] = [{self.B}, {self.nV}, 8]")
            EST.validate(e)
        if sensing is not None or obstacle_sensing is not None:
            from . import sensing as SE
            if sense_seed is not None and not 0 <= int(sense_seed) < 2 ** 64:
                raise ValueError("sense_seed must be in [0, 2**64)")
            if not 0 <= int(b_offset) < 2 ** 32:
                raise ValueError("b_offset must be in [0, 2**32)")
        if sensing is not None:
            s = sensing.detach().cpu().numpy() if isinstance(sensing, torch.Tensor) \
                else np.asarray(sensing, float)
            if tuple(s.shape) != (self.B, self.nV, SE.NP):
                raise ValueError(f"sensing must be [B, nVeh, 8] = [{self.B}, {self.nV}, 8]")
            # the measured tick k_meas - lag must lie in the previous step's path
            SE.validate(s, max_lag=self.tps - self.tdx)
            if sense_seed is None and not SE.is_nominal(s):
                raise ValueError("sensing rows that draw need reset(..., sense_seed=...)")
        if obstacle_sensing is not None:
            if obstacles is None:
                raise ValueError("obstacle_sensing needs obstacles= rows: pass "
                                 "obstacles.nominal(scenario, B) for the scenario's own")
            os_ = obstacle_sensing.detach().cpu().numpy() \
                if isinstance(obstacle_sensing, torch.Tensor) else np.asarray(obstacle_sensing, float)
            if tuple(os_.shape) != (self.B, self.nO, SE.ONP):
                raise ValueError(f"obstacle_sensing must be [B, nObst, 3] = [{self.B}, {self.nO}, 3]")
            SE.validate_obstacle_sensing(os_)
            if sense_seed is None and os_.any():
                raise ValueError("obstacle_sensing rows that draw need reset(..., sense_seed=...)")
        if obstacles is not None:
            from . import obstacles as OB
            if not self.nO:
                raise ValueError("obstacles given, but the scenario has no obstacles")
            o = obstacles.detach().cpu().numpy() if isinstance(obstacles, torch.Tensor) \
                else np.asarray(obstacles, float)
            if tuple(o.shape) != (self.B, self.nO, OB.NP):
                raise ValueError(f"obstacles must be [B, nObst, 7] = [{self.B}, {self.nO}, 7]")
            OB.validate(o)
        if truth is not None:
            from . import truth as TR
            t = truth.detach().cpu().numpy() if isinstance(truth, torch.Tensor) \
                else np.asarray(truth, float)
            if tuple(t.shape) != (self.B, self.nV, TR.NP):
                raise ValueError("truth must be [B, nVeh, 5]")
            TR.validate(t, self.h_max)
        if seed is None and getattr(getattr(self.sc, "model", None), "is_noise", False):
            raise ValueError("scenario.model.is_noise is set: pass reset(..., seed=...) to run "
                             "the rollout with model noise (it never runs noise-free silently)")
        if seed is not None and noise is not None:
            raise ValueError("pass either noise (constant terms) or seed, not both")
        self.rng = None if seed is None else PL.NoiseStream(seed, sigma, 0, b_offset)
        x = torch.as_tensor(np.asarray(x_init, float) if not isinstance(x_init, torch.Tensor)
                            else x_init, dtype=torch.float64, device=self.device)
        if tuple(x.shape) != (self.B, self.nV, 6):
            raise ValueError("x_init must be [B, nVeh, 6]")
        self.state.copy_(x)
        self.x_init = x.clone()
        self.control.fill_(float("nan"))
        u0 = torch.tensor([float(u) for u in self.sc.u0], dtype=torch.float64, device=self.device)
        self.control[:, :, 0:self.tdu + self.tps + 1] = u0[None, :, None]
        self.noise = None if noise is None else torch.as_tensor(noise, dtype=torch.float64,
                                                                device=self.device)
        self.truth = None if truth is None else torch.as_tensor(
            truth, dtype=torch.float64, device=self.device).contiguous()
        self.obst_rows = None if obstacles is None else torch.as_tensor(
            obstacles, dtype=torch.float64, device=self.device).contiguous().clone()
        self.sense_rows = None if sensing is None else torch.as_tensor(
            sensing, dtype=torch.float64, device=self.device).contiguous().clone()
        self.osense_rows = None if obstacle_sensing is None else torch.as_tensor(
            obstacle_sensing, dtype=torch.float64, device=self.device).contiguous().clone()
        # without a seed every row is nominal or zero and draws nothing
        self.sense_seed = 0 if sense_seed is None else int(sense_seed)
        self.sense_offset = int(b_offset)
        # the last delivered measurement: NaN, so the first one is always delivered
        self.x_held = None if sensing is None else torch.full(
            (self.B, self.nV, 6), float("nan"), dtype=torch.float64, device=self.device)
        self.est_rows = None if estimator is None else torch.as_tensor(
            estimator, dtype=torch.float64, device=self.device).contiguous().clone()
        self.est_x = self.est_cov = None
        if estimator is not None:
            # no lane is initialised; the span of step 0 is empty
            self.est_x, self.est_cov = EST.alloc(self.B, self.nV, self.device)
        self.est_tick = None           # the global tick of the previous step's measurement
        self.trk_rows = None if tracker is None else torch.as_tensor(
            tracker, dtype=torch.float64, device=self.device).contiguous().clone()
        self.trk_x = self.trk_cov = None
        if tracker is not None:
            self.trk_x, self.trk_cov = TRK.alloc(self.B, self.nO, self.device)
        self.trka_rows = None if tracker_accel is None else torch.as_tensor(
            tracker_accel, dtype=torch.float64, device=self.device).contiguous().clone()
        if tracker_accel is not None:
            # one filter or the other: the state, the tick and the record are shared
            self.trk_x, self.trk_cov = TRKA.alloc(self.B, self.nO, self.device)
        self.imm_rows = self.imm_state = None
        if imm is not None:
            self.imm_rows = tuple(torch.as_tensor(a, dtype=torch.float64, device=self.device)
                                  .contiguous().clone() for a in (imm_trk, imm_sw))
            self.imm_state = IMM.alloc(self.B, self.nO, self.imm_rows[0].shape[2], self.device)
        # (kappa, m_max) of reset(..., margin=); without a filter there is nothing to take it from
        self.margin = margin if (tracker_accel is not None or imm is not None) else None
        self.obst_margin = None        # this step's margins [B, nObst, Hp]
        self.trk_tick = None           # the global tick of the previous obstacle measurement
        self.trk_rec = None            # this step's (estimate, nis, measurement)
        self.man_rows = None if manoeuvres is None else torch.as_tensor(
            manoeuvres, dtype=torch.float64, device=self.device).contiguous().clone()
        self.obst_state = None         # this step's snapshot rows
        self.gov_rows = self.gov_dreq = None
        if governor is not None:
            self.gov_rows = torch.as_tensor(governor, dtype=torch.float64,
                                            device=self.device).contiguous().clone()
            # the required centre distances of every realisation's variant
            self.gov_dreq = GOV.required(self.sc, self.variants, self.variant_of, self.device)
        self.yld_rows = None
        if right_of_way is not None:
            self.yld_rows = torch.as_tensor(right_of_way, dtype=torch.float64,
                                            device=self.device).contiguous().clone()
            self.gov_dreq = YLD.required(self.sc, self.variants, self.variant_of, self.device)
        self.drive_rows = self.a_cmd = self.drive_truth = None
        self.state_c = self.last_path_c = None     # the controller's side of state / last_path
        if drive is not None:
            self.drive_rows = torch.as_tensor(drive, dtype=torch.float64,
                                              device=self.device).contiguous().clone()
            self.a_cmd = x[:, :, 4].clone()
            self.state_c = x.clone()
            if self.truth is None:
                from . import truth as TR
                self.drive_truth = TR.nominal(self.params, self.B, self.device)
            else:
                self.drive_truth = self.truth
        self.last_path = None
        self.u_prev = None
        self.history = []
        self.i = 0
        if self.path_metrics is not None:
            self.path_metrics.reset(self.B)

    def _obstacle_prediction(self, tick_meas):
        """Iter.obstacleFutureTrajectories (MPC_Iter.py:45-51) from the constant-velocity
        obstacle state at the measurement tick (main.py:61-71, 123); the same for every
        realisation of a variant.  Returns a device tensor [B, nObst, 2, Hp] or None."""
        if not self.nO:
            return None
        if self.obst_rows is not None:
            # the obstacle truth: the true pose at the measurement tick, extrapolated
            # straight, per (realisation, obstacle) on the device
            from . import obstacles as OB
            sc = self.sc
            rows, t_meas = self.obst_rows, tick_meas * sc.tick_length
            if self.man_rows is not None:
                # the obstacle manoeuvres: the true pose and current speed at the measurement
                # tick as a row; measured at its own t = 0 it is that pose exactly
                from . import manoeuvres as MAN
                rows, t_meas = MAN.state(self.obst_rows, self.man_rows, t_meas), 0.0
                self.obst_state = rows
            if self.imm_rows is not None:
                # the bank of include/scpqp_imm.h: the same measurement and time since the
                # previous one, every mode filtered, the weighted prediction
                from . import imm as IMM
                g0 = tick_meas if self.trk_tick is None else self.trk_tick
                x_imm, cov, mu = self.imm_state
                obst, x_hat, z, nis = IMM.step(rows, self.osense_rows, self.sense_seed, self.i,
                                               self.sense_offset, *self.imm_rows, t_meas,
                                               (tick_meas - g0) * sc.tick_length,
                                               sc.delay_x + sc.dt + sc.delay_u, sc.dt, self.Hp,
                                               x_imm, cov, mu)
                self.trk_tick = tick_meas
                self.trk_rec = (x_hat, nis, z, mu.clone())
                if self.margin is not None:
                    from . import margin as MG
                    self.obst_margin = MG.step(self.imm_rows[0], x_imm, cov, mu,
                                               sc.delay_x + sc.dt + sc.delay_u, sc.dt, self.Hp,
                                               *self.margin)
                return obst
            if self.trk_rows is not None or self.trka_rows is not None:
                # the obstacle tracker (include/scpqp_tracker.h): the same measurement,
                # filtered over the time since the previous one, predicted on its arc; or the
                # one with an acceleration state (include/scpqp_tracker_accel.h), predicted
                # on its pieces
                if self.trka_rows is not None:
                    from . import tracker_accel as TRK
                else:
                    from . import tracker as TRK
                g0 = tick_meas if self.trk_tick is None else self.trk_tick
                obst, z, nis = TRK.step(rows, self.osense_rows, self.sense_seed, self.i,
                                        self.sense_offset,
                                        self.trk_rows if self.trka_rows is None else self.trka_rows,
                                        t_meas,
                                        (tick_meas - g0) * sc.tick_length,
                                        sc.delay_x + sc.dt + sc.delay_u, sc.dt, self.Hp,
                                        self.trk_x, self.trk_cov)
                self.trk_tick = tick_meas
                self.trk_rec = (self.trk_x.clone(), nis, z)
                if self.margin is not None:
                    from . import margin as MG
                    self.obst_margin = MG.step(self.trka_rows, self.trk_x, self.trk_cov, None,
                                               sc.delay_x + sc.dt + sc.delay_u, sc.dt, self.Hp,
                                               *self.margin)
                return obst
            if self.osense_rows is not None:
                # the sensing truth: the same extrapolation from a noisy pose and speed
                from . import sensing as SE
                return SE.predict_sensed(rows, self.osense_rows, self.sense_seed, self.i,
                                         self.sense_offset, t_meas,
                                         sc.delay_x + sc.dt + sc.delay_u, sc.dt, self.Hp)
            return OB.predict(rows, t_meas, sc.delay_x + sc.dt + sc.delay_u, sc.dt, self.Hp)
        if self.var_obstacles is not None:
            # one prediction per variant on the host, gathered per realisation on the device
            fut = np.stack([self._predict(ob, tick_meas) for ob in self.var_obstacles])
            t = torch.as_tensor(fut, dtype=torch.float64, device=self.device)
            return t[self.variant_of.long()].contiguous()
        t = torch.as_tensor(self._predict(self.obstacles, tick_meas), dtype=torch.float64,
                            device=self.device)
        return t[None].expand(self.B, -1, -1, -1).contiguous()

    def _predict(self, ob, tick_meas):
        sc = self.sc
        t_meas = tick_meas * sc.tick_length
        x = t_meas * ob[:, 3] * np.cos(ob[:, 2]) + ob[:, 0]
        y = t_meas * ob[:, 3] * np.sin(ob[:, 2]) + ob[:, 1]
        lead = sc.delay_x + sc.dt + sc.delay_u
        step = ((np.arange(self.Hp) + 1) * sc.dt + lead)[None, :] * ob[:, 3:4]   # [nO, Hp]
        fut = np.zeros((self.nO, 2, self.Hp))
        fut[:, 0] = step * np.cos(ob[:, 2:3]) + x[:, None]
        fut[:, 1] = step * np.sin(ob[:, 2:3]) + y[:, None]
        return fut

    def _held_command(self, tick_now):
        return held_command_tick(tick_now, self.tdx, self.tdu, self.tps, self.ticks_total)

    def step(self):
        i, sc, B, nV, Hp, tps = self.i, self.sc, self.B, self.nV, self.Hp, self.tps
        f = dict(dtype=torch.float64, device=self.device)
        if self.timing:
            torch.cuda.synchronize(self.device)
        t_step = time.perf_counter()
        tick_now = i * tps
        # what the controller's side reads: the realised state and path, with a drive their
        # copies whose column 4 holds the command in force instead of the realised acceleration
        state_c = self.state if self.drive_rows is None else self.state_c
        path_c = self.last_path if self.drive_rows is None else self.last_path_c
        # measured state: tick_now - ticks_delay_x (inside the previous step's path)
        if self.tdx == 0 or path_c is None:
            x_meas = state_c
        else:
            x_meas = path_c[:, :, tps - min(self.tdx, tick_now), :].contiguous()
        delivered = None
        if self.sense_rows is not None:
            # the sensing truth: what the controller gets of that tick (include/scpqp_sensing.h)
            from . import sensing as SE
            delivered = torch.empty((B, nV), dtype=torch.int32, device=self.device)
            if path_c is None:
                x_meas = SE.measure(state_c.contiguous(), 0, self.sense_rows, self.sense_seed, i,
                                    self.sense_offset, self.x_held, delivered)
            else:
                x_meas = SE.measure(path_c, tps - min(self.tdx, tick_now), self.sense_rows,
                                    self.sense_seed, i, self.sense_offset, self.x_held, delivered)
        x_in, nis = x_meas, None
        if self.est_rows is not None:
            # the state estimator (include/scpqp_estimator.h): predict over the ticks
            # (g0, g1] since the previous measurement, tick j with the control tick the
            # plant's output j read (below), then correct with this step's measurement
            from . import estimator as EST
            g1 = max(0, tick_now - self.tdx)
            g0 = g1 if self.est_tick is None else self.est_tick
            u_span = None
            if g1 > g0:
                span = [min(self.ticks_total, j + 1) for j in range(g0 + 1, g1 + 1)]
                u_span = self.control[:, :, torch.as_tensor(span, device=self.device)].contiguous()
            x_meas = x_meas.contiguous()
            nis = EST.step(self.params, u_span, sc.tick_length, x_meas, delivered, self.est_rows,
                           self.est_x, self.est_cov, h_max=self.h_max)
            self.est_tick = g1
            x_in = self.est_x.clone()
        speed = self.state[:, :, 3]
        umax = torch.minimum(torch.full_like(speed, float(sc.mechanicalSteeringLimit)),
                             torch.atan(LATERAL_ACC_LIMIT * self.L[None, :] / speed ** 2))
        src = self._held_command(tick_now)
        u_hold = torch.zeros((B, nV), **f) if src is None else self.control[:, :, src].contiguous()
        # IterClass delay compensation (MPC_Iter.py:24-33)
        horizon = sc.delay_x + sc.dt + sc.delay_u
        # with a seed: this step's noise stream (epoch i), else None and nothing changes
        rng = None if self.rng is None else self.rng.at(i)
        x_plan = x_in
        if self.gov_rows is not None or self.yld_rows is not None:
            # the acceleration in force at tick_now is the governor's own command: with a
            # measurement delay the compensation assumes it over the whole span
            x_plan = x_in.clone()
            x_plan[:, :, 4] = self.state[:, :, 4] if self.drive_rows is None else self.a_cmd
        x0, dtraj = PL.delay_compensate(self.params, x_plan.contiguous(), u_hold, horizon,
                                        noise=self.noise, h_max=self.h_max, device=self.device,
                                        rng=rng)
        # SCP solve, warm-started from the previous controller output (SCP_controller.py:42-43)
        obst = self._obstacle_prediction(max(0, tick_now - self.tdx))
        u_warm = self.u_prev
        # the draws of comp_jacobian's one ode call (Model.py:58)
        ec_noise = None if rng is None else PL.draw_ec_noise(rng, B, nV, self.device)
        out = self.solver.solve(x0, u_hold, ec_noise, u_warm=u_warm, obst=obst, out=self.out,
                                variant=self.variant_of, obst_margin=self.obst_margin)
        self.u_prev = out.u.clone()
        gov = None
        if self.gov_rows is not None:
            # the speed governor (include/scpqp_governor.h) on this step's plan
            from . import governor as GOV
            gov = GOV.step(self.gov_rows, x0, out.traj, None if obst is None else obst.contiguous(),
                           self.obst_margin, *self.gov_dreq, sc.dt, sc.delay_u, hp_max=Hp)
        elif self.yld_rows is not None:
            # the same with right of way and graded braking (include/scpqp_yield.h)
            from . import yielding as YLD
            gov = YLD.step(self.yld_rows, x0, out.traj, None if obst is None else obst.contiguous(),
                           self.obst_margin, *self.gov_dreq, sc.dt, sc.delay_u, hp_max=Hp)
        if self.timing:
            torch.cuda.synchronize(self.device)
        t_ctrl = time.perf_counter() - t_step
        U = out.u.clone()
        PL.clip_controls(U, u_hold, umax, nV, Hp, self.du_lim)
        # actuator-delayed control path (main.py:176-182)
        sl = np.arange(i * tps + 1 + self.tdu + tps, (i + 1) * tps + 1 + self.tdu + tps)
        sl[sl >= self.ticks_total] = self.ticks_total
        sl_t = torch.as_tensor(np.unique(sl), device=self.device)
        first = U.view(B, nV, -1)[:, :, 0]
        self.control[:, :, sl_t] = first[:, :, None].expand(B, nV, len(sl_t))
        # plant over [i dt, (i+1) dt]: output k reads control tick ceil(t_k / tick) + 1
        timelist = np.linspace(i * sc.dt, (i + 1) * sc.dt, tps + 1)
        idx = [min(self.ticks_total, math.ceil(t / sc.tick_length) + 1) for t in timelist]
        u_tick = self.control[:, :, torch.as_tensor(idx, device=self.device)].contiguous()
        x_start = self.state
        if self.drive_rows is not None:
            # the drive truth (include/scpqp_drive.h): the command in force over this step
            path = PL.plant_step(self.params, x_start, u_tick, sc.tick_length, noise=self.noise,
                                 h_max=self.h_max, device=self.device, rng=rng,
                                 truth=self.drive_truth, drive=self.drive_rows, a_cmd=self.a_cmd)
        else:
            path = PL.plant_step(self.params, x_start, u_tick, sc.tick_length, noise=self.noise,
                                 h_max=self.h_max, device=self.device, rng=rng, truth=self.truth)
        if self.path_metrics is not None:
            # every global tick once: entry 0 of a later step is the previous step's last
            self.path_metrics.accumulate(path, tick0=i * tps, k_first=0 if i == 0 else 1,
                                         variant=self.variant_of, obstacles=self.obst_rows,
                                         manoeuvres=self.man_rows, check_off=False)
        self.last_path = path
        self.state = path[:, :, tps, :].contiguous()
        if self.drive_rows is not None:
            # the controller's copy of the path carries the command that was in force over it,
            # its copy of the state the command that takes effect at the start of step i + 1
            self.last_path_c = path.clone()
            self.last_path_c[:, :, :, 4] = self.a_cmd[:, :, None]
            if gov is not None:
                self.a_cmd = gov[0].clone()
            self.state_c = self.state.clone()
            self.state_c[:, :, 4] = self.a_cmd
        elif gov is not None:
            # the command takes effect at the start of step i + 1
            self.state[:, :, 4] = gov[0]
        rec = dict(x0=x0, u0=u_hold, umax=umax, U=U, traj=out.traj.clone(),
                   n_scp=out.n_scp.clone(), status=out.status.clone())
        if rng is not None:
            rec["ec_noise"] = ec_noise
            rec["epoch"] = i
        if self.obst_rows is not None:
            rec["obst"] = obst      # what the controller was told of the obstacle truth
        if self.man_rows is not None:
            rec["obst_state"] = self.obst_state   # the manoeuvring obstacles at the measurement tick
        if self.trk_rows is not None or self.trka_rows is not None:
            # the tracker's estimate, its innovations and the obstacle measurement it took
            rec["obst_est"], rec["obst_nis"], rec["obst_meas"] = self.trk_rec
        if self.imm_rows is not None:
            # the bank's combined estimate, every mode's innovation and probability
            rec["obst_est"], rec["obst_nis"], rec["obst_meas"], rec["obst_mu"] = self.trk_rec
        if self.obst_margin is not None:
            rec["obst_margin"] = self.obst_margin   # what the solve added to its safety distances
        if gov is not None:
            rec["accel_cmd"], rec["gov_k_conf"], rec["gov_clear"] = gov[:3]
            if len(gov) > 3:
                rec["gov_k_any"], rec["gov_who"], rec["gov_d_stop"] = gov[3:]
        if self.drive_rows is not None:
            rec["accel_real"] = self.state[:, :, 4].clone()   # realised, at the step's end
        if self.sense_rows is not None:
            rec["x_meas"] = x_meas  # what the controller was told of the vehicles
            rec["delivered"] = delivered
        if self.est_rows is not None:
            rec["x_est"] = x_in     # what the controller planned from: a clone of the estimate
            rec["nis"] = nis
            if self.sense_rows is None:
                rec["x_meas"] = x_meas.clone()
        if self.evaluate:
            # main.py:201-202: evaluateInOriginalProblem on the clipped U and the prediction
            ref = self.solver.sample_reference(x0, variant=self.variant_of)
            rec["ref"] = ref
            rec["evaluation"] = evaluate_in_original_problem(
                sc, U.view(B, nV, Hp).transpose(1, 2), rec["traj"], ref, obst,
                variants=self.variants, variant_of=self.variant_of,
                obst_margin=self.obst_margin)
        if self.keep_path:
            rec["path"] = path
            rec["delay_traj"] = dtraj
            rec["u_tick"] = u_tick
            rec["x_start"] = path[:, :, 0, :]
        if self.trace:
            rec["u_warm"] = u_warm
            rec["obst"] = obst
            # kept on the host (a diagnostic mode: c2 at B = 1024 would hold ~106 MB per
            # step on the device), up to the largest SCP count of the step; iterations
            # past a problem's own n_scp stay NaN as on the device
            ns = int(out.n_scp.max().item())
            tr = torch.full((B,) + tuple(out.trace.shape[1:]), float("nan"), dtype=out.trace.dtype)
            tr[:, :ns] = out.trace[:, :ns].cpu()
            rec["trace"] = tr
            rec["u"] = out.u.clone()
        if self.timing:
            torch.cuda.synchronize(self.device)
        rec["controllerRuntime"] = t_ctrl               # batch latency: every realisation
        rec["stepTime"] = time.perf_counter() - t_step   # of the batch shares it
        self.history.append(rec)
        self.i += 1
        return rec

    def run(self, n_steps):
        for _ in range(n_steps):
            self.step()
        return self.history

    def result_for_plot(self, b):
        """``result_for_plot1`` of main.py:213-225 for realisation b, the dict
        draw_video.py:44-56 reads back, as numpy arrays over the steps run so far
        (needs keep_path=True and evaluate=True).  Unset path ticks stay NaN and
        unrun steps zero, as main.py initialises them (main.py:56-62).  Timing fields
        are the batch's per-step wall times (meaningful with timing=True)."""
        if not self.keep_path or not self.evaluate:
            raise ValueError("result_for_plot needs keep_path=True and evaluate=True")
        sc, nV, Hp, tps = self.sc, self.nV, self.Hp, self.tps
        Nsim, T = int(sc.Nsim), self.ticks_total
        veh = np.full((6, nV, T + 1), np.nan)
        veh[:, :, 0] = self.x_init[b].cpu().numpy().T
        obs = np.zeros((self.nO, 2, T + 1))
        if self.obst_rows is not None:
            # the realisation's own obstacle motion (include/scpqp_obstacles.h)
            from . import obstacles as OB
            if self.man_rows is not None:
                # and its manoeuvres (include/scpqp_manoeuvres.h)
                from . import manoeuvres as MAN
                p = MAN.pose(self.obst_rows[b:b + 1], self.man_rows[b:b + 1], sc.tick_length, 0,
                             T)[0].cpu().numpy()
            else:
                p = OB.pose(self.obst_rows[b:b + 1], sc.tick_length, 0, T)[0].cpu().numpy()
            obs[:, 0], obs[:, 1] = p[:, :, 0], p[:, :, 1]
        elif self.nO:
            t = np.arange(T + 1) * sc.tick_length                       # main.py:61-71
            ob = self.obstacles
            obs[:, 0] = t[None] * (ob[:, 3] * np.cos(ob[:, 2]))[:, None] + ob[:, 0:1]
            obs[:, 1] = t[None] * (ob[:, 3] * np.sin(ob[:, 2]))[:, None] + ob[:, 1:2]
        out = dict(
            vehiclePathFullRes=veh, obstaclePathFullRes=obs,
            controlPathFullRes=self.control[b].cpu().numpy(),
            controlPredictions=np.zeros((Hp, nV, Nsim)),
            trajectoryPredictions=np.zeros((Hp, 2, nV, Nsim)),
            initial_pos=np.zeros((2, nV, Nsim)),
            ReferenceTrajectory=np.zeros((Hp, 2, nV, Nsim)),
            MPC_delay_compensation_trajectory=np.zeros((PL.DELAY_STEPS, 6, nV, Nsim)),
            evaluations_obj_value=[float(r["evaluation"]["predictionObjectiveValue"][b])
                                   for r in self.history],
            controllerRuntime=np.zeros((Nsim, 1)), stepTime=np.zeros((Nsim, 1)))
        for i, r in enumerate(self.history[:Nsim]):
            lo = tps * i + 1
            hi = min(T + 1, tps * (i + 1) + 1)
            veh[:, :, lo:hi] = r["path"][b, :, 1:1 + hi - lo].cpu().numpy().transpose(2, 0, 1)
            out["controlPredictions"][:, :, i] = r["U"][b].view(nV, Hp).T.cpu().numpy()
            out["trajectoryPredictions"][:, :, :, i] = r["traj"][b].cpu().numpy()
            out["initial_pos"][:, :, i] = r["x0"][b, :, 0:2].T.cpu().numpy()
            out["ReferenceTrajectory"][:, :, :, i] = r["ref"][b].cpu().numpy()
            out["MPC_delay_compensation_trajectory"][:, :, :, i] = r["delay_traj"][b].cpu().numpy()
            out["controllerRuntime"][i, 0] = r["controllerRuntime"]
            out["stepTime"][i, 0] = r["stepTime"]
        return out

    def dump_result(self, fp, b):
        """json.dump of result_for_plot(b) with main.py:226-231's encoding (nested
        lists, NaN written as NaN)."""
        res = self.result_for_plot(b)
        json.dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}, fp)

    def metrics(self):
        """The realised-path metrics of the steps run since reset(): a dict of device
        tensors per realisation (``PathMetrics.result``; needs ``metrics=True``)."""
        if self.path_metrics is None:
            raise ValueError("metrics() needs ClosedLoopBatch(..., metrics=True)")
        return self.path_metrics.result()

    def metrics_summary(self):
        """``metrics.summarize`` of this batch: collision rate, clearance quantiles and
        cross-track figures as plain Python numbers."""
        from .metrics import summarize
        return summarize(self.metrics())

    def close(self):
        if self.path_metrics is not None:
            self.path_metrics.close()
        self.solver.close()
