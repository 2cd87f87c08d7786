"""Interacting-multiple-model obstacle tracker: a bank of up to four six-state filters per
(realisation, obstacle) between the obstacle sensing and the obstacle prediction
(include/scpqp_imm.h; csrc/imm.hip).

Every mode of a bank is the filter of scpqp/tracker_accel.py with its own row of 14 fields; a
Markov chain says how often the obstacle changes its mind, the measurement's likelihood under
each mode moves the probabilities, and the planner is told the probability-weighted prediction
(``ClosedLoopBatch.reset(..., imm=(trk, sw))``).  A bank is two float64 tensors:

``trk`` ``[B, nObst, M, 14]``   the tuning of every mode (the fields of scpqp/tracker_accel.py)
``sw``  ``[B, nObst, M + 1, M]`` row 0 the initial probabilities, rows 1..M the transition
                                 matrix ``Pi[i][j]`` = P(mode j at this call | mode i before)

The two single filters (scpqp/tracker.py, scpqp/tracker_accel.py) are unchanged; a lane runs one
of the three.

The defaults of ``bank`` are choices, not tunings: three modes that differ in what the
prediction keeps (nothing, the turn rate, the turn rate and the acceleration) and in what the
filter believes in: a quantity a mode does not believe in (the turn rate and the acceleration
of "straight", the acceleration of "arc") gets a tenth (``QUIET``) of the single filter's
initial sigma and process-noise density, so that the measurements can tell the modes apart (a
hold alone changes the prediction, not the likelihood); the brake mode's ``q_accel`` is three
times the single filter's so that it picks up the onset of a braking within a call or two; a
chance of 0.9 per call to stay in a mode with the rest spread evenly; a uniform start.  None of
them was fitted to a rollout.

``off``       the bank without a filter: the untracked prediction, bitwise
``is_off``    True when every row is the off row
``bank``      a bank for an obstacle sensing, from ``tracker_accel.matched`` rows
``validate``  host-side check of a bank before a rollout
``alloc``     the state a bank carries between steps
``step``      one step of every lane's bank (scpqp_obstacles_track_imm)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as LB
from . import tracker_accel as TRKA

NP = LB.TRKA_NP
NS = LB.TRKA_NS
NZ = LB.TRKA_NZ
MAX_MODES = LB.IMM_MAX_MODES
SUM_TOL = LB.IMM_SUM_TOL
MODES = ("straight", "arc", "brake")
STAY = 0.9
# a quantity a mode does not believe in: this share of tracker_accel's p0 and q of it
QUIET = 0.1
# the brake mode: this multiple of tracker_accel.Q_DEFAULT's q_accel
BRAKE_Q_ACCEL = 3.0

_need_obstacles = TRKA._need_obstacles
_host = TRKA._host
_gpu = TRKA._gpu


def _need_modes(M):
    if not 1 <= M <= MAX_MODES:
        raise ValueError(f"a bank holds 1..{MAX_MODES} modes, got {M}")


def off(B, n_obst, n_modes=len(MODES), device=None):
    """(trk [B, nObst, M, 14], sw [B, nObst, M + 1, M]) of zeros: no filter, the untracked
    prediction (the sw of an off lane is not read)."""
    _need_obstacles(int(n_obst))
    _need_modes(int(n_modes))
    f = dict(dtype=torch.float64, device=torch.device(device or "cuda"))
    return (torch.zeros((int(B), int(n_obst), int(n_modes), NP), **f),
            torch.zeros((int(B), int(n_obst), int(n_modes) + 1, int(n_modes)), **f))


def is_off(trk):
    """True when every row of every lane is exactly the off row (host side)."""
    return bool((_host(trk) == 0.0).all())


def mode_rows(osense_rows, mode, **kw):
    """``tracker_accel.matched`` rows [B, nObst, 14] of one named mode: "straight" (both holds
    0; turn rate and acceleration quiet: ``p0`` and ``q`` of both times QUIET), "arc" (the turn
    rate held, the acceleration neither held nor believed in) or "brake" (both held, ``q_accel``
    times BRAKE_Q_ACCEL).  ``kw`` goes to ``matched`` and overrides."""
    q = list(TRKA.Q_DEFAULT)
    if mode == "straight":
        q[3], q[4] = QUIET * q[3], QUIET * q[4]
        kw = dict(dict(w_hold=0.0, a_hold=0.0, p0_yaw=QUIET * TRKA.P0_YAW,
                       p0_accel=QUIET * TRKA.P0_ACCEL), **kw)
    elif mode == "arc":
        q[4] = QUIET * q[4]
        kw = dict(dict(a_hold=0.0, p0_accel=QUIET * TRKA.P0_ACCEL), **kw)
    elif mode == "brake":
        q[4] = BRAKE_Q_ACCEL * q[4]
    else:
        raise ValueError(f"unknown mode {mode!r}: one of {MODES}")
    return TRKA.matched(osense_rows, q=kw.pop("q", q), **kw)


def bank(osense_rows, modes=MODES, stay=STAY, device=None, **kw):
    """A bank for an obstacle sensing ``[B, nObst, 3]`` (scpqp/sensing.py): ``trk`` holds
    ``mode_rows`` of every name in ``modes``, ``Pi`` has ``stay`` on the diagonal and the rest
    spread evenly over the other modes (one mode: 1), ``mu0`` is uniform.  Returns
    ``(trk [B, nObst, M, 14], sw [B, nObst, M + 1, M])`` where the sensing rows live."""
    modes = tuple(modes)
    M = len(modes)
    _need_modes(M)
    stay = float(stay)
    if not 0.0 <= stay <= 1.0:
        raise ValueError("stay must lie in [0, 1]")
    if isinstance(osense_rows, torch.Tensor):
        device = osense_rows.device
    dev = torch.device(device or "cuda")
    trk = torch.stack([mode_rows(osense_rows, m, device="cpu", **kw).cpu() for m in modes], dim=2)
    B, nO = trk.shape[:2]
    one = np.empty((M + 1, M))
    one[0] = 1.0 / M
    if M == 1:
        one[1] = 1.0
    else:
        one[1:] = (1.0 - stay) / (M - 1)
        one[1:][np.eye(M, dtype=bool)] = stay
    sw = np.broadcast_to(one, (B, nO, M + 1, M)).copy()
    validate(trk, sw)
    return (trk.to(dev).contiguous(),
            torch.as_tensor(sw, dtype=torch.float64, device=dev))


def validate(trk, sw):
    """ValueError on a bank the device would treat as bad (include/scpqp_imm.h): a bad row of
    any mode, off and non-off rows mixed in a lane, an ``sw`` entry that is not finite or
    negative, ``mu0`` or a row of ``Pi`` that does not sum to 1 within 1e-12.  The ``sw`` of an
    off lane is not read.  The message names the lane.  Host side."""
    t, s = _host(trk), _host(sw)
    if t.ndim != 4 or t.shape[3] != NP or not 1 <= t.shape[2] <= MAX_MODES:
        raise ValueError(f"trk must be [B, nObst, M, 14] with 1 <= M <= {MAX_MODES}")
    B, nO, M = t.shape[:3]
    if tuple(s.shape) != (B, nO, M + 1, M):
        raise ValueError(f"sw must be [B, nObst, M + 1, M] = [{B}, {nO}, {M + 1}, {M}]")
    for j in range(M):
        try:
            TRKA.validate(t[:, :, j])
        except ValueError as e:
            raise ValueError(f"mode {j}: {e}") from None
    on = (t != 0.0).any(axis=3)
    mixed = np.argwhere(on.any(axis=2) & ~on.all(axis=2))
    if len(mixed):
        b, o = mixed[0]
        raise ValueError(f"trk[{b}, {o}]: off and non-off rows in one lane")
    lane_on = on.all(axis=2)
    bad = np.argwhere((~np.isfinite(s) | (s < 0.0)) & lane_on[:, :, None, None])
    if len(bad):
        b, o, i, j = bad[0]
        raise ValueError(f"sw[{b}, {o}, {i}, {j}] must be finite and >= 0")
    sums = np.zeros((B, nO, M + 1))
    for j in range(M):
        sums = sums + np.where(lane_on[:, :, None], s[..., j], 1.0 / M)
    bad = np.argwhere(~(np.abs(sums - 1.0) <= SUM_TOL))
    if len(bad):
        b, o, i = bad[0]
        what = "mu0" if i == 0 else f"row {i - 1} of Pi"
        raise ValueError(f"sw[{b}, {o}]: {what} does not sum to 1")


def alloc(B, n_obst, n_modes, device=None):
    """(x_imm [B, nObst, M, 6] filled with NaN: no lane is initialised, cov [B, nObst, M, 6, 6]
    of zeros, mu [B, nObst, M] of zeros): what ``step`` carries from one MPC step to the next."""
    _need_obstacles(int(n_obst))
    _need_modes(int(n_modes))
    B, nO, M = int(B), int(n_obst), int(n_modes)
    f = dict(dtype=torch.float64, device=torch.device(device or "cuda"))
    return (torch.full((B, nO, M, NS), float("nan"), **f), torch.zeros((B, nO, M, NS, NS), **f),
            torch.zeros((B, nO, M), **f))


def step(rows, osense, seed, epoch, b_offset, trk, sw, t_meas, t_since, lead, dt, hp, x_imm, cov,
         mu):
    """One step of every lane's bank (scpqp_obstacles_track_imm): measure the obstacle truth
    ``rows`` [B, nObst, 7] at ``t_meas`` through ``osense`` [B, nObst, 3] (None: the exact
    sensor) as ``tracker_accel.step`` does, mix the modes, predict every mode over ``t_since``
    seconds, initialise on or correct with the measurement, move the probabilities, and predict
    the weighted horizon.  ``trk`` [B, nObst, M, 14], ``sw`` [B, nObst, M + 1, M]; ``x_imm``
    [B, nObst, M, 6], ``cov`` [B, nObst, M, 6, 6] and ``mu`` [B, nObst, M] are updated in place.
    Returns ``(obst [B, nObst, 2, hp], x_hat [B, nObst, 6], z [B, nObst, 4], nis [B, nObst, M])``:
    the controller's prediction, the combined estimate, the measurement, and every mode's
    normalised innovation squared (NaN where the lane did not correct).  Device tensors."""
    from .obstacles import _rows_arg
    from .plant import _ptr, _stream
    from .sensing import _stream_struct
    rows = _rows_arg(rows)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    if not isinstance(trk, torch.Tensor) or trk.dim() != 4:
        raise ValueError("trk must be a [B, nObst, M, 14] tensor")
    M = int(trk.shape[2])
    _need_modes(M)
    trk = _gpu(trk, "trk", (B, nO, M, NP))
    sw = _gpu(sw, "sw", (B, nO, M + 1, M))
    x_imm = _gpu(x_imm, "x_imm", (B, nO, M, NS))
    cov = _gpu(cov, "cov", (B, nO, M, NS, NS))
    mu = _gpu(mu, "mu", (B, nO, M))
    st = None
    if osense is not None:
        osense = _gpu(osense, "osense", (B, nO, LB.OSENSE_NP))
        st = C.byref(_stream_struct(seed, epoch, b_offset))
    t_since = float(t_since)
    if not (t_since >= 0.0 and np.isfinite(t_since)):
        raise ValueError("t_since must be finite and >= 0")
    lib = LB.load()
    f = dict(dtype=torch.float64, device=rows.device)
    obst = torch.empty((B, nO, 2, int(hp)), **f)
    x_hat = torch.empty((B, nO, NS), **f)
    z = torch.empty((B, nO, NZ), **f)
    nis = torch.empty((B, nO, M), **f)
    LB.check(lib.scpqp_obstacles_track_imm(B, nO, int(hp), M, _ptr(rows), _ptr(osense), st,
                                           _ptr(trk), _ptr(sw), float(t_meas), t_since,
                                           float(lead), float(dt), _ptr(x_imm), _ptr(cov),
                                           _ptr(mu), _ptr(x_hat), _ptr(z), _ptr(nis), _ptr(obst),
                                           _stream(rows.device)), lib)
    return obst, x_hat, z, nis
