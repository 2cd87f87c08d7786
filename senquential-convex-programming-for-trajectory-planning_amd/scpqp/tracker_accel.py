"""Obstacle tracker with an acceleration state: a six-state extended Kalman filter per
(realisation, obstacle) between the obstacle sensing and the obstacle prediction
(include/scpqp_tracker_accel.h; csrc/tracker_accel.hip).

A tuning is a float64 tensor ``[B, nObst, 14]`` of rows ``(r_pos, r_heading, r_speed, q_pos,
q_heading, q_speed, q_yaw, q_accel, p0_yaw, p0_accel, w_clamp, a_clamp, w_hold, a_hold)``: the
sigmas the filter assumes of the measured position, heading and speed, its process-noise
densities on position, heading, speed, turn rate and acceleration, the sigmas of the turn rate
and of the acceleration at initialisation, the largest turn rate and acceleration the
prediction may use, and the seconds for which the prediction keeps each
(``ClosedLoopBatch.reset(..., tracker_accel=)``).  The filter runs on the model the manoeuvring
obstacles themselves use (scpqp/manoeuvres.py): one piece of constant acceleration and constant
turn rate with its stop rule.  Its prediction brakes to a stop and never reverses.  A row per
lane: a tuning sweep runs in one batch.  The five-state tracker (scpqp/tracker.py) is unchanged.

The defaults of the fields the five-state tracker does not have are choices, not tunings:
``q_accel`` 1 m/s^2/sqrt(s) lets the estimate follow a braking that sets in within a second,
``p0_accel`` 3 m/s^2 covers comfortable braking, ``a_clamp`` 6 m/s^2 is about what a road
vehicle can do, and both holds are longer than any horizon, so the prediction keeps what the
filter learnt unless a study says otherwise.  None of them was fitted to a rollout.

``off``         the rows without a filter: the untracked prediction, bitwise
``rows``        rows from scalars or arrays per field
``matched``     rows whose R is an obstacle sensing's own sigmas, raised to a floor (R must be > 0)
``from_table``  rows gathered from a table of K candidates, for discrete studies
``validate``    host-side check of the rows before a rollout
``alloc``       the state a filter carries between steps: a NaN estimate and a covariance
``step``        one tracker step of every lane (scpqp_obstacles_track_accel)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as LB

NP = LB.TRKA_NP
NS = LB.TRKA_NS
NZ = LB.TRKA_NZ
FIELDS = LB.TRKA_FIELDS
_R = (LB.TRKA_R_POS, LB.TRKA_R_HEADING, LB.TRKA_R_SPEED)
# R may not be 0: the smallest sigmas `matched` assumes of a sensor that reports none
FLOOR = (1e-3, 1e-3, 1e-3)
# per sqrt(second): position, heading, speed, turn rate as in scpqp/tracker.py, and the
# acceleration (a choice, see above)
Q_DEFAULT = (0.01, 0.005, 0.02, 0.02, 1.0)
P0_YAW = 0.5
P0_ACCEL = 3.0
W_CLAMP = 1.0
A_CLAMP = 6.0
# longer than any horizon: the prediction keeps the turn rate and the acceleration
W_HOLD = 1e3
A_HOLD = 1e3


def _need_obstacles(nO):
    if not 1 <= nO <= LB.MAX_OBST:
        raise ValueError(f"a tracker needs 1..{LB.MAX_OBST} obstacles, got {nO}")


def _host(rows):
    return rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, float)


def off(B, n_obst, device=None):
    """[B, nObst, 14] of zeros: no filter, the untracked prediction."""
    _need_obstacles(int(n_obst))
    return torch.zeros((int(B), int(n_obst), NP), dtype=torch.float64,
                       device=torch.device(device or "cuda"))


def is_off(rows):
    """True when every row is exactly the off row (host side)."""
    return bool((_host(rows) == 0.0).all())


def rows(B, n_obst, r_pos=0.05, r_heading=0.01, r_speed=0.1, q_pos=Q_DEFAULT[0],
         q_heading=Q_DEFAULT[1], q_speed=Q_DEFAULT[2], q_yaw=Q_DEFAULT[3], q_accel=Q_DEFAULT[4],
         p0_yaw=P0_YAW, p0_accel=P0_ACCEL, w_clamp=W_CLAMP, a_clamp=A_CLAMP, w_hold=W_HOLD,
         a_hold=A_HOLD, device=None):
    """[B, nObst, 14] from one value per field: a scalar, or an array that broadcasts to
    [B, nObst] (``[B, 1]``: one tuning per realisation, the shape of a sweep).  Validated."""
    B, n_obst = int(B), int(n_obst)
    _need_obstacles(n_obst)
    out = np.empty((B, n_obst, NP))
    for f, val in enumerate((r_pos, r_heading, r_speed, q_pos, q_heading, q_speed, q_yaw, q_accel,
                             p0_yaw, p0_accel, w_clamp, a_clamp, w_hold, a_hold)):
        try:
            out[..., f] = np.broadcast_to(np.asarray(_host(val), float), (B, n_obst))
        except ValueError:
            raise ValueError(f"{FIELDS[f]} does not broadcast to [B, nObst] = [{B}, {n_obst}]") from None
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def matched(osense_rows, floor=FLOOR, q=Q_DEFAULT, p0_yaw=P0_YAW, p0_accel=P0_ACCEL,
            w_clamp=W_CLAMP, a_clamp=A_CLAMP, w_hold=W_HOLD, a_hold=A_HOLD, device=None):
    """Rows for an obstacle sensing ``[B, nObst, 3]`` (scpqp/sensing.py): R_* is the sensor's
    own sigma of that field, raised to ``floor`` = (pos, heading, speed) since R must be > 0
    (an exact sensor still gives a legal row), Q_* is ``q`` = (pos, heading, speed, yaw,
    accel), and the other fields are the same for every lane.  The result lives where the
    sensing rows live (``device`` for host rows)."""
    if isinstance(osense_rows, torch.Tensor):
        device = osense_rows.device
    s = _host(osense_rows)
    if s.ndim != 3 or s.shape[2] != LB.OSENSE_NP:
        raise ValueError("obstacle sensing rows must be [B, nObst, 3]")
    floor = [float(v) for v in floor]
    q = [float(v) for v in q]
    if len(floor) != 3 or len(q) != 5:
        raise ValueError("floor holds three values: pos, heading, speed; q five: pos, heading, "
                         "speed, yaw, accel")
    if not all(np.isfinite(v) and v > 0.0 for v in floor):
        raise ValueError("every floor must be finite and > 0")
    out = np.empty(s.shape[:2] + (NP,))
    for k in range(3):
        out[..., _R[k]] = np.maximum(s[..., k], floor[k])
    for k in range(5):
        out[..., LB.TRKA_Q_POS + k] = q[k]
    out[..., LB.TRKA_P0_YAW] = float(p0_yaw)
    out[..., LB.TRKA_P0_ACCEL] = float(p0_accel)
    out[..., LB.TRKA_W_CLAMP] = float(w_clamp)
    out[..., LB.TRKA_A_CLAMP] = float(a_clamp)
    out[..., LB.TRKA_W_HOLD] = float(w_hold)
    out[..., LB.TRKA_A_HOLD] = float(a_hold)
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def from_table(rows, index, device=None):
    """rows [K, nObst, 14], index [B] -> the tuning [B, nObst, 14] with realisation b holding
    rows[index[b]] (a discrete study: K candidate tunings)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nObst, 14]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(rows):
    """ValueError on rows the device would treat as bad (include/scpqp_tracker_accel.h): a
    non-finite or negative field, or a row that is not off with some r_* = 0.  The message
    names the row and the field.  Host side: one copy of the array."""
    t = _host(rows)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("rows must be [B, nObst, 14]")
    bad = np.argwhere(~np.isfinite(t))
    if len(bad):
        b, o, f = bad[0]
        raise ValueError(f"rows[{b}, {o}]: {FIELDS[f]} is not finite")
    bad = np.argwhere(t < 0.0)
    if len(bad):
        b, o, f = bad[0]
        raise ValueError(f"rows[{b}, {o}]: {FIELDS[f]} must be >= 0")
    on = (t != 0.0).any(axis=2)
    for f in _R:
        bad = np.argwhere(on & (t[..., f] == 0.0))
        if len(bad):
            b, o = bad[0]
            raise ValueError(f"rows[{b}, {o}]: {FIELDS[f]} must be > 0 in a row that is not off")


def alloc(B, n_obst, device=None):
    """(x_trk [B, nObst, 6] filled with NaN: no lane is initialised, cov [B, nObst, 6, 6] of
    zeros): what ``step`` carries from one MPC step to the next."""
    _need_obstacles(int(n_obst))
    device = torch.device(device or "cuda")
    x_trk = torch.full((int(B), int(n_obst), NS), float("nan"), dtype=torch.float64, device=device)
    cov = torch.zeros((int(B), int(n_obst), NS, NS), dtype=torch.float64, device=device)
    return x_trk, cov


def _gpu(t, what, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda \
            or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float64 {list(shape)} tensor on the GPU")
    return t


def step(rows, osense, seed, epoch, b_offset, trk, t_meas, t_since, lead, dt, hp, x_trk, cov):
    """One tracker step of every lane (scpqp_obstacles_track_accel): measure the obstacle
    truth ``rows`` [B, nObst, 7] at ``t_meas`` through ``osense`` [B, nObst, 3] (None: the
    exact sensor; then ``seed``, ``epoch`` and ``b_offset`` are not read) as
    ``sensing.predict_sensed`` does, predict the filter over ``t_since`` seconds, initialise on
    or correct with the measurement, and predict the horizon.  ``trk`` [B, nObst, 14];
    ``x_trk`` [B, nObst, 6] and ``cov`` [B, nObst, 6, 6] are updated in place.  Returns
    ``(obst [B, nObst, 2, hp], z [B, nObst, 4], nis [B, nObst])``: the controller's prediction,
    the measurement, and the normalised innovation squared of the lanes that corrected (NaN
    elsewhere).  Every array is a device tensor."""
    from .obstacles import _rows_arg
    from .plant import _ptr, _stream
    from .sensing import _stream_struct
    rows = _rows_arg(rows)
    B, nO = int(rows.shape[0]), int(rows.shape[1])
    trk = _gpu(trk, "trk", (B, nO, NP))
    x_trk = _gpu(x_trk, "x_trk", (B, nO, NS))
    cov = _gpu(cov, "cov", (B, nO, NS, NS))
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
    z = torch.empty((B, nO, NZ), **f)
    nis = torch.empty((B, nO), **f)
    LB.check(lib.scpqp_obstacles_track_accel(B, nO, int(hp), _ptr(rows), _ptr(osense), st,
                                             _ptr(trk), float(t_meas), t_since, float(lead),
                                             float(dt), _ptr(x_trk), _ptr(cov), _ptr(z),
                                             _ptr(nis), _ptr(obst), _stream(rows.device)), lib)
    return obst, z, nis
