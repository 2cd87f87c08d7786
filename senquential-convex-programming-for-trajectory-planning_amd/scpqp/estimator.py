"""State estimator: an extended Kalman filter per (realisation, vehicle) between the sensor
and the planner (include/scpqp_estimator.h; csrc/estimator.hip).

An estimator tuning is a float64 tensor ``[B, nVeh, 8]`` of rows ``(r_pos, r_heading, r_speed,
r_steer, q_pos, q_heading, q_speed, q_steer)``: the sigmas the filter assumes of the measured
position, heading, speed and steering angle, and its process-noise densities on the same
states (``ClosedLoopBatch.reset(..., estimator=)``).  The filter predicts with the
controller's nominal model and the commands the controller issued, and corrects with every
measurement that arrives; it knows nothing of the sensor's lag, compass offset or odometer
scale.  A row per lane: a tuning sweep runs in one batch.

``off``         the rows without a filter: the measurement goes through, bitwise
``rows``        rows from scalars or arrays per field
``matched``     rows whose R is a sensing truth's own sigmas, raised to a floor (R must be > 0)
``from_table``  rows gathered from a table of K candidates, for discrete studies
``validate``    host-side check of the rows before a rollout
``alloc``       the state a filter carries between steps: a NaN estimate and a covariance
``step``        one filter step of every lane (scpqp_est_step)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as LB
from . import plant as PL

NP = LB.EST_NP
NS = LB.EST_NS
FIELDS = LB.EST_FIELDS
_R = (LB.EST_R_POS, LB.EST_R_HEADING, LB.EST_R_SPEED, LB.EST_R_STEER)
# R may not be 0: the smallest sigmas `matched` assumes of a sensor that reports none
FLOOR = (1e-3, 1e-3, 1e-3, 1e-3)
# a small allowance for what the nominal model leaves out, per sqrt(second)
Q_DEFAULT = (0.02, 0.01, 0.05, 0.01)


def _need_vehicles(nV):
    if not 1 <= nV <= LB.MAX_VEH:
        raise ValueError(f"an estimator needs 1..{LB.MAX_VEH} vehicles, got {nV}")


def _host(rows):
    return rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, float)


def off(B, n_veh, device=None):
    """[B, nVeh, 8] of zeros: no filter, the measurement is the estimate."""
    _need_vehicles(int(n_veh))
    return torch.zeros((int(B), int(n_veh), NP), dtype=torch.float64,
                       device=torch.device(device or "cuda"))


def is_off(rows):
    """True when every row is exactly the off row (host side)."""
    return bool((_host(rows) == 0.0).all())


def rows(B, n_veh, r_pos=0.05, r_heading=0.01, r_speed=0.1, r_steer=0.01, q_pos=Q_DEFAULT[0],
         q_heading=Q_DEFAULT[1], q_speed=Q_DEFAULT[2], q_steer=Q_DEFAULT[3], device=None):
    """[B, nVeh, 8] from one value per field: a scalar, or an array that broadcasts to
    [B, nVeh] (``[B, 1]``: one tuning per realisation, the shape of a sweep).  Validated."""
    B, n_veh = int(B), int(n_veh)
    _need_vehicles(n_veh)
    out = np.empty((B, n_veh, NP))
    for f, val in enumerate((r_pos, r_heading, r_speed, r_steer, q_pos, q_heading, q_speed,
                             q_steer)):
        try:
            out[..., f] = np.broadcast_to(np.asarray(_host(val), float), (B, n_veh))
        except ValueError:
            raise ValueError(f"{FIELDS[f]} does not broadcast to [B, nVeh] = [{B}, {n_veh}]") from None
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def matched(sensing_rows, floor=FLOOR, q=Q_DEFAULT, device=None):
    """Rows for a sensing truth ``[B, nVeh, 8]`` (scpqp/sensing.py): R_* is the sensor's own
    sigma of that field, raised to ``floor`` = (pos, heading, speed, steer) since R must be > 0,
    and Q_* is ``q`` = (pos, heading, speed, steer).  The result lives where the sensing rows
    live (``device`` for host rows)."""
    if isinstance(sensing_rows, torch.Tensor):
        device = sensing_rows.device
    s = _host(sensing_rows)
    if s.ndim != 3 or s.shape[2] != LB.SENSE_NP:
        raise ValueError("sensing rows must be [B, nVeh, 8]")
    floor = [float(v) for v in floor]
    q = [float(v) for v in q]
    if len(floor) != 4 or len(q) != 4:
        raise ValueError("floor and q hold four values: pos, heading, speed, steer")
    if not all(np.isfinite(v) and v > 0.0 for v in floor):
        raise ValueError("every floor must be finite and > 0")
    sig = (LB.SENSE_SIG_POS, LB.SENSE_SIG_HEADING, LB.SENSE_SIG_SPEED, LB.SENSE_SIG_STEER)
    out = np.empty(s.shape[:2] + (NP,))
    for k in range(4):
        out[..., _R[k]] = np.maximum(s[..., sig[k]], floor[k])
        out[..., 4 + k] = q[k]
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def from_table(rows, index, device=None):
    """rows [K, nVeh, 8], index [B] -> the tuning [B, nVeh, 8] with realisation b holding
    rows[index[b]] (a discrete study: K candidate tunings)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nVeh, 8]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(rows):
    """ValueError on rows the device would treat as bad (include/scpqp_estimator.h): a
    non-finite or negative field, or a row that is not off with some r_* = 0.  The message
    names the row and the field.  Host side: one copy of the array."""
    t = _host(rows)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("rows must be [B, nVeh, 8]")
    bad = np.argwhere(~np.isfinite(t))
    if len(bad):
        b, v, f = bad[0]
        raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} is not finite")
    bad = np.argwhere(t < 0.0)
    if len(bad):
        b, v, f = bad[0]
        raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} must be >= 0")
    on = (t != 0.0).any(axis=2)
    for f in _R:
        bad = np.argwhere(on & (t[..., f] == 0.0))
        if len(bad):
            b, v = bad[0]
            raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} must be > 0 in a row that is not off")


def alloc(B, n_veh, device=None):
    """(x_est [B, nVeh, 6] filled with NaN: no lane is initialised, cov [B, nVeh, 5, 5] of
    zeros): what ``step`` carries from one MPC step to the next."""
    _need_vehicles(int(n_veh))
    device = torch.device(device or "cuda")
    x_est = torch.full((int(B), int(n_veh), 6), float("nan"), dtype=torch.float64, device=device)
    cov = torch.zeros((int(B), int(n_veh), NS, NS), dtype=torch.float64, device=device)
    return x_est, cov


def _gpu(t, what, dtype, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda \
            or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        kind = "float64" if dtype == torch.float64 else "int32"
        raise ValueError(f"{what} must be a contiguous {kind} {list(shape)} tensor on the GPU")
    return t


def step(params, u_span, tick, x_meas, delivered, rows, x_est, cov, nis=None, h_max=PL.H_MAX):
    """One filter step of every lane (scpqp_est_step): predict over the ``n_span`` ticks of
    ``u_span`` [B, nVeh, n_span] (the command that acted over each tick since the previous
    call; None or n_span = 0: no prediction), then initialise on or correct with ``x_meas``
    [B, nVeh, 6] where ``delivered`` (int32 [B, nVeh]; None: everywhere) is 1.  ``x_est``
    [B, nVeh, 6] and ``cov`` [B, nVeh, 5, 5] are updated in place.  Returns ``nis``
    [B, nVeh], the normalised innovation squared of the lanes that corrected (NaN elsewhere);
    pass a tensor to have it written there.  Every array is a device tensor."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3:
        raise ValueError("rows must be a float64 [B, nVeh, 8] tensor on the GPU")
    B, nV = int(rows.shape[0]), int(rows.shape[1])
    if nV != params.n_veh:
        raise ValueError("rows and params disagree on the number of vehicles")
    rows = _gpu(rows, "rows", torch.float64, (B, nV, NP))
    x_meas = _gpu(x_meas, "x_meas", torch.float64, (B, nV, 6))
    x_est = _gpu(x_est, "x_est", torch.float64, (B, nV, 6))
    cov = _gpu(cov, "cov", torch.float64, (B, nV, NS, NS))
    n_span = 0
    if u_span is not None:
        if not isinstance(u_span, torch.Tensor) or u_span.dim() != 3:
            raise ValueError("u_span must be a float64 [B, nVeh, n_span] tensor on the GPU")
        n_span = int(u_span.shape[2])
        u_span = _gpu(u_span, "u_span", torch.float64, (B, nV, n_span)) if n_span else None
    if delivered is not None:
        delivered = _gpu(delivered, "delivered", torch.int32, (B, nV))
    if nis is None:
        nis = torch.empty((B, nV), dtype=torch.float64, device=rows.device)
    else:
        nis = _gpu(nis, "nis", torch.float64, (B, nV))
    lib = LB.load()
    LB.check(lib.scpqp_est_step(C.byref(params), B, n_span, float(tick), float(h_max), PL._ptr(u_span),
                                PL._ptr(x_meas), PL._ptr(delivered), PL._ptr(rows),
                                PL._ptr(x_est), PL._ptr(cov), PL._ptr(nis),
                                PL._stream(rows.device)), lib)
    return nis
