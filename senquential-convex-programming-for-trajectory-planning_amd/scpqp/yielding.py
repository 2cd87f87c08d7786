"""Right of way and graded braking for the speed governor: a longitudinal command per
(realisation, vehicle) from the planner's own plan (include/scpqp_yield.h; csrc/yield.hip).

A tuning is a float64 tensor ``[B, nVeh, 10]`` of rows: the governor's seven fields
(scpqp/governor.py) and ``(prio, a_ease, s_stand)``: the rank (the larger has right of way), the
gentlest deceleration commanded on a conflict, and the speed at or below which another vehicle
is standing and is yielded to whatever its rank (0: no such rule)
(``ClosedLoopBatch.reset(..., right_of_way=)``).  In a conflict between two vehicles' plans only
the outranked one brakes, with the deceleration that stops it at the last plan point before the
conflict, between ``a_ease`` and ``a_brake``.  Equal ranks, ``a_ease = a_brake`` and
``s_stand = 0`` give the governor, bit for bit.

``off``            the rows without a governor: the acceleration stays what it is, bitwise
``rows``           rows from scalars or arrays per field
``from_governor``  governor rows and ranks
``from_table``     rows gathered from a table of K candidates, for discrete studies
``validate``       host-side check of the rows before a rollout
``required``       the required centre distances (``governor.required``)
``step``           one step of every lane (scpqp_yield_step)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as LB
from . import governor as GOV
from .governor import _gpu, _host, _need_vehicles, _per_batch, required  # noqa: F401

NP = LB.YLD_NP
FIELDS = LB.YLD_FIELDS


def off(B, n_veh, device=None):
    """[B, nVeh, 10] of zeros: no governor, the acceleration state is left alone."""
    _need_vehicles(int(n_veh))
    return torch.zeros((int(B), int(n_veh), NP), dtype=torch.float64,
                       device=torch.device(device or "cuda"))


def is_off(rows):
    """True when every row is exactly the off row (host side)."""
    return bool((_host(rows) == 0.0).all())


def rows(B, n_veh, v_ref, a_acc, a_brake, k_v, look, prio, j_max=float("inf"), band=0.0,
         a_ease=None, s_stand=0.0, device=None):
    """[B, nVeh, 10] from one value per field: a scalar, or an array that broadcasts to
    [B, nVeh] (``[nVeh]``: one value per vehicle, the shape of a ranking).  ``a_ease=None``
    means ``a_brake``: full braking on every counted conflict.  Validated."""
    B, n_veh = int(B), int(n_veh)
    _need_vehicles(n_veh)
    out = np.empty((B, n_veh, NP))
    vals = (v_ref, a_acc, a_brake, k_v, j_max, look, band, prio,
            a_brake if a_ease is None else a_ease, s_stand)
    for f, val in enumerate(vals):
        try:
            out[..., f] = np.broadcast_to(np.asarray(_host(val), float), (B, n_veh))
        except ValueError:
            raise ValueError(f"{FIELDS[f]} does not broadcast to [B, nVeh] = [{B}, {n_veh}]") from None
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def from_governor(gov_rows, prio, a_ease=None, s_stand=0.0, device=None):
    """Governor rows [B, nVeh, 7] and ranks (a scalar, or an array that broadcasts to
    [B, nVeh]) -> [B, nVeh, 10].  With ``a_ease=None`` (= each row's ``a_brake``), equal ranks
    and ``s_stand = 0`` the result reduces to the governor.  An off governor row stays an off
    row.  Validated."""
    device = torch.device(device or (gov_rows.device if isinstance(gov_rows, torch.Tensor) else "cuda"))
    g = np.array(_host(gov_rows), float)
    if g.ndim != 3 or g.shape[2] != GOV.NP:
        raise ValueError("governor rows must be [B, nVeh, 7]")
    B, nV = g.shape[:2]
    out = np.zeros((B, nV, NP))
    out[..., :GOV.NP] = g
    extra = (prio, g[..., LB.GOV_A_BRAKE] if a_ease is None else a_ease, s_stand)
    for f, val in zip((LB.YLD_PRIO, LB.YLD_A_EASE, LB.YLD_S_STAND), extra):
        try:
            out[..., f] = np.broadcast_to(np.asarray(_host(val), float), (B, nV))
        except ValueError:
            raise ValueError(f"{FIELDS[f]} does not broadcast to [B, nVeh] = [{B}, {nV}]") from None
    out[(g == 0.0).all(axis=2)] = 0.0
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=device)


def from_table(rows, index, device=None):
    """rows [K, nVeh, 10], index [B] -> the tuning [B, nVeh, 10] with realisation b holding
    rows[index[b]] (a discrete study: K candidate tunings)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nVeh, 10]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(rows):
    """ValueError on rows the device would treat as bad (include/scpqp_yield.h): the governor's
    rules on the first seven fields, a rank that is not an integer in 0 .. 2^20, a negative or
    non-finite a_ease or s_stand, or a_ease above a_brake.  The message names the row and the
    field.  Host side: one copy of the array."""
    t = _host(rows)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("rows must be [B, nVeh, 10]")
    GOV.validate(t[..., :GOV.NP])
    for f in (LB.YLD_PRIO, LB.YLD_A_EASE, LB.YLD_S_STAND):
        bad = np.argwhere(~np.isfinite(t[..., f]))
        if len(bad):
            b, v = bad[0]
            raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} is not finite")
        bad = np.argwhere(t[..., f] < 0.0)
        if len(bad):
            b, v = bad[0]
            raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} must be >= 0")
    prio = t[..., LB.YLD_PRIO]
    bad = np.argwhere((prio != np.floor(prio)) | (prio > LB.YLD_PRIO_MAX))
    if len(bad):
        b, v = bad[0]
        raise ValueError(f"rows[{b}, {v}]: prio must be an integer in 0..{LB.YLD_PRIO_MAX}")
    bad = np.argwhere(t[..., LB.YLD_A_EASE] > t[..., LB.GOV_A_BRAKE])
    if len(bad):
        b, v = bad[0]
        raise ValueError(f"rows[{b}, {v}]: a_ease must be <= a_brake")


def step(rows, x0, traj, obst, obst_margin, dreq_obs, dreq_veh, t_hold, t_back, hp=None,
         hp_max=None, diag=True):
    """One step of every lane (scpqp_yield_step), after the solve of the same MPC step.  The
    arguments are those of ``governor.step`` with ``rows`` [B, nVeh, 10].  Returns ``(a_cmd,
    k_conf int32, clear, k_any int32, who int32, d_stop)``, each [B, nVeh]: the governor's three
    first; with ``diag=False`` only ``a_cmd`` is computed and the others are None.  Device
    tensors."""
    from .plant import _ptr, _stream
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3:
        raise ValueError("rows must be a float64 [B, nVeh, 10] tensor on the GPU")
    B, nV = int(rows.shape[0]), int(rows.shape[1])
    _need_vehicles(nV)
    f64, i32 = torch.float64, torch.int32
    rows = _gpu(rows, "rows", f64, B * nV * NP, [B, nV, NP])
    if rows.shape[2] != NP:
        raise ValueError("rows must be a float64 [B, nVeh, 10] tensor on the GPU")
    x0 = _gpu(x0, "x0", f64, B * nV * 6, [B, nV, 6])
    if hp_max is None:
        if not isinstance(traj, torch.Tensor) or traj.dim() != 4:
            raise ValueError("traj must be [B, Hp, 2, nVeh], or pass hp_max with its slots")
        hp_max = int(traj.shape[1])
    hp_max = int(hp_max)
    traj = _gpu(traj, "traj", f64, B * hp_max * 2 * nV, [B, hp_max, 2, nV])
    nO = 0
    if obst is not None:
        if not isinstance(obst, torch.Tensor) or obst.dim() < 2:
            raise ValueError("obst must be a float64 [B, nObst, 2, Hp] tensor on the GPU")
        nO = int(obst.shape[1])
    if nO:
        obst = _gpu(obst, "obst", f64, B * nO * 2 * hp_max, [B, nO, 2, hp_max])
        if obst_margin is not None:
            obst_margin = _gpu(obst_margin, "obst_margin", f64, B * nO * hp_max, [B, nO, hp_max])
        dreq_obs = _per_batch(dreq_obs, "dreq_obs", B, (nV, nO))
        _gpu(dreq_obs, "dreq_obs", f64, B * nV * nO, [B, nV, nO])
    else:
        obst = obst_margin = dreq_obs = None
    dreq_veh = _gpu(_per_batch(dreq_veh, "dreq_veh", B, (nV, nV)), "dreq_veh", f64, B * nV * nV,
                    [B, nV, nV])
    if hp is not None:
        hp = _gpu(hp, "hp", i32, B, [B])
    new = lambda dt: torch.empty((B, nV), dtype=dt, device=rows.device) if diag else None
    a_cmd = torch.empty((B, nV), dtype=f64, device=rows.device)
    k_conf, k_any, who, clear, d_stop = new(i32), new(i32), new(i32), new(f64), new(f64)
    lib = LB.load()
    LB.check(lib.scpqp_yield_step(nV, nO, hp_max, B, float(t_hold), float(t_back), _ptr(x0),
                                  _ptr(traj), _ptr(obst), _ptr(obst_margin), _ptr(hp),
                                  _ptr(dreq_obs), _ptr(dreq_veh), _ptr(rows), _ptr(a_cmd),
                                  _ptr(k_conf), _ptr(k_any), _ptr(who), _ptr(clear), _ptr(d_stop),
                                  _stream(rows.device)), lib)
    return a_cmd, k_conf, clear, k_any, who, d_stop
