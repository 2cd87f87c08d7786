"""Speed governor: a longitudinal command per (realisation, vehicle) from the planner's own
plan (include/scpqp_governor.h; csrc/governor.hip).

A governor tuning is a float64 tensor ``[B, nVeh, 7]`` of rows ``(v_ref, a_acc, a_brake, k_v,
j_max, look, band)``: the cruise speed, the largest acceleration and deceleration, the gain of
the speed loop, the slew limit of the command (``inf``: none), how many plan steps are examined
and the clearance demanded on top of the required distance
(``ClosedLoopBatch.reset(..., governor=)``).  When one of the plan's first ``look`` points comes
closer to a told obstacle point or to another vehicle's plan than the required distance plus
``band``, the vehicle brakes with ``a_brake``; otherwise it returns to ``v_ref``.  A row per
lane: a tuning sweep runs in one batch.

``off``         the rows without a governor: the acceleration stays what it is, bitwise
``rows``        rows from scalars or arrays per field
``from_table``  rows gathered from a table of K candidates, for discrete studies
``validate``    host-side check of the rows before a rollout
``required``    the required centre distances of a scenario (or of each realisation's variant)
``step``        one governor step of every lane (scpqp_governor_step)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as LB

NP = LB.GOV_NP
FIELDS = LB.GOV_FIELDS


def _need_vehicles(nV):
    if not 1 <= nV <= LB.MAX_VEH:
        raise ValueError(f"a governor needs 1..{LB.MAX_VEH} vehicles, got {nV}")


def _host(rows):
    return rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, float)


def off(B, n_veh, device=None):
    """[B, nVeh, 7] of zeros: no governor, the acceleration state is left alone."""
    _need_vehicles(int(n_veh))
    return torch.zeros((int(B), int(n_veh), NP), dtype=torch.float64,
                       device=torch.device(device or "cuda"))


def is_off(rows):
    """True when every row is exactly the off row (host side)."""
    return bool((_host(rows) == 0.0).all())


def rows(B, n_veh, v_ref, a_acc, a_brake, k_v, look, j_max=float("inf"), band=0.0, device=None):
    """[B, nVeh, 7] from one value per field: a scalar, or an array that broadcasts to
    [B, nVeh] (``[nVeh]``: one value per vehicle; ``[B, 1]``: one tuning per realisation, the
    shape of a sweep).  Validated."""
    B, n_veh = int(B), int(n_veh)
    _need_vehicles(n_veh)
    out = np.empty((B, n_veh, NP))
    for f, val in enumerate((v_ref, a_acc, a_brake, k_v, j_max, look, band)):
        try:
            out[..., f] = np.broadcast_to(np.asarray(_host(val), float), (B, n_veh))
        except ValueError:
            raise ValueError(f"{FIELDS[f]} does not broadcast to [B, nVeh] = [{B}, {n_veh}]") from None
    validate(out)
    return torch.as_tensor(out, dtype=torch.float64, device=torch.device(device or "cuda"))


def from_table(rows, index, device=None):
    """rows [K, nVeh, 7], index [B] -> the tuning [B, nVeh, 7] with realisation b holding
    rows[index[b]] (a discrete study: K candidate tunings)."""
    device = torch.device(device or (rows.device if isinstance(rows, torch.Tensor) else "cuda"))
    rows = torch.as_tensor(rows, dtype=torch.float64, device=device)
    if rows.dim() != 3 or rows.shape[2] != NP:
        raise ValueError("rows must be [K, nVeh, 7]")
    idx = torch.as_tensor(index, device=device).reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError("index outside the table")
    return rows[idx].contiguous()


def validate(rows):
    """ValueError on rows the device would treat as bad (include/scpqp_governor.h): a negative
    field, a non-finite one other than j_max = inf, or a look that is not an integer or lies
    above the largest horizon.  The message names the row and the field.  Host side: one copy
    of the array."""
    t = _host(rows)
    if t.ndim != 3 or t.shape[2] != NP:
        raise ValueError("rows must be [B, nVeh, 7]")
    fin = np.isfinite(t)
    fin[..., LB.GOV_J_MAX] |= t[..., LB.GOV_J_MAX] == np.inf
    bad = np.argwhere(~fin)
    if len(bad):
        b, v, f = bad[0]
        raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} is not finite")
    bad = np.argwhere(t < 0.0)
    if len(bad):
        b, v, f = bad[0]
        raise ValueError(f"rows[{b}, {v}]: {FIELDS[f]} must be >= 0")
    look = t[..., LB.GOV_LOOK]
    bad = np.argwhere((look != np.floor(look)) | (look > LB.MAX_HP))
    if len(bad):
        b, v = bad[0]
        raise ValueError(f"rows[{b}, {v}]: look must be an integer in 0..{LB.MAX_HP}")


def required(scenario, variants=None, variant_of=None, device=None):
    """(dreq_obs [1 | B, nVeh, nObst], dreq_veh [1 | B, nVeh, nVeh]) float64 device tensors: the
    required centre distances ``dsafeObstacles`` and ``dsafeVehicles`` of the scenario, the
    distances of ``evaluateInOriginalProblem`` (without ``dsafeExtra``).  With ``variants`` (a
    list of scenarios) and ``variant_of`` [B], realisation b holds those of
    ``variants[variant_of[b]]``; without, the leading extent is 1 and ``step`` repeats it."""
    device = torch.device(device or "cuda")
    if variants is None and variant_of is not None:
        raise ValueError("variant_of needs variants")
    if variants is not None and variant_of is None:
        raise ValueError("variants needs variant_of [B]")
    nV, nO = int(scenario.nVeh), int(scenario.nObst)
    scs = [scenario] if variants is None else list(variants)
    f = dict(dtype=torch.float64, device=device)
    dv = torch.as_tensor(np.stack([np.asarray(sc.dsafeVehicles, float).reshape(nV, nV)
                                   for sc in scs]), **f)
    do = torch.as_tensor(np.stack([np.asarray(sc.dsafeObstacles, float).reshape(nV, nO)
                                   if nO else np.zeros((nV, 0)) for sc in scs]), **f)
    if variants is not None:
        idx = torch.as_tensor(variant_of, device=device).reshape(-1).long()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(scs)):
            raise ValueError("variant_of indexes outside variants")
        dv, do = dv[idx], do[idx]
    return do.contiguous(), dv.contiguous()


def _gpu(t, what, dtype, numel, shape_text):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda \
            or t.numel() != numel or not t.is_contiguous():
        kind = "float64" if dtype == torch.float64 else "int32"
        raise ValueError(f"{what} must be a contiguous {kind} {shape_text} tensor on the GPU")
    return t


def _per_batch(t, what, B, tail):
    """[1 | B, *tail] -> contiguous [B, *tail]."""
    if not isinstance(t, torch.Tensor) or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail \
            or t.shape[0] not in (1, B):
        raise ValueError(f"{what} must be a [1 | B, {', '.join(map(str, tail))}] tensor")
    return t.expand((B,) + tail).contiguous()


def step(rows, x0, traj, obst, obst_margin, dreq_obs, dreq_veh, t_hold, t_back, hp=None,
         hp_max=None, diag=True):
    """One governor step of every lane (scpqp_governor_step), after the solve of the same MPC
    step.  ``rows`` [B, nVeh, 7]; ``x0`` [B, nVeh, 6] the state the plan starts from; ``traj``
    the solve's output ([B, Hp, 2, nVeh], or its slots with ``hp_max`` given); ``obst``
    [B, nObst, 2, Hp] and ``obst_margin`` [B, nObst, Hp] what the solve was given (None: no
    obstacle, no margin); ``dreq_obs``, ``dreq_veh``: ``required(...)``; ``hp`` int32 [B] or
    None.  Returns ``(a_cmd [B, nVeh], k_conf int32 [B, nVeh], clear [B, nVeh])``; with
    ``diag=False`` only ``a_cmd`` is computed and the other two are None.  Device tensors."""
    from .plant import _ptr, _stream
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3:
        raise ValueError("rows must be a float64 [B, nVeh, 7] tensor on the GPU")
    B, nV = int(rows.shape[0]), int(rows.shape[1])
    _need_vehicles(nV)
    f64, i32 = torch.float64, torch.int32
    rows = _gpu(rows, "rows", f64, B * nV * NP, [B, nV, NP])
    if rows.shape[2] != NP:
        raise ValueError("rows must be a float64 [B, nVeh, 7] tensor on the GPU")
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
    a_cmd = torch.empty((B, nV), dtype=f64, device=rows.device)
    k_conf = torch.empty((B, nV), dtype=i32, device=rows.device) if diag else None
    clear = torch.empty((B, nV), dtype=f64, device=rows.device) if diag else None
    lib = LB.load()
    LB.check(lib.scpqp_governor_step(nV, nO, hp_max, B, float(t_hold), float(t_back), _ptr(x0),
                                     _ptr(traj), _ptr(obst), _ptr(obst_margin), _ptr(hp),
                                     _ptr(dreq_obs), _ptr(dreq_veh), _ptr(rows), _ptr(a_cmd),
                                     _ptr(k_conf), _ptr(clear), _stream(rows.device)), lib)
    return a_cmd, k_conf, clear
