"""The bicycle plant around the solve, batched on the GPU (csrc/plant.hip).

``delay_compensate``  IterClass delay compensation (MPC_Iter.py:24-33)
``plant_step``        closed-loop plant simulation of one MPC step (main.py:176-191)
``clip_controls``     steering-limit enforcement (main.py:164-174)
``NoiseStream``       seed, sigma and counter part of the reference's model noise
                      (Model.py:84-86), drawn on the device per right-hand-side
                      evaluation (include/scpqp_noise.h); ``rng=`` of the two
                      integrators, and ``draw_ec_noise`` for the solve's ec_noise
``plant_step(..., truth=)``  the plant step with a truth row per (realisation, vehicle)
                      (include/scpqp_truth.h; rows from scpqp/truth.py)
``plant_step(..., drive=, a_cmd=)``  the same behind a longitudinal actuator per
                      (realisation, vehicle) (include/scpqp_drive.h; rows from scpqp/drive.py)

Arrays are torch-ROCm float64 tensors on the GPU; PyTorch only provides the
memory and the stream.  The reference integrates with scipy (odeint / dopri5);
the kernels use fixed-step RK4 with steps of at most ``h_max`` seconds (default
2.5 ms: ~1e-11 from the exact flow, below the reference's 1e-8 tolerances).
There is no CPU path: without the HIP library or a GPU these raise.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as LB

H_MAX = 2.5e-3
STEER_TAU = 0.1       # Model.py:83: dx[5] = (u_ref - u) / 0.1
DELAY_STEPS = 10      # MPC_Iter.py:21: outputs of the delay-compensation trajectory


SIGMA_NOISE = 3e-6    # Model.py:85-86: np.random.normal(0, 0.000003)


class NoiseStream:
    """The reference's per-evaluation model noise as a counter-based stream: ``seed`` keys
    the generator, ``epoch`` is the MPC step index and ``b_offset`` the global index of the
    call's first realisation (a rank holding realisations [r * per_rank, (r + 1) * per_rank)
    passes ``b_offset = r * per_rank``), so a realisation's draws do not depend on how the
    batch is split.  ``at(epoch)`` gives the stream of another step."""

    def __init__(self, seed, sigma=SIGMA_NOISE, epoch=0, b_offset=0):
        self.seed, self.epoch, self.b_offset = int(seed), int(epoch), int(b_offset)
        self.sigma = float(sigma)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2**64)")
        if not (0.0 <= self.sigma < float("inf")):
            raise ValueError("sigma must be finite and >= 0")
        if not 0 <= self.epoch < 2 ** 32 or not 0 <= self.b_offset < 2 ** 32:
            raise ValueError("epoch and b_offset must be in [0, 2**32)")

    def at(self, epoch):
        return NoiseStream(self.seed, self.sigma, epoch, self.b_offset)

    def c_struct(self):
        return LB.Noise(seed=self.seed, sigma=self.sigma, epoch=self.epoch, b_offset=self.b_offset)


def _one_noise_source(noise, rng):
    if noise is not None and rng is not None:
        raise ValueError("pass either noise (constant terms) or rng (a NoiseStream), not both")
    if rng is not None and not isinstance(rng, NoiseStream):
        raise TypeError("rng must be a NoiseStream")


def plant_params(lf, lr):
    """scpqp_plant_params for per-vehicle axle distances (Model.py:26-27)."""
    lf = [float(v) for v in lf]
    lr = [float(v) for v in lr]
    if not 1 <= len(lf) <= LB.MAX_VEH or len(lr) != len(lf):
        raise ValueError("need 1..16 vehicles with lf and lr each")
    p = LB.PlantParams()
    p.n_veh = len(lf)
    for v in range(len(lf)):
        p.lf[v] = lf[v]
        p.lr[v] = lr[v]
    return p


def _dev(t, device):
    return torch.as_tensor(t, dtype=torch.float64, device=device).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def delay_compensate(params, x_meas, u_hold, horizon, n_out=DELAY_STEPS, noise=None, h_max=H_MAX,
                     device=None, want_traj=True, rng=None):
    """x_meas [B, nVeh, 6], u_hold [B, nVeh] -> (x0 [B, nVeh, 6],
    traj [B, n_out, 6, nVeh] or None): MPC_Iter.py:24-33 for every problem.
    ``noise`` [B, nVeh, 2]: constant terms of dx[0], dx[1]; ``rng`` (a NoiseStream):
    the reference's noise, drawn anew per right-hand-side evaluation."""
    _one_noise_source(noise, rng)
    device = torch.device(device or "cuda")
    lib = LB.load()
    x = _dev(x_meas, device)
    u = _dev(u_hold, device)
    B, V = int(x.shape[0]), params.n_veh
    if tuple(x.shape) != (B, V, 6) or tuple(u.shape) != (B, V):
        raise ValueError("x_meas must be [B, nVeh, 6] and u_hold [B, nVeh]")
    nz = None if noise is None else _dev(noise, device)
    if nz is not None and tuple(nz.shape) != (B, V, 2):
        raise ValueError("noise must be [B, nVeh, 2]")
    x0 = torch.empty((B, V, 6), dtype=torch.float64, device=device)
    traj = torch.empty((B, n_out, 6, V), dtype=torch.float64, device=device) if want_traj else None
    if rng is not None:
        ns = rng.c_struct()
        LB.check(lib.scpqp_delay_compensate_noisy(C.byref(params), B, float(horizon), int(n_out),
                                                  _ptr(x), _ptr(u), C.byref(ns), _ptr(x0),
                                                  _ptr(traj), float(h_max), _stream(device)), lib)
        return x0, traj
    LB.check(lib.scpqp_delay_compensate(C.byref(params), B, float(horizon), int(n_out), _ptr(x),
                                        _ptr(u), _ptr(nz), _ptr(x0), _ptr(traj), float(h_max),
                                        _stream(device)), lib)
    return x0, traj


def plant_step(params, x_start, u_tick, tick, noise=None, h_max=H_MAX, device=None, rng=None,
               truth=None, drive=None, a_cmd=None):
    """x_start [B, nVeh, 6], u_tick [B, nVeh, K] (K = ticks_per_sim + 1) ->
    x_path [B, nVeh, K, 6]: main.py:184-191 (output k integrated from t0 over
    k ticks with the constant control u_tick[..., k]).  ``noise`` / ``rng`` as in
    delay_compensate; with ``rng`` every output tick k has its own noise stream, as
    every restart of the reference's integrator consumes fresh draws.  ``truth``
    [B, nVeh, 5]: the plant parameters of every (realisation, vehicle)
    (include/scpqp_truth.h; scpqp/truth.py) instead of ``params``' geometry and the
    nominal steering lag.  delay_compensate takes none: it is the controller's prediction.
    ``drive`` [B, nVeh, 6] with ``a_cmd`` [B, nVeh]: the longitudinal actuator of every
    (realisation, vehicle) and the acceleration commanded over the step
    (include/scpqp_drive.h; scpqp/drive.py); x_start[..., 4] is then the realised
    acceleration.  One without the other is refused; without ``truth`` the nominal rows are
    filled in."""
    _one_noise_source(noise, rng)
    if (drive is None) != (a_cmd is None):
        raise ValueError("drive and a_cmd go together: pass both or neither")
    device = torch.device(device or "cuda")
    lib = LB.load()
    x = _dev(x_start, device)
    u = _dev(u_tick, device)
    B, V = int(x.shape[0]), params.n_veh
    K = int(u.shape[-1])
    if tuple(x.shape) != (B, V, 6) or tuple(u.shape) != (B, V, K) or K < 1:
        raise ValueError("x_start must be [B, nVeh, 6] and u_tick [B, nVeh, K]")
    nz = None if noise is None else _dev(noise, device)
    out = torch.empty((B, V, K, 6), dtype=torch.float64, device=device)
    if drive is not None:
        from . import truth as TR
        dr, ac = _dev(drive, device), _dev(a_cmd, device)
        if tuple(dr.shape) != (B, V, LB.DRIVE_NP) or tuple(ac.shape) != (B, V):
            raise ValueError("drive must be [B, nVeh, 6] and a_cmd [B, nVeh]")
        tr = TR.nominal(params, B, device) if truth is None else _dev(truth, device)
        if tuple(tr.shape) != (B, V, LB.TRUTH_NP):
            raise ValueError("truth must be [B, nVeh, 5]")
        if nz is not None and tuple(nz.shape) != (B, V, 2):
            raise ValueError("noise must be [B, nVeh, 2]")
        ns = None if rng is None else rng.c_struct()
        LB.check(lib.scpqp_plant_step_drive(C.byref(params), B, K - 1, float(tick), _ptr(x),
                                            _ptr(u), _ptr(tr), _ptr(nz),
                                            None if ns is None else C.byref(ns), _ptr(ac),
                                            _ptr(dr), _ptr(out), float(h_max),
                                            _stream(device)), lib)
        return out
    if truth is not None:
        tr = _dev(truth, device)
        if tuple(tr.shape) != (B, V, LB.TRUTH_NP):
            raise ValueError("truth must be [B, nVeh, 5]")
        if nz is not None and tuple(nz.shape) != (B, V, 2):
            raise ValueError("noise must be [B, nVeh, 2]")
        ns = None if rng is None else rng.c_struct()
        LB.check(lib.scpqp_plant_step_truth(C.byref(params), B, K - 1, float(tick), _ptr(x),
                                            _ptr(u), _ptr(tr), _ptr(nz),
                                            None if ns is None else C.byref(ns), _ptr(out),
                                            float(h_max), _stream(device)), lib)
        return out
    if rng is not None:
        ns = rng.c_struct()
        LB.check(lib.scpqp_plant_step_noisy(C.byref(params), B, K - 1, float(tick), _ptr(x),
                                            _ptr(u), C.byref(ns), _ptr(out), float(h_max),
                                            _stream(device)), lib)
        return out
    LB.check(lib.scpqp_plant_step(C.byref(params), B, K - 1, float(tick), _ptr(x), _ptr(u),
                                  _ptr(nz), _ptr(out), float(h_max), _stream(device)), lib)
    return out


def noise_fill(rng, B, n_veh, site, k=0, n_eval=1, device=None):
    """The raw draws of ``rng``: [B, n_veh, n_eval, 2] = sigma * (z0, z1) of evaluations
    c0 = 0..n_eval-1 at (site, k) (scpqp_noise_fill)."""
    if not isinstance(rng, NoiseStream):
        raise TypeError("rng must be a NoiseStream")
    device = torch.device(device or "cuda")
    lib = LB.load()
    out = torch.empty((int(B), int(n_veh), int(n_eval), 2), dtype=torch.float64, device=device)
    ns = rng.c_struct()
    LB.check(lib.scpqp_noise_fill(C.byref(ns), int(B), int(n_veh), int(site), int(k), int(n_eval),
                                  _ptr(out), _stream(device)), lib)
    return out


def draw_ec_noise(rng, B, n_veh, device=None):
    """ec_noise [B, n_veh, 2] of ScpQpSolver.solve / linearize / evaluate: the draws of
    the one ode call inside comp_jacobian (Model.py:58) at ``rng.epoch``."""
    return noise_fill(rng, B, n_veh, LB.NOISE_SITE_LINEARIZE, 0, 1, device).view(int(B), int(n_veh), 2)


def clip_controls(u, u0, umax, n_veh, hp, du_lim):
    """In place on the solver's vehicle-major controls u [B, >= nVeh*hp]
    (main.py:164-174).  u0, umax: [B, nVeh] device tensors."""
    lib = LB.load()
    if u.dtype != torch.float64 or not u.is_contiguous() or u.dim() != 2:
        raise ValueError("u must be a contiguous float64 [B, ld] tensor")
    u0 = _dev(u0, u.device)
    um = _dev(umax, u.device)
    B, ld = int(u.shape[0]), int(u.shape[1])
    LB.check(lib.scpqp_clip_controls(B, int(n_veh), int(hp), ld, float(du_lim), _ptr(u), _ptr(u0),
                                     _ptr(um), _stream(u.device)), lib)
    return u
