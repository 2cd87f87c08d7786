"""Time per call of the obstacle margin step next to the IMM tracker step that feeds it
(include/scpqp_margin.h), on the frog scenario's obstacles with braking manoeuvres.

    python tools/margin_time.py [B] [n_modes] [calls]

Prints one JSON line: HIP-event milliseconds per call, the median over ``calls`` calls each, of
``imm.step`` and of ``margin.step`` (with and without ``sigma_out``) on the state after eight
tracker steps.  Default B = 1024, 4 modes (straight, arc, brake and a second brake mode with a
larger q_accel), hp = 10, 22 obstacles.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "senquential-convex-programming-for-trajectory-planning_amd")]

import numpy as np  # noqa: E402


def main():
    import torch
    from oracle import scp_reference as R
    from scpqp import imm as IMM
    from scpqp import manoeuvres as MAN
    from scpqp import margin as MG
    from scpqp.obstacles import ObstacleDist
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    sc = R.frog_scenario(Hp=10)
    nO, hp, dt = sc.nObst, sc.Hp, float(sc.dt)
    lead = sc.delay_x + sc.dt + sc.delay_u
    rows = ObstacleDist(sc, 0).uniform("yaw_rate", 0.3).sample(B, device="cuda")
    man = MAN.rows(B, nO, MAN.brake(np.full((B, nO), 1.0), 3.0, 20.0), device="cuda")
    osense = torch.zeros((B, nO, 3), dtype=torch.float64, device="cuda")
    osense[..., 0], osense[..., 1] = 0.05, 0.01
    names = ("straight", "arc", "brake", "brake")[:M]
    trk, sw = IMM.bank(osense, modes=names)
    if M == 4:
        trk[:, :, 3, 7] *= 3.0           # the second brake mode: a larger q_accel
    st = IMM.alloc(B, nO, M, "cuda")

    def imm_step(s):
        snap = MAN.state(rows, man, s * dt)
        return IMM.step(snap, osense, 1, s, 0, trk, sw, 0.0, 0.0 if s == 0 else dt, lead, dt, hp, *st)

    for s in range(8):
        imm_step(s)
    snap = MAN.state(rows, man, 8 * dt)
    kappa = MG.kappa_for(0.05)

    def timed(fn):
        ms = []
        for _ in range(calls + 5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms[5:]))

    saved = [t.clone() for t in st]

    def imm_call():
        for t, s0 in zip(st, saved):
            t.copy_(s0)
        IMM.step(snap, osense, 1, 8, 0, trk, sw, 0.0, dt, lead, dt, hp, *st)

    def copy_only():
        for t, s0 in zip(st, saved):
            t.copy_(s0)

    out = dict(B=B, n_obst=nO, hp=hp, n_modes=M, calls=calls,
               state_copy_ms=timed(copy_only), imm_step_ms_with_state_copy=timed(imm_call))
    for t, s0 in zip(st, saved):
        t.copy_(s0)
    mg = torch.empty((B, nO, hp), dtype=torch.float64, device="cuda")
    out["margin_step_ms"] = timed(lambda: MG.step(trk, *st, lead, dt, hp, kappa, 2.0, out=mg))
    out["margin_step_sigma_ms"] = timed(lambda: MG.step(trk, *st, lead, dt, hp, kappa, 2.0, sigma=True))
    out["mean_margin"] = float(mg.nanmean().item())
    out["nan_lanes"] = int(torch.isnan(mg[..., 0]).sum().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
