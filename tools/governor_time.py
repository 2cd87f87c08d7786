"""Time per call of the speed governor step (include/scpqp_governor.h) at the shape of
profiles/margin_rollout.txt: the frog scenario's one vehicle and 22 obstacles, hp = 10.

    python tools/governor_time.py [B] [calls] [look]

Prints one JSON line: HIP-event milliseconds per call of ``governor.step``, the median over
``calls`` calls, with and without the diagnostic outputs, on a plan along the lane and the
scenario's own obstacle prediction with margins of 1 m.  Default B = 1024, LOOK = 10 (the
whole horizon: the most pairs a lane of this shape can examine).
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
    from scpqp import governor as GOV
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    look = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    sc = R.frog_scenario(Hp=10)
    nV, nO, hp, dt = sc.nVeh, sc.nObst, sc.Hp, float(sc.dt)
    f = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0)
    x0 = torch.as_tensor(np.array(sc.x0, float)[None] + rng.normal(0, 0.05, (B, nV, 6)), **f)
    traj = torch.zeros((B, hp, 2, nV), **f)
    traj[:, :, 0, :] = x0[:, None, :, 0] + 4.0 * dt * torch.arange(1, hp + 1, **f)[None, :, None]
    traj[:, :, 1, :] = x0[:, None, :, 1]
    fut = R.obstacle_future(sc, np.asarray(sc.obstacles, float), hp)
    obst = torch.as_tensor(fut, **f)[None].expand(B, -1, -1, -1).contiguous()
    margin = torch.ones((B, nO, hp), **f)
    rows = GOV.rows(B, nV, v_ref=4.0, a_acc=1.0, a_brake=3.0, k_v=0.5, look=look, device="cuda")
    dreq = GOV.required(sc, device="cuda")
    dreq = tuple(t.expand(B, -1, -1).contiguous() for t in dreq)

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

    call = lambda diag: GOV.step(rows, x0, traj, obst, margin, *dreq, dt, float(sc.delay_u),
                                 diag=diag)
    out = dict(B=B, n_veh=nV, n_obst=nO, hp=hp, look=look, calls=calls,
               governor_step_ms=timed(lambda: call(True)),
               governor_step_no_diag_ms=timed(lambda: call(False)))
    a, k, c = call(True)
    out["frac_conflict"] = float((k >= 0).float().mean().item())
    out["bad_lanes"] = int((k == -2).sum().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
