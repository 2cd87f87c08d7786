"""A dsafeExtra sweep as one mixed launch against one launch per value
(include/scpqp_variants.h).

K values of dsafeExtra, linearly spaced over [0.5, 1.5], times R problems each of the
4-vehicle circle at Hp 20 (make_batch, base_seed 0; problem b uses value b // R):
  mixed     one handle with the K variants, one launch of K * R problems
  separate  K handles, one launch of R problems each, back to back on one stream
Both forms solve the same problems; the outputs are compared exactly.  Each form is timed
with hipEvents around the whole form, after a warm-up, `reps` times.

    python tools/variant_sweep.py [K=16] [R=64] [reps=5]

Prints one JSON line.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "senquential-convex-programming-for-trajectory-planning_amd")]

import numpy as np  # noqa: E402


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    Rn = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import torch
    from oracle import scp_reference as R
    from scpqp import batch as BT
    from scpqp.solver import ScpQpSolver
    values = np.linspace(0.5, 1.5, K)
    scs = []
    for v in values:
        sc = R.circle_scenario(4, Hp=20)
        sc.dsafeExtra = float(v)
        scs.append(sc)
    B = K * Rn
    bt = BT.make_batch(scs[0], B, base_seed=0)
    dev = torch.device("cuda", 0)
    x0, u0, ec = (torch.as_tensor(a, device=dev) for a in (bt.x0, bt.u0, bt.ec_noise))
    var = torch.as_tensor(np.arange(B) // Rn, dtype=torch.int32, device=dev)
    mixed = ScpQpSolver(scs[0], max_batch=B, variants=scs)
    out_m = mixed.alloc_out(B)
    parts = [ScpQpSolver(sc, max_batch=Rn) for sc in scs]
    outs = [p.alloc_out(Rn) for p in parts]
    sl = [slice(k * Rn, (k + 1) * Rn) for k in range(K)]
    ins = [(x0[s].contiguous(), u0[s].contiguous(), ec[s].contiguous()) for s in sl]

    def run_mixed():
        mixed.solve(x0, u0, ec, variant=var, out=out_m)

    def run_separate():
        for p, o, (a, b, c) in zip(parts, outs, ins):
            p.solve(a, b, c, out=o)

    def timed(fn):
        fn()                                   # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    # alternate the two forms so that a drift of the clocks hits both
    t_m, t_s = [], []
    for _ in range(2):
        t_m += timed(run_mixed)
        t_s += timed(run_separate)
    same = all(torch.equal(getattr(out_m, f)[s], getattr(o, f))
               for s, o in zip(sl, outs)
               for f in ("u", "traj", "status", "n_scp", "n_ipm", "obj", "max_violation"))
    n_scp = out_m.n_scp.view(K, Rn).float().mean(1).cpu().tolist()
    res = mixed.resources()
    print(json.dumps({
        "sweep": f"{K} dsafeExtra values x {Rn} problems, 4-vehicle circle, Hp 20",
        "mixed_ms": t_m, "separate_ms": t_s,
        "mixed_ms_median": float(np.median(t_m)), "separate_ms_median": float(np.median(t_s)),
        "speedup": float(np.median(t_s) / np.median(t_m)),
        "bitwise_equal": bool(same), "grid": res["grid"],
        "mean_n_scp_per_value": [round(x, 2) for x in n_scp],
        "status_converged_frac": float(((out_m.status & 0xff) == 0).float().mean().item())}))
    for p in parts + [mixed]:
        p.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
