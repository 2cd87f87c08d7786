"""The triangular solves' sweeps with the step index a compile-time constant (Solver of
scpqp_kernel.h): every solution entry is written into its owner lane by a
``v_writelane`` whose lane is an immediate computed from the step index, one step late, and
the last entry of every row slot by a flush.  A wrong lane, a missed flush or a wrong first
step corrupts the solution of every IPM iteration, so parity with the oracle through the
public ABI sees it.  The four compile-time sizes where that lane arithmetic differs:

  n =  41   one row slot                                             c5 class Hp 10
  n =  81   two slots, 17 rows in the second (``j & 63`` wraps)      c2, and c5 class Hp 20
  n = 121   two slots, 57 rows in the second                         c5 class Hp 30
  n = 241   four slots, factor in the workspace, chunks of 8,        c3
            the last chunk partial (one row)

and one run-time shape, whose sweeps keep the select form and stay rolled.

Per size: 3 distinct problems in one launch, and the first of them alone (B = 1, bitwise the
same as in the launch of 3).  One QP and the full SCP solve against the oracle at the
tolerances of tests/test_gpu_dispatch.py (one QP |u| <= 1e-8 rad; full solve |u| <= 1e-7 rad,
|traj| <= 1e-6 m), with equal SCP counts on both sides.  The oracle runs once per row.
"""
import multiprocessing as mp

import numpy as np
import pytest
import torch

from scpqp.solver import ScpQpSolver, plan_query, unpack_problem

import dispatch_cases as DC
import scp_parity as SP
from test_gpu_parity import QP_TOL

pytestmark = pytest.mark.gpu

B = 3
# id: (kernel, scenario, vehicles, hp_max, horizons of the 3 problems or None, sizes n run)
ROWS = {
    "c2_n81": ((0, 1, 2, 3, 1), "circle", 4, 20, None, (81,)),
    "c5_n41_n81_n121": ((0, 1, 2, 2, 2), "circle", 4, 30, (10, 20, 30), (41, 81, 121)),
    "c3_n241": ((1, 1, 4, 2, 3), "circle", 8, 30, None, (241,)),
    "runtime_n65": ((0, 0, 2, 3, 0), "circle", 1, 64, None, (65,)),
}


def inputs(rid):
    """The row's first B problems of dispatch_cases' batch (seed 303, stock start)."""
    _, kind, n_veh, hp_max, hps, _ = ROWS[rid]
    sc, bt = DC.make_inputs(kind, n_veh, hp_max, 1.0, hps)
    return sc, bt


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(B) as p:
        yield p


_cache = {}


def oracle(pool, rid):
    if rid not in _cache:
        _, kind, n_veh, _, _, _ = ROWS[rid]
        sc, bt = inputs(rid)
        _cache[rid] = pool.map(DC.oracle_job, DC.oracle_jobs(kind, n_veh, sc, bt)[:B], chunksize=1)
    return _cache[rid]


def hp_arg(rid, bt, dev, sel):
    if ROWS[rid][4] is None:
        return None
    return torch.as_tensor(bt.hp[sel], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("rid", list(ROWS))
def test_sweeps_against_the_oracle(gpu, pool, rid):
    kernel, kind, n_veh, hp_max, hps, sizes = ROWS[rid]
    sc, bt = inputs(rid)
    assert plan_query(sc.nVeh, sc.nObst, hp_max, hps is not None)["kernel"] == kernel
    assert tuple(sc.nVeh * int(h) + 1 for h in sorted(set(bt.hp[:B].tolist()))) == sizes
    orc = oracle(pool, rid)
    S = ScpQpSolver(sc, max_batch=B, hp_max=hp_max)
    three = slice(0, B)
    one = slice(0, 1)
    # one QP
    qp = S.solve(bt.x0[three], bt.u0[three], bt.ec_noise[three], hp=hp_arg(rid, bt, gpu, three),
                 max_scp_iter=1)
    torch.cuda.synchronize()
    e_qp = []
    for b, (_, u_one, _, _) in enumerate(orc):
        u, _ = unpack_problem(qp, b, sc.nVeh, int(bt.hp[b]))
        e_qp.append(float(np.max(np.abs(u.cpu().numpy() - u_one))))
    # the full solve, B = 3 and B = 1
    out = S.solve(bt.x0[three], bt.u0[three], bt.ec_noise[three], hp=hp_arg(rid, bt, gpu, three),
                  trace=True)
    torch.cuda.synchronize()
    u3, traj3, scp3 = out.u.clone(), out.traj.clone(), out.n_scp.clone()
    alone = S.solve(bt.x0[one], bt.u0[one], bt.ec_noise[one], hp=hp_arg(rid, bt, gpu, one))
    torch.cuda.synchronize()
    n_dev = scp3.tolist()
    n_orc = [r.n_scp for r, _, _, _ in orc]
    e_u, e_t = [], []
    for b, (r, _, _, _) in enumerate(orc):
        H = int(bt.hp[b])
        ub, tb = unpack_problem(out, b, sc.nVeh, H)
        e_u.append(float(np.max(np.abs(ub.cpu().numpy() - r.u))))
        e_t.append(float(np.max(np.abs(tb.cpu().numpy() - r.traj))))
    print(f"solve_sweeps {rid}: one QP |u| {max(e_qp):.2e} rad; full solve |u| {max(e_u):.2e} rad "
          f"|traj| {max(e_t):.2e} m; n_scp device {n_dev} oracle {n_orc}")
    assert max(e_qp) <= QP_TOL, (rid, e_qp)
    assert n_dev == n_orc, (rid, n_dev, n_orc)
    assert max(e_u) <= SP.U_TOL, (rid, e_u)
    assert max(e_t) <= SP.TRAJ_TOL, (rid, e_t)
    assert torch.equal(alone.n_scp, scp3[:1])
    assert torch.equal(alone.u[0], u3[0])
    assert torch.equal(alone.traj[0], traj3[0])
    S.close()
