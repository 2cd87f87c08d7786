"""Oracle parity of every solve-kernel instantiation the host plan can reach.

The case table (tests/dispatch_cases.py) has one row per reachable instantiation
``(HG, VG, RM, OCC, SH)``; tests/test_dispatch_host.py proves on the CPU that the table is
exactly the reachable set.  The rows that earlier parity tests run get the two cheap checks
here (kernel identity, workgroup reuse); every other row also gets the linearisation, one
QP, the full SCP solve per iteration, and, on some, a mixed-horizon launch.

Tolerances are the project's stated ones (tests/test_gpu_parity.py, tests/scp_parity.py):
stage intermediates 1e-12 relative, one QP |u| <= 1e-8 rad, end to end |u| <= 1e-7 rad and
|traj| <= 1e-6 m with a stop flip explained per iteration.  Inputs: 8 problems per row whose
oracle solves are certified, uncapped, at least 3 SCP iterations long, end with an active
collision row and have an unambiguous first QP (dispatch_cases docstring).  Each test prints a ``dispatch_parity``
line with its worst errors (profiles/dispatch_parity.txt is one run's output).
"""
import multiprocessing as mp

import numpy as np
import pytest
import torch

from oracle import scp_reference as R
from scpqp.solver import ScpQpSolver, plan_query, unpack_problem

import dispatch_cases as DC
import scp_parity as SP
from test_gpu_configs import _properties
from test_gpu_parity import QP_TOL, rel

pytestmark = pytest.mark.gpu

ALL_IDS = [c.id for c in DC.CASES]
NEW_IDS = [c.id for c in DC.NEW_CASES]
MIXED_IDS = [c.id for c in DC.MIXED_CASES]


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(8) as p:
        yield p


_oracle_cache = {}


def oracle(pool, key, kind, n_veh, sc, bt):
    """The oracle's results of a row's problems: computed once, shared by its tests."""
    if key not in _oracle_cache:
        _oracle_cache[key] = pool.map(DC.oracle_job, DC.oracle_jobs(kind, n_veh, sc, bt), chunksize=1)
    return _oracle_cache[key]


def hp_arg(case, bt, dev):
    """The horizon array of a row whose kernel is the one a call WITH the array runs: a
    device tensor (the solver drops a host array that is all hp_max)."""
    if not case.has_hp:
        return None
    return torch.as_tensor(bt.hp, dtype=torch.int32, device=dev)


def obst_arg(sc, bt):
    return bt.obst if sc.nObst else None


def solver_for(sc, bt, max_batch):
    return ScpQpSolver(sc, max_batch=max_batch, hp_max=bt.hp_max)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_kernel_identity(gpu, cid):
    """(a) The query names the row's instantiation, and the handle agrees with the query."""
    c = DC.by_id(cid)
    sc, bt = DC.case_inputs(c)
    q = plan_query(sc.nVeh, sc.nObst, c.hp_max, c.has_hp)
    assert q["kernel"] == c.kernel
    S = solver_for(sc, bt, DC.N_PROBLEMS)
    res = S.resources()
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert res["plan"] == q["plan"]
    assert res["lds_bytes"] == q["lds_bytes"]
    assert res["ws_bytes_per_wg"] == 8 * q["ws_doubles_per_wg"]
    assert res["grid"] == q["per_cu"] * cus
    S.close()


@pytest.mark.parametrize("cid", ALL_IDS)
def test_workgroup_reuse(gpu, cid):
    """(e) One launch of 2 grid + 8 problems, the row's 8 problems tiled in a shuffled order:
    every workgroup takes further problems with the previous one's LDS and workspace
    contents in place, behind varying predecessors.  Every copy equals, bitwise, the same
    problem of the 8-problem launch."""
    c = DC.by_id(cid)
    sc, bt = DC.case_inputs(c)
    n = DC.N_PROBLEMS
    q = plan_query(sc.nVeh, sc.nObst, c.hp_max, c.has_hp)
    grid = q["per_cu"] * torch.cuda.get_device_properties(gpu).multi_processor_count
    B = 2 * grid + n
    idx = np.random.default_rng(0).permutation(np.arange(B) % n)
    S = solver_for(sc, bt, B)
    assert S.resources()["grid"] == grid
    small = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp_arg(c, bt, gpu), obst=obst_arg(sc, bt))
    torch.cuda.synchronize()
    u8, scp8, ipm8 = small.u.clone(), small.n_scp.clone(), small.n_ipm.clone()
    hp = None if not c.has_hp else torch.as_tensor(bt.hp[idx], dtype=torch.int32, device=gpu)
    big = S.solve(bt.x0[idx], bt.u0[idx], bt.ec_noise[idx], hp=hp,
                  obst=bt.obst[idx] if sc.nObst else None)
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu)
    assert int(scp8.min()) >= 1
    assert torch.equal(big.n_scp, scp8[sel])
    assert torch.equal(big.n_ipm, ipm8[sel])
    assert torch.equal(big.u, u8[sel])
    print(f"dispatch_parity {cid} reuse: B {B} on grid {grid}, bitwise equal; "
          f"n_scp {scp8.tolist()}")
    S.close()


@pytest.mark.parametrize("cid", NEW_IDS)
def test_linearisation(gpu, cid):
    """(b) Stage intermediates at test_linearize_parity's tolerances."""
    c = DC.by_id(cid)
    sc, bt = DC.case_inputs(c)
    S = solver_for(sc, bt, DC.N_PROBLEMS)
    lin = S.linearize(bt.x0, bt.u0, bt.ec_noise, hp=hp_arg(c, bt, gpu), obst=obst_arg(sc, bt))
    nV = sc.nVeh
    worst = 0.0
    for b in range(DC.N_PROBLEMS):
        H = int(bt.hp[b])
        p = R.make_problem(sc, bt.x0[b], bt.u0[b], bt.ec_noise[b], Hp=H,
                           obst=DC.problem_obst(sc, bt, b))
        L = R.linearise(p, "faithful")
        g = lin["g"][b].reshape(-1)[:nV * H * 2].reshape(nV, H, 2).cpu().numpy()
        ct = lin["const_term"][b].reshape(-1)[:nV * H * 2].reshape(nV, 2 * H).cpu().numpy()
        ps = lin["psi0"][b].reshape(-1)[:nV * H].reshape(nV, H).cpu().numpy()
        rp = lin["ref_points"][b].reshape(-1)[:H * 2 * nV].reshape(H, 2, nV).cpu().numpy()
        errs = (rel(lin["Ad"][b].cpu().numpy(), L.Ad), rel(lin["Bd"][b].cpu().numpy(), L.Bd),
                float(np.max(np.abs(lin["Ed"][b].cpu().numpy() - L.Ed))), rel(g, L.g),
                rel(ct, L.const), float(np.max(np.abs(rp - p.ref_points))))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-12, (cid, b, errs)
        assert rel(ps, L.Psi0) <= 1e-10, (cid, b)
    print(f"dispatch_parity {cid} linearisation: worst relative error {worst:.2e}")
    S.close()


@pytest.mark.parametrize("cid", NEW_IDS)
def test_one_qp(gpu, pool, cid):
    """(c) One QP from the same linearisation point against the oracle's one-QP solve."""
    c = DC.by_id(cid)
    sc, bt = DC.case_inputs(c)
    orc = oracle(pool, cid, c.scenario, c.n_veh, sc, bt)
    S = solver_for(sc, bt, DC.N_PROBLEMS)
    out = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp_arg(c, bt, gpu), obst=obst_arg(sc, bt),
                  max_scp_iter=1)
    torch.cuda.synchronize()
    errs = []
    for b, (_, u_one, _, _) in enumerate(orc):
        u, _ = unpack_problem(out, b, sc.nVeh, int(bt.hp[b]))
        errs.append(float(np.max(np.abs(u.cpu().numpy() - u_one))))
    print(f"dispatch_parity {cid} one QP: worst |u| error {max(errs):.2e} rad")
    assert max(errs) <= QP_TOL, (cid, errs)
    S.close()


def _full_solve(gpu, pool, key, kind, n_veh, sc, bt, hp, what):
    """(d) The full SCP solve with its trace against the oracle's history (SP.compare: final
    u / traj on equal SCP counts, else per iteration with the stop flip explained; no
    problem skipped), and the evaluator-consistency properties on the returned u."""
    orc = oracle(pool, key, kind, n_veh, sc, bt)
    nV, nO = sc.nVeh, sc.nObst
    S = solver_for(sc, bt, DC.N_PROBLEMS)
    out = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=obst_arg(sc, bt), trace=True)
    torch.cuda.synchronize()
    if nO == 0:
        _properties(S, sc, bt, out, nV, bt.hp_max, hp=hp)
    else:
        ev = S.evaluate(out.u, bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst)
        assert torch.max(torch.abs(ev["traj"] - out.traj)).item() <= 1e-12 * 30
        assert torch.allclose(ev["obj"], out.obj, rtol=1e-12, atol=0)
        assert torch.equal(ev["feasible"], out.feasible)
    eu = et = 0.0
    flips = 0
    for b, (r, _, _, _) in enumerate(orc):
        H = int(bt.hp[b])
        ub, tb = unpack_problem(out, b, nV, H)
        cmp_ = SP.compare(ub.cpu().numpy(), tb.cpu().numpy(), int(out.n_scp[b].item()),
                          SP.device_trace(out, b, nV, nO, H, bt.hp_max), r, nV, H,
                          what=f"{what}[{b}] (Hp {H})")
        eu = max(eu, cmp_["u_err"])
        et = max(et, cmp_.get("traj_err", 0.0))
        flips += cmp_["mismatch"]
    print(f"dispatch_parity {what} full solve: worst |u| error {eu:.2e} rad, |traj| error "
          f"{et:.2e} m, {flips} stop flips explained; n_scp device {out.n_scp.tolist()} "
          f"oracle {[r.n_scp for r, _, _, _ in orc]}, active rows {[a for _, _, a, _ in orc]}")
    S.close()
    return out


@pytest.mark.parametrize("cid", NEW_IDS)
def test_full_solve(gpu, pool, cid):
    c = DC.by_id(cid)
    sc, bt = DC.case_inputs(c)
    _full_solve(gpu, pool, cid, c.scenario, c.n_veh, sc, bt, hp_arg(c, bt, gpu), cid)


@pytest.mark.parametrize("cid", MIXED_IDS)
def test_mixed_horizons(gpu, pool, cid):
    """(f) The row's kernel with a horizon array of hp_max, a middle and a small value: the
    order_kernel path and the kernel's run-time Hb < hp_max path.  Every problem against
    the oracle at its own horizon; outputs past a problem's horizon stay zero."""
    c = DC.by_id(cid)
    n_veh, hp_max, hps, _ = c.mixed
    sc, bt = DC.mixed_inputs(c)
    assert plan_query(sc.nVeh, sc.nObst, hp_max, True)["kernel"] == c.kernel
    assert sorted(set(bt.hp.tolist())) == sorted(hps)
    hp = torch.as_tensor(bt.hp, dtype=torch.int32, device=gpu)
    out = _full_solve(gpu, pool, cid + "/mixed", c.scenario, n_veh, sc, bt, hp,
                      f"{cid} mixed {n_veh}x{hp_max} Hp {hps}")
    u = out.u.cpu().numpy().reshape(DC.N_PROBLEMS, -1)
    traj = out.traj.cpu().numpy().reshape(DC.N_PROBLEMS, -1)
    for b in range(DC.N_PROBLEMS):
        H = int(bt.hp[b])
        assert np.all(u[b, sc.nVeh * H:] == 0.0), (cid, b)
        assert np.all(traj[b, H * 2 * sc.nVeh:] == 0.0), (cid, b)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_cold_ipm_iteration_count(gpu, pool, cid):
    """The IPM around the factorisation converges with an inexact Newton direction, so a
    factor or a substitution that has lost digits shows up as more iterations, not as a wrong
    u.  The device's cold iteration count of the first QP (trace slot 5 of SCP iteration 0, no
    u_warm) against the oracle's qp_ipm(init="omega") on the same scaled QP, every problem of
    the row: device <= oracle + DC.IPM_COUNT_MARGIN."""
    c = DC.by_id(cid)
    sc, bt = DC.case_inputs(c)
    orc = pool.map(DC.ipm_count_job, DC.oracle_jobs(c.scenario, c.n_veh, sc, bt), chunksize=1)
    S = solver_for(sc, bt, DC.N_PROBLEMS)
    out = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp_arg(c, bt, gpu), obst=obst_arg(sc, bt),
                  max_scp_iter=1, trace=True)
    torch.cuda.synchronize()
    dev = [SP.device_trace(out, b, sc.nVeh, sc.nObst, int(bt.hp[b]), bt.hp_max)[0]["ipm_iters"]
           for b in range(DC.N_PROBLEMS)]
    S.close()
    diff = [d - o for d, (o, _) in zip(dev, orc)]
    print(f"ipm_count {cid}: device {dev} oracle {[o for o, _ in orc]} (status "
          f"{[s for _, s in orc]}) device - oracle max {max(diff)} min {min(diff)}")
    assert all(d >= 1 for d in dev), (cid, dev)
    assert max(diff) <= DC.IPM_COUNT_MARGIN, (cid, diff)
