"""The IPM's constraint-space row values and the memory plan they live in.

The step bodies of the interior point method and the polish reach a row's s, lam, rp, dd,
sa, la through an accessor (csrc/scpqp_kernel.h, Rows): kernels whose row-slot count
ceil(mc / 256) is a compile-time constant of at most 2 (the c2 / c4 shape and c5's horizon
classes) carry them in registers through a phase; every other kernel keeps the memory form.
The Newton direction has no storage of its own any more (seven vectors per plan, not nine),
and plan 1 at three workgroups per CU keeps tv in LDS, in the storage of the evaluated
positions pb (live only outside a QP solve).

* Compiled shapes: full SCP solves with the per-iteration trace, every iteration of every
  problem against the restatement's structured mode at the tolerances of tests/scp_parity.py.
  A solve of three or more SCP iterations runs a warm-started QP after cold ones, with an
  evaluation and a linearisation (pb) between two QP solves (tv) each time.
* Row-slot boundaries on the run-time-horizon kernels (mc = m + 2 N + 1): fewer rows than
  one wave, just under one full slot, a few rows in the second slot, and a second slot
  that is nearly half full.
* scpqp_evaluate and scpqp_linearize on the c2 shape (pb's other users).
* The c2 plan's resources.

The oracle solves run once, in one pool, for all of these.
"""
import multiprocessing as mp

import numpy as np
import pytest
import torch

from oracle import scp_reference as R
from scpqp import batch as BT
from scpqp.solver import ScpQpSolver, unpack_problem

import scp_parity as SP

pytestmark = pytest.mark.gpu

# name -> (vehicles, scenario horizon, batch, mixed horizons, base seed)
SOLVES = {
    "c2": (4, 20, 4, None, 4242),
    "c5_classes": (4, 30, 6, (10, 20, 30), 77),
    # run-time horizon: mc = 21, 253, 267, 361 rows
    "rows_21": (2, 4, 1, None, 5),
    "rows_253": (4, 18, 1, None, 6),
    "rows_267": (4, 19, 1, None, 7),
    "rows_361": (3, 40, 1, None, 8),
}


def _mc(nV, H):
    return nV * (nV - 1) // 2 * H + 2 * nV * H + 1


def _batch(name):
    nV, Hs, B, mixed, seed = SOLVES[name]
    sc = R.circle_scenario(nV, Hp=Hs)
    return sc, BT.make_batch(sc, B, base_seed=seed, mixed_hp=mixed)


@pytest.fixture(scope="module")
def oracle():
    """name -> the restatement's SCP results (with history) of that batch's problems."""
    jobs, keys = [], []
    for name, (nV, Hs, B, _, _) in SOLVES.items():
        _, bt = _batch(name)
        for b in range(B):
            jobs.append((nV, int(bt.hp[b]), bt.x0[b], bt.u0[b], bt.ec_noise[b], Hs))
            keys.append(name)
    with mp.get_context("spawn").Pool(min(16, len(jobs))) as pool:
        res = pool.map(SP.oracle_job, jobs)
    out = {name: [] for name in SOLVES}
    for k, r in zip(keys, res):
        out[k].append(r)
    return out


def _solve_and_compare(name, oracle):
    nV, Hs, B, mixed, _ = SOLVES[name]
    sc, bt = _batch(name)
    S = ScpQpSolver(sc, max_batch=B, hp_max=bt.hp_max)
    out = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=bt.hp if mixed else None, trace=True)
    torch.cuda.synchronize()
    n_scp = out.n_scp.cpu().numpy()
    for b in range(B):
        H, r = int(bt.hp[b]), oracle[name][b]
        tr = SP.device_trace(out, b, nV, 0, H, bt.hp_max)
        worst = 0.0
        for it in range(min(int(n_scp[b]), r.n_scp)):
            t, h = tr[it], r.history[it]
            e = float(np.max(np.abs(t["z"][:nV * H] - h["z"][:nV * H])))
            worst = max(worst, e)
            assert e <= SP.U_TOL, f"{name}[{b}] iteration {it}: |u| err {e:.2e}"
            assert abs(t["obj"] - h["obj"]) <= SP.OBJ_RTOL * max(1.0, abs(h["obj"])), (name, b, it)
        ub, tb = unpack_problem(out, b, nV, H)
        c = SP.compare(ub.cpu().numpy(), tb.cpu().numpy(), int(n_scp[b]), tr, r, nV, H,
                       what=f"{name}[{b}]")
        print(f"{name}[{b}] Hp {H} mc {_mc(nV, H)}: n_scp {int(n_scp[b])} (oracle {r.n_scp}), "
              f"per-iteration |u| err {worst:.2e}, stop flip {c['mismatch']}")
    # the evaluator on the returned u (pb after the last QP's tv) reproduces the outputs
    ev = S.evaluate(out.u, bt.x0, bt.u0, bt.ec_noise, hp=bt.hp if mixed else None)
    assert torch.max(torch.abs(ev["traj"] - out.traj)).item() <= 1e-12 * 30
    assert torch.allclose(ev["obj"], out.obj, rtol=1e-12, atol=0)
    S.close()
    return out, n_scp


@pytest.mark.parametrize("name", ["c2", "c5_classes"])
def test_compiled_shapes_full_solves(gpu, oracle, name):
    out, n_scp = _solve_and_compare(name, oracle)
    # QPs of one problem back to back, the third and later ones warm-started
    assert n_scp.max() >= 3
    if name == "c5_classes":
        _, bt = _batch(name)
        assert bt.hp.tolist() == [10, 20, 30, 10, 20, 30]
        assert [_mc(4, h) for h in (10, 20, 30)] == [141, 281, 421]


@pytest.mark.parametrize("name,mc", [("rows_21", 21), ("rows_253", 253), ("rows_267", 267),
                                     ("rows_361", 361)])
def test_row_slot_boundaries_runtime_horizon(gpu, oracle, name, mc):
    nV, Hs = SOLVES[name][:2]
    assert _mc(nV, Hs) == mc
    _solve_and_compare(name, oracle)


def test_evaluate_and_linearize_on_the_c2_shape(gpu):
    sc = R.circle_scenario(4, Hp=20)
    B, nV, H = 2, 4, 20
    bt = BT.make_batch(sc, B, base_seed=909)
    S = ScpQpSolver(sc, max_batch=B)
    U = np.random.default_rng(3).uniform(-sc.uLim, sc.uLim, (B, nV * H))
    # a solve first: the handle's LDS plan has held a QP's tv where pb goes
    S.solve(bt.x0, bt.u0, bt.ec_noise)
    ev = S.evaluate(U, bt.x0, bt.u0, bt.ec_noise)
    lin = S.linearize(bt.x0, bt.u0, bt.ec_noise)

    def rel(a, b):
        return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))

    for b in range(B):
        p = R.make_problem(sc, bt.x0[b], bt.u0[b], bt.ec_noise[b], Hp=H)
        Ls = R.linearise(p, "structured")
        r = R.evaluate_structured(p, Ls, U[b], obst_quirk=True)
        assert ev["obj"][b].item() == pytest.approx(r.obj, rel=1e-12)
        assert ev["max_violation"][b].item() == pytest.approx(r.max_violation, rel=1e-10, abs=1e-12)
        assert ev["sum_violations"][b].item() == pytest.approx(r.sum_violations, rel=1e-10, abs=1e-12)
        assert bool(ev["feasible"][b].item()) == r.feasible
        cv = ev["c_veh"][b].reshape(nV, nV, H).cpu().numpy()
        fin = np.isfinite(r.c_veh)
        assert np.array_equal(np.isfinite(cv), fin)
        assert np.max(np.abs(cv[fin] - r.c_veh[fin])) <= 1e-10
        tro, _ = R.forward_u(Ls, U[b], nV, H)
        assert np.max(np.abs(ev["traj"][b].reshape(H, 2, nV).cpu().numpy() - tro)) <= 1e-12 * 30
        Lf = R.linearise(p, "faithful")
        assert rel(lin["g"][b].reshape(nV, H, 2).cpu().numpy(), Lf.g) <= 1e-12
        assert rel(lin["const_term"][b].reshape(nV, 2 * H).cpu().numpy(), Lf.const) <= 1e-12
        assert rel(lin["psi0"][b].reshape(nV, H).cpu().numpy(), Lf.Psi0) <= 1e-10
        assert np.max(np.abs(lin["ref_points"][b].reshape(H, 2, nV).cpu().numpy() - p.ref_points)) <= 1e-12
    S.close()


def test_c2_plan_resources(gpu):
    sc = R.circle_scenario(4, Hp=20)
    S = ScpQpSolver(sc, max_batch=8)
    res = S.resources()
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    print("c2 resources:", res, "CUs", cus)
    assert res["grid"] == 3 * cus
    assert res["lds_bytes"] <= 53248
    assert res["ws_bytes_per_wg"] < 20304
    S.close()
