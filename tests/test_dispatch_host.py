"""The host plan and kernel dispatch, without a GPU: ``scpqp_plan_query`` (the function
``launch`` selects its kernel through) over every shape ``scpqp_create`` accepts.

* The set of instantiations some accepted shape runs equals the set the case table
  (tests/dispatch_cases.py) names, so a plan change that makes another kernel reachable
  fails here until a parity case is added for it.
* Every instantiation of SCPQP_KERNEL_LIST that no shape runs is in UNREACHABLE.
* The plan's arithmetic is consistent with the kernel it selects on every accepted shape.
* The case table's inputs exercise the solver (oracle alone, dispatch_cases docstring).
"""
import ctypes as C
import multiprocessing as mp
import os
import re

import pytest

from scpqp import _lib as LB
from scpqp.solver import plan_query

import dispatch_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 163840
LDS_GRANULE = 2048

# compiled, declared and dispatched, but no accepted shape runs them
UNREACHABLE = {
    (1, 1, 1, 2, 0), (1, 1, 1, 3, 0),                    # plan 2 at one row slot
    (0, 1, 3, 3, 0), (0, 1, 4, 2, 0), (0, 1, 4, 3, 0),   # plan 1 at three slots not lean, or four
    (0, 0, 3, 2, 0), (0, 0, 3, 3, 0), (0, 0, 4, 2, 0), (0, 0, 4, 3, 0),   # plan 0 beyond two slots
}


def kernel_list():
    """(HG, VG, RM, OCC, SH) of SCPQP_KERNEL_LIST in csrc/scpqp.hip, parsed the way
    test_abi.py::test_every_kernel_instantiation_in_exactly_one_group does."""
    csrc = os.path.join(ROOT, "senquential-convex-programming-for-trajectory-planning_amd", "csrc")
    host = open(os.path.join(csrc, "scpqp.hip")).read()
    body = host[host.index("#define SCPQP_RT_LIST"):host.index("#define SCPQP_EXTERN_LAUNCH")]
    listed = set()
    tf = {"true": 1, "false": 0}
    for hgv, vgv in re.findall(r"SCPQP_RT_LIST\(X, (true|false), (true|false)\)", body):
        for r, o in ((1, 2), (1, 3), (2, 2), (2, 3), (3, 2), (3, 3), (4, 2), (4, 3)):
            listed.add((tf[hgv], tf[vgv], r, o, 0))
    for hg, vg, r, o, s in re.findall(r"X\((\w+), (\w+), (\d), (\d), (\d)\)",
                                      body.split("#define SCPQP_KERNEL_LIST")[1]):
        listed.add((tf[hg], tf[vg], int(r), int(o), int(s)))
    return listed


@pytest.fixture(scope="module")
def accepted():
    """{(n_veh, n_obst, hp_max, has_hp): PlanInfo fields} of every shape the query accepts,
    and the refused ones' codes.  The struct call is made directly: ~38k calls."""
    lib = LB.load()
    ok, refused = {}, {}
    info = LB.PlanInfo()
    names = [n for n, _ in LB.PlanInfo._fields_]
    for V in range(0, LB.MAX_VEH + 2):
        for O in range(-1, LB.MAX_OBST + 2):
            for H in range(0, LB.MAX_HP + 2):
                D = LB.Dims(n_veh=V, hp_max=H, n_obst=O, max_batch=0)
                for has_hp in (0, 1):
                    rc = lib.scpqp_plan_query(C.byref(D), has_hp, C.byref(info))
                    if rc == 0:
                        ok[(V, O, H, has_hp)] = {n: getattr(info, n) for n in names}
                    else:
                        refused[(V, O, H, has_hp)] = (rc, lib.scpqp_last_error().decode())
    return ok, refused


def kernel_of(q):
    return (q["hg"], q["vg"], q["rm"], q["occ"], q["sh"])


def test_query_applies_creates_size_checks(accepted):
    """The same codes for the same reasons as scpqp_create (tests/test_abi.py): sizes out of
    range are SCPQP_E_ARG, n > 256 and a shape no LDS plan holds are SCPQP_E_SIZE; every
    in-range shape is either planned or refused with one of those two messages."""
    ok, refused = accepted
    lib = LB.load()
    info = LB.PlanInfo()
    assert lib.scpqp_plan_query(None, 0, C.byref(info)) == -1
    D = LB.Dims(n_veh=4, hp_max=20, n_obst=0, max_batch=0)
    assert lib.scpqp_plan_query(C.byref(D), 0, None) == -1
    D = LB.Dims(n_veh=4, hp_max=20, n_obst=0, max_batch=-1)
    assert lib.scpqp_plan_query(C.byref(D), 0, C.byref(info)) == -1
    n_plan = 0
    for (V, O, H, has_hp), (rc, msg) in refused.items():
        in_range = 1 <= V <= LB.MAX_VEH and 0 <= O <= LB.MAX_OBST and 1 <= H <= LB.MAX_HP
        if not in_range:
            assert rc == -1 and "out of range" in msg, (V, O, H, rc, msg)
        elif V * H + 1 > 256:
            assert rc == -4 and "> 256" in msg, (V, O, H, rc, msg)
        else:
            assert rc == -4 and "too large for the LDS plan" in msg, (V, O, H, rc, msg)
            n_plan += 1
    assert n_plan > 0          # e.g. 16 vehicles, 32 obstacles, Hp 15
    for (V, O, H, has_hp) in ok:
        assert 1 <= V <= LB.MAX_VEH and 0 <= O <= LB.MAX_OBST and 1 <= H <= LB.MAX_HP
        assert V * H + 1 <= 256
    # the wrapper raises where the constructor would
    with pytest.raises(RuntimeError, match="too large for the LDS plan"):
        plan_query(16, 32, 15)
    with pytest.raises(RuntimeError, match="> 256"):
        plan_query(8, 0, 64)


def test_reachable_instantiations_are_the_case_table(accepted):
    ok, _ = accepted
    reachable = {kernel_of(q) for q in ok.values()}
    table = [c.kernel for c in DC.CASES]
    assert len(table) == len(set(table)), "two rows for one instantiation"
    faulted = set(DC.REACHABLE_UNTESTED_FAULTED)
    assert not faulted & set(table)
    assert reachable == set(table) | faulted
    # every row without an earlier parity test is one the GPU file tests
    assert {c.kernel for c in DC.NEW_CASES} == {c.kernel for c in DC.CASES if c.covered_by is None}


def test_unreachable_instantiations_are_pinned(accepted):
    ok, _ = accepted
    reachable = {kernel_of(q) for q in ok.values()}
    listed = kernel_list()
    assert len(listed) == 29
    assert reachable <= listed, "the dispatch selects an instantiation that is not compiled"
    assert listed - reachable == UNREACHABLE


def test_unreachable_list_is_in_the_design_document():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in UNREACHABLE:
        assert "`(%d,%d,%d,%d,%d)`" % k in txt, k


def test_plan_is_consistent_with_the_kernel_on_every_accepted_shape(accepted):
    ok, _ = accepted
    assert len(ok) > 30000
    for (V, O, H, has_hp), q in ok.items():
        what = (V, O, H, has_hp, q)
        R = (V * H + 1 + 63) // 64
        assert q["row_slots"] == R and q["rm"] == R and R <= 4, what   # never the dispatch's default:
        assert 0 < q["lds_bytes"] <= LDS_LIMIT, what
        granules = (q["lds_bytes"] + LDS_GRANULE - 1) // LDS_GRANULE * LDS_GRANULE
        assert 1 <= q["per_cu"] <= 3 and q["per_cu"] * granules <= LDS_LIMIT, what
        assert q["occ"] in (2, 3) and (q["occ"] == 3) == (q["per_cu"] == 3), what
        assert q["plan"] in (0, 1, 2), what
        assert bool(q["lean"]) == (q["plan"] == 1 and q["occ"] == 2), what
        assert (q["hg"], q["vg"]) == ((0, 0), (0, 1), (1, 1))[q["plan"]], what
        assert (q["ws_doubles_per_wg"] > 0) == (q["plan"] > 0), what
        assert q["sh"] in (0, q["shape"]), what
        # a horizon array never changes the plan, only the compiled shape
        other = ok[(V, O, H, 1 - has_hp)]
        for k in ("plan", "lean", "per_cu", "lds_bytes", "ws_doubles_per_wg", "row_slots"):
            assert q[k] == other[k], what


@pytest.mark.parametrize("cid", [c.id for c in DC.CASES])
def test_case_runs_the_instantiation_it_names(cid):
    c = DC.by_id(cid)
    sc = DC.scenario(c.scenario, c.n_veh, c.hp_max)
    assert sc.nVeh == c.n_veh
    q = plan_query(sc.nVeh, sc.nObst, c.hp_max, c.has_hp)
    assert q["kernel"] == c.kernel
    if c.mixed is not None:
        n_veh, hp_max, hps, _ = c.mixed
        scm = DC.scenario(c.scenario, n_veh, hp_max)
        assert plan_query(scm.nVeh, scm.nObst, hp_max, True)["kernel"] == c.kernel
        assert max(hps) == hp_max and len(set(hps)) == 3 and min(hps) >= 1


def test_mixed_horizon_cases_cover_the_kinds():
    """A workspace-factor kernel, a lean kernel, and 8 vehicles at Hp 30 with a horizon array
    (which runs a run-time kernel, not the compiled c3 one)."""
    ks = [c for c in DC.MIXED_CASES]
    assert len(ks) >= 3
    assert any(c.kernel[0] == 1 and c.mixed[:2] != (8, 30) for c in ks)
    assert any(plan_query(DC.scenario(c.scenario, *c.mixed[:2]).nVeh,
                          DC.scenario(c.scenario, *c.mixed[:2]).nObst, c.mixed[1], True)["lean"]
               for c in ks)
    assert any(c.scenario == "circle" and c.mixed[:2] == (8, 30) for c in ks)
    assert plan_query(8, 0, 30, False)["kernel"] == (1, 1, 4, 2, 3)
    assert plan_query(8, 0, 30, True)["kernel"] == (1, 1, 4, 2, 0)


def test_some_case_runs_at_one_workgroup_per_cu_and_some_with_three_row_slots():
    per_cu = {c.id: plan_query(DC.scenario(c.scenario, c.n_veh, c.hp_max).nVeh,
                               DC.scenario(c.scenario, c.n_veh, c.hp_max).nObst, c.hp_max,
                               c.has_hp)["per_cu"] for c in DC.NEW_CASES}
    assert 1 in per_cu.values() and 2 in per_cu.values() and 3 in per_cu.values()
    assert any(c.kernel[2] == 3 for c in DC.NEW_CASES)


@pytest.fixture(scope="module")
def oracle_runs():
    """The 8 problems of every new case on the oracle, in one spawn pool."""
    jobs, owner = [], []
    for c in DC.NEW_CASES:
        sc, bt = DC.case_inputs(c)
        js = DC.oracle_jobs(c.scenario, c.n_veh, sc, bt)
        jobs += js
        owner += [c.id] * len(js)
    with mp.get_context("spawn").Pool(8) as pool:
        res = pool.map(DC.oracle_job, jobs, chunksize=1)
    out = {}
    for cid, r in zip(owner, res):
        out.setdefault(cid, []).append(r)
    return out


@pytest.mark.parametrize("cid", [c.id for c in DC.NEW_CASES])
def test_case_inputs_exercise_the_solver(oracle_runs, cid):
    """The input conditions of the case table, on the oracle alone.  (Every QP
    certified: the oracle raised otherwise, and oracle_job asserts the history's flags.)"""
    runs = oracle_runs[cid]
    assert len(runs) == DC.N_PROBLEMS
    print(cid, "n_scp", [r.n_scp for r, _, _, _ in runs], "active rows",
          [a for _, _, a, _ in runs], "one-QP mode spread %.1e" % max(s for _, _, _, s in runs))
    for b, (r, _, active, spread) in enumerate(runs):
        assert r.converged and r.n_scp < 20, (cid, b, r.n_scp)
        assert r.n_scp >= 3, (cid, b, r.n_scp)
        assert active >= 1, (cid, b)
        assert spread <= DC.ONE_QP_MODE_SPREAD, (cid, b, spread)
