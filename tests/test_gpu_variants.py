"""Scenario variants on the GPU (include/scpqp_variants.h): one launch whose problems use
different scenario-level parameters.

The main check is bitwise: problems are solved independently of each other, so a mixed
launch must give each problem exactly what a handle created from its own scenario gives
it (the project relies on the same invariance in test_gpu_distributed.py and
test_split_invariance).  Oracle parity per variant then shows that the block a problem
reads is really its variant's: at tests/scp_parity.py's tolerances, no problem skipped.

Three variants of a scenario are used throughout:
  v0  the scenario as built
  v1  dsafeExtra 0.5, R 2000
  v2  dsafeExtra 1.5, Q 2, Q_final 10, every polyline's end point rotated by 0.05 rad
      about the origin
with dsafeVehicles / dsafeObstacles recomputed.  Problems come from
make_batch(base_seed=0); the shapes are the smallest that reach each way the kernel is
compiled (rows in registers, compiled horizon classes with the work-order permutation,
the factor in the workspace, obstacle rows, five vehicles with obstacles).
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

import metrics_mirror as MM
import scp_parity as SP
import test_gpu_metrics as TGM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import batch as BT
from scpqp.solver import ScpQpSolver, unpack_problem

pytestmark = pytest.mark.gpu

X0_SIGMA = np.array([0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def three_variants(build):
    v0, v1, v2 = build(), build(), build()
    nV = v0.nVeh
    v1.dsafeExtra = 0.5
    v1.R = [2000.0] * nV
    v2.dsafeExtra = 1.5
    v2.Q = [2.0] * nV
    v2.Q_final = [10.0] * nV
    c, s = math.cos(0.05), math.sin(0.05)
    for t in v2.referenceTrajectories:
        x, y = t[-1]
        t[-1] = (c * x - s * y, s * x + c * y)
    for v in (v0, v1, v2):
        v.dsafeVehicles, v.dsafeObstacles = R.safety_distances(v)
    return [v0, v1, v2]


# name -> (scenario builder, B, make_batch keywords, variant of problem b, variants used)
CASES = {
    "c2": (lambda: R.circle_scenario(4, Hp=20), 12, dict(), lambda b: b % 3, 3),
    "c5_mixed": (lambda: R.circle_scenario(4, Hp=30), 12, dict(mixed_hp=(10, 20, 30)),
                 lambda b: (b // 3) % 3, 3),
    "c3": (lambda: R.circle_scenario(8, Hp=30), 4, dict(), lambda b: b % 2, 2),
    "frog": (lambda: R.frog_scenario(Hp=10), 6, dict(), lambda b: b % 3, 3),
    "parallel5": (lambda: R.parallel_scenario(5, Hp=10), 6, dict(), lambda b: b % 3, 3),
}
_cache = {}


def case(name):
    """The case's variants, batch, variant indices and its mixed launch (with the trace),
    computed once and shared by the tests; nothing mutates them."""
    if name not in _cache:
        build, B, kw, var_of, n_var = CASES[name]
        scs = three_variants(build)[:n_var]
        bt = BT.make_batch(scs[0], B, base_seed=0, **kw)
        var = np.array([var_of(b) for b in range(B)], np.int32)
        assert sorted(set(var.tolist())) == list(range(n_var))
        mixed = "mixed_hp" in kw
        S = ScpQpSolver(scs[0], max_batch=B, hp_max=bt.hp_max, variants=scs)
        out = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=bt.hp if mixed else None,
                      obst=bt.obst if scs[0].nObst else None, trace=True, variant=var)
        torch.cuda.synchronize()
        _cache[name] = dict(scs=scs, bt=bt, var=var, mixed=mixed, S=S, out=out)
    return _cache[name]


def call_kw(c, idx=None):
    """The per-problem inputs of the case (all, or the problems ``idx``) as keywords."""
    bt, sl = c["bt"], slice(None) if idx is None else idx
    kw = dict(u0=bt.u0[sl], ec_noise=bt.ec_noise[sl])
    if c["mixed"]:
        kw["hp"] = bt.hp[sl]
    if c["scs"][0].nObst:
        kw["obst"] = bt.obst[sl]
    return kw


def bits(t):
    """Exact comparison key: the bit pattern (the trace holds NaN where nothing is written)."""
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(bits(got), bits(want)), what


def per_variant(c, run):
    """run(solver of variant k alone, the indices of its problems) for every variant."""
    for k, sc in enumerate(c["scs"]):
        idx = np.nonzero(c["var"] == k)[0]
        Sk = ScpQpSolver(sc, max_batch=len(idx), hp_max=c["bt"].hp_max)
        run(Sk, idx, k)
        Sk.close()


# ------------------------------------------------------------------ 1. mixed == separate
@pytest.mark.parametrize("name", sorted(CASES))
def test_mixed_launch_equals_separate_handles(gpu, name):
    c = case(name)
    fields = [f.name for f in dataclasses.fields(c["out"])]
    assert "trace" in fields and len(fields) == 13

    def run(Sk, idx, k):
        ref = Sk.solve(c["bt"].x0[idx], trace=True, **call_kw(c, idx))
        torch.cuda.synchronize()
        for f in fields:
            assert_same(getattr(c["out"], f)[idx], getattr(ref, f), f"{name} variant {k}: {f}")

    per_variant(c, run)
    # the variants do differ: with entry 0 for all, every problem of another variant changes
    base = c["S"].solve(c["bt"].x0, **call_kw(c))
    torch.cuda.synchronize()
    differs = (base.u != c["out"].u).any(dim=1).cpu().numpy()
    assert np.array_equal(differs, c["var"] != 0), name
    assert (c["out"].n_scp > 0).all()


@pytest.mark.parametrize("name", ["c2", "frog"])
def test_other_entry_points_equal_separate_handles(gpu, name):
    c = case(name)
    bt, var, S = c["bt"], c["var"], c["S"]
    nV = c["scs"][0].nVeh
    U = np.random.default_rng(5).uniform(-c["scs"][0].uLim, c["scs"][0].uLim, (bt.size, nV * bt.hp_max))
    ev = S.evaluate(U, bt.x0, variant=var, **call_kw(c))
    lin = S.linearize(bt.x0, variant=var, **call_kw(c))
    ref = S.sample_reference(bt.x0, hp=bt.hp if c["mixed"] else None, variant=var)

    def run(Sk, idx, k):
        kw = call_kw(c, idx)
        e = Sk.evaluate(U[idx], bt.x0[idx], **kw)
        for f in ev:
            assert_same(ev[f][idx], e[f], f"{name} variant {k}: evaluate {f}")
        li = Sk.linearize(bt.x0[idx], **kw)
        for f in lin:
            assert_same(lin[f][idx], li[f], f"{name} variant {k}: linearize {f}")
        r = Sk.sample_reference(bt.x0[idx], hp=kw.get("hp"))
        assert_same(ref[idx], r, f"{name} variant {k}: sample_reference")

    per_variant(c, run)
    # v1's R, v2's Q and polylines: one problem and one u under the three variants
    i0, i1, i2 = (int(np.nonzero(var == k)[0][0]) for k in range(3))
    same_u = S.evaluate(np.repeat(U[:1], bt.size, 0), np.repeat(bt.x0[:1], bt.size, 0), variant=var,
                        **{k: np.repeat(np.asarray(v)[:1], bt.size, 0) for k, v in call_kw(c).items()})
    objs = [same_u["obj"][i].item() for i in (i0, i1, i2)]
    assert len(set(objs)) == 3


# ------------------------------------------------------------------ 2. oracle parity
@pytest.mark.parametrize("name", ["c2", "frog"])
def test_oracle_parity_per_variant(gpu, name):
    c = case(name)
    bt, out = c["bt"], c["out"]
    for b in range(bt.size):
        sc = c["scs"][int(c["var"][b])]
        nV, nO, H = sc.nVeh, sc.nObst, int(bt.hp[b])
        ob = bt.obst[b].reshape(-1)[:nO * 2 * H].reshape(nO, 2, H)
        p = R.make_problem(sc, bt.x0[b], bt.u0[b], bt.ec_noise[b], Hp=H, obst=ob)
        r = R.scp_solve(p, mode="structured", keep_history=True)
        u, tr = unpack_problem(out, b, nV, H)
        got = SP.compare(u.cpu().numpy(), tr.cpu().numpy(), int(out.n_scp[b].item()),
                         SP.device_trace(out, b, nV, nO, H, bt.hp_max), r, nV, H,
                         what=f"{name}[{b}] variant {int(c['var'][b])}")
        print(f"{name}[{b}] variant {int(c['var'][b])}: n_scp {int(out.n_scp[b].item())} / "
              f"{r.n_scp}, {got}")


# ------------------------------------------------------------------ 3. defaults
def test_defaults(gpu):
    c = case("c2")
    bt, S = c["bt"], c["S"]
    fields = [f.name for f in dataclasses.fields(c["out"])]
    # a table is installed: variant=None is entry 0, i.e. a plain v0 handle
    got = S.solve(bt.x0, bt.u0, bt.ec_noise, trace=True)
    plain = ScpQpSolver(c["scs"][0], max_batch=bt.size)
    want = plain.solve(bt.x0, bt.u0, bt.ec_noise, trace=True)
    # a handle that never saw set_variants: variant=zeros is variant=None
    zeros = plain.solve(bt.x0, bt.u0, bt.ec_noise, trace=True, variant=np.zeros(bt.size, np.int32))
    torch.cuda.synchronize()
    for f in fields:
        assert_same(getattr(got, f), getattr(want, f), f"variant=None after set_variants: {f}")
        assert_same(getattr(zeros, f), getattr(want, f), f"variant=zeros without a table: {f}")
    with pytest.raises(ValueError):
        plain.solve(bt.x0, bt.u0, bt.ec_noise, variant=np.zeros(bt.size - 1, np.int32))
    plain.close()


# ------------------------------------------------------------------ 4. out of range
def test_out_of_range_index(gpu):
    c = case("c2")
    bt, S = c["bt"].slice(0, 6), c["S"]
    var = c["var"][:6].copy()
    good = S.solve(bt.x0, bt.u0, bt.ec_noise, variant=var, trace=True)
    var[2], var[4] = 3, -1
    sentinel = S.alloc_out(6, trace=True)
    for f in dataclasses.fields(sentinel):
        t = getattr(sentinel, f.name)
        if f.name != "trace":      # the trace keeps its NaN fill: unwritten iterations stay NaN
            t.fill_(-7.0 if t.dtype == torch.float64 else -7)
    want_untouched = {f.name: getattr(sentinel, f.name).clone() for f in dataclasses.fields(sentinel)}
    bad = S.solve(bt.x0, bt.u0, bt.ec_noise, variant=var, out=sentinel)
    torch.cuda.synchronize()
    ok = [0, 1, 3, 5]
    for b in (2, 4):
        assert bad.status[b].item() == LB.ST_INVALID
        for f in ("n_scp", "n_ipm", "n_polish", "n_refine", "n_warm"):
            assert getattr(bad, f)[b].item() == 0, f
        for f in ("u", "traj", "obj", "max_violation", "sum_violations", "feasible", "trace"):
            assert_same(getattr(bad, f)[b], want_untouched[f][b], f"nothing else is written: {f}")
    for f in dataclasses.fields(good):
        assert_same(getattr(bad, f.name)[ok], getattr(good, f.name)[ok], f.name)
    assert ((good.status & 0xff) == LB.ST_CONVERGED).all()
    # a table of three: set_variants rejects what may not differ, naming the field
    other = R.circle_scenario(4, Hp=20)
    other.dt = 0.5
    with pytest.raises(RuntimeError, match="dt"):
        S.set_variants([c["scs"][0], other])
    assert S.n_variants == 3


# ------------------------------------------------------------------ 5. metrics
def test_metrics_variants(gpu):
    from scpqp.metrics import PathMetrics
    rng = np.random.default_rng(31)
    lines = [[(-9, 0), (9, 0)], [(0, -5), (3, 0), (5, 5)], [(-4, -4), (0, -3), (2, 0), (4, 4)],
             [(-9, 2), (9, 2)]]
    obst = [(1.0, -1.0, 0.4, 2.0, 4.0, 2.0), (-2.0, 2.0, math.pi / 2, 0.0, 2.0, 2.0)]
    scs = [TGM.scenario([0.98, 2.0, 1.0, 0.98], [0.88, 0.5, 1.0, 0.88], obst, lines, dsafe=2.0),
           TGM.scenario([1.5, 2.0, 1.0, 0.98], [0.88, 0.5, 1.0, 0.88],
                        [(2.0, -1.0, 0.4, 2.0, 4.0, 2.0), (-2.0, 1.0, 0.3, 1.0, 2.0, 2.0)],
                        lines[::-1], dsafe=1.0),
           TGM.scenario([0.98, 2.0, 2.5, 0.98], [0.88, 0.5, 1.0, 0.88],
                        [(1.0, -3.0, 1.4, 0.5, 3.0, 2.0), (-1.0, 2.0, 0.0, 0.0, 2.0, 1.0)],
                        [[(-9, 1), (9, 1)]] * 4, dsafe=3.0)]
    B, K = 6, 11
    var = np.array([0, 1, 2, 2, 0, 1], np.int32)
    steps = [TGM.random_path(rng, B, 4, K, 3.0) for _ in range(2)]
    calls = [(x, 10 * i, 0 if i == 0 else 1) for i, x in enumerate(steps)]
    for k, sc in enumerate(scs):
        for x, tick0, _ in calls:
            assert TGM.smallest_margin(MM.Constants.of_scenario(sc), x[var == k], tick0) > 1e-6

    def run(pm, sl, variant):
        pm.reset(len(sl))
        dense = []
        for x, tick0, kf in calls:
            dense.append(pm.accumulate(torch.as_tensor(x[sl], device=gpu), tick0, kf, dense=True,
                                       variant=variant))
        return pm.result(), dense

    pm = PathMetrics(scs[0], B, gpu, variants=scs)
    res, dense = run(pm, np.arange(B), var)
    torch.cuda.synchronize()
    for k, sc in enumerate(scs):
        idx = np.nonzero(var == k)[0]
        one = PathMetrics(sc, len(idx), gpu)
        rk, dk = run(one, idx, None)
        for f in TGM.INT_FIELDS + TGM.DBL_FIELDS:
            assert_same(res[f][idx], rk[f], f"variant {k}: {f}")
        for d, d1 in zip(dense, dk):
            for f in d:
                assert_same(d[f][idx], d1[f], f"variant {k}: dense {f}")
        one.close()
        # the mirror with the realisations' own constants
        want = MM.run(MM.Constants.of_scenario(sc), [(x[idx], t0, kf) for x, t0, kf in calls],
                      len(idx))
        TGM.check_result({f: v[idx] for f, v in res.items()}, want, f"variants[{k}]")
    # out of range: the realisation's accumulator stays at its reset values
    bad = var.copy()
    bad[1], bad[3] = 3, -1
    pm.reset(B)
    pm.accumulate(torch.as_tensor(steps[0], device=gpu), 0, 0, variant=bad)
    out = pm.result()
    for b in (1, 3):
        assert math.isinf(out["min_gap_veh"][b].item()) and math.isinf(out["min_margin_obs"][b].item())
        assert out["n_ticks_seen"][b].item() == 0 and out["first_collision_tick"][b].item() == -1
        assert out["argmin_gap_veh"][b].tolist() == [-1, -1, -1]
        assert (out["sum_sq_xtrack"][b] == 0).all()
    assert out["n_ticks_seen"][[0, 2, 4, 5]].tolist() == [K] * 4
    with pytest.raises(ValueError):
        pm.accumulate(torch.as_tensor(steps[0], device=gpu), 0, 0, variant=bad[:5])
    other = TGM.scenario([0.98] * 4, [0.88] * 4, obst, lines, tick_length=0.02)
    with pytest.raises(RuntimeError, match="tick_length"):
        pm.set_variants([scs[0], other])
    pm.close()


# ------------------------------------------------------------------ 6. rollout
def rollout_case(gpu, scs, x_init, steps):
    """B = 4 with variant_of = [0, 0, 1, 1] against two rollouts of B = 2 with b_offset 0
    and 2: bitwise equal states, control paths, U, n_scp and every metrics field."""
    from scpqp.rollout import ClosedLoopBatch
    variant_of = [0, 0, 1, 1]
    both = ClosedLoopBatch(scs[0], 4, device=gpu, keep_path=True, metrics=True, variants=scs,
                           variant_of=variant_of)
    both.reset(x_init, seed=1)
    both.run(steps)
    parts = []
    for k, sc in enumerate(scs):
        cl = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
        cl.reset(x_init[2 * k:2 * k + 2], seed=1, b_offset=2 * k)
        cl.run(steps)
        parts.append(cl)
    torch.cuda.synchronize()
    cat = lambda get: torch.cat([get(p) for p in parts])   # noqa: E731
    assert_same(both.state, cat(lambda p: p.state), "state")
    assert_same(both.control, cat(lambda p: p.control), "control path")
    for i in range(steps):
        for f in ("U", "n_scp", "status", "path", "traj", "x0", "ref"):
            assert_same(both.history[i][f], cat(lambda p: p.history[i][f]), f"step {i}: {f}")
        ev = both.history[i]["evaluation"]
        for f in ev:
            assert_same(ev[f], cat(lambda p: p.history[i]["evaluation"][f]), f"step {i}: evaluation {f}")
    res = both.metrics()
    for f in res:
        assert_same(res[f], cat(lambda p: p.metrics()[f]), f"metrics {f}")
    assert res["n_ticks_seen"].tolist() == [steps * int(scs[0].ticks_per_sim) + 1] * 4
    from scpqp.metrics import summarize, summarize_by_variant
    by = summarize_by_variant(res, variant_of)
    assert by == {k: summarize(p.metrics()) for k, p in enumerate(parts)}
    out = both, parts
    return out


def test_rollout_with_variants_circle(gpu):
    scs = three_variants(lambda: R.circle_scenario(4, Hp=10))[:2]
    rng = np.random.default_rng(23)
    x_init = np.array(scs[0].x0)[None] + rng.normal(0, 1, (4, 4, 6)) * X0_SIGMA
    both, parts = rollout_case(gpu, scs, x_init, 3)
    # the two variants plan differently from the same kind of start
    assert not torch.equal(parts[0].history[0]["U"], parts[1].history[0]["U"])
    for cl in [both] + parts:
        cl.close()


def test_rollout_with_variants_frog_two_obstacle_sets(gpu):
    a, b = R.frog_scenario(Hp=10), R.frog_scenario(Hp=10)
    for ob in b.obstacles:
        ob[0] += 1.0
    b.dsafeVehicles, b.dsafeObstacles = R.safety_distances(b)
    rng = np.random.default_rng(29)
    x_init = np.array(a.x0)[None] + rng.normal(0, 1, (4, 1, 6)) * X0_SIGMA
    both, parts = rollout_case(gpu, [a, b], x_init, 2)
    obst = both._obstacle_prediction(0)
    assert torch.equal(obst[0], obst[1]) and torch.equal(obst[2], obst[3])
    assert torch.equal(obst[2, :, 0], obst[0, :, 0] + 1.0) and torch.equal(obst[2, :, 1], obst[0, :, 1])
    for cl in [both] + parts:
        cl.close()


# ------------------------------------------------------------------ 7. rejections
def test_rollout_rejects_variants_that_differ_in_shared_attributes(gpu):
    from scpqp.rollout import ClosedLoopBatch
    base = R.circle_scenario(4, Hp=10)
    lf = R.circle_scenario(4, Hp=10)
    lf.Lf = [0.4] * 4
    with pytest.raises(ValueError, match="Lf"):
        ClosedLoopBatch(base, 2, device=gpu, variants=[base, lf], variant_of=[0, 1])
    hp = R.circle_scenario(4, Hp=12)
    with pytest.raises(ValueError, match="Hp"):
        ClosedLoopBatch(base, 2, device=gpu, variants=[base, hp], variant_of=[0, 1])
    with pytest.raises(ValueError, match="variant_of"):
        ClosedLoopBatch(base, 2, device=gpu, variants=[base, base])
    with pytest.raises(ValueError, match="variant_of"):
        ClosedLoopBatch(base, 2, device=gpu, variants=[base, base], variant_of=[0, 2])
