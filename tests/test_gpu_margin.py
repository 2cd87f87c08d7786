"""Obstacle margins on the GPU (include/scpqp_margin.h).

Solver input: every case of tests/margin_cases.py on its solve kernel against the margin-aware
oracle mirror (tests/margin_solver_mirror.py) at the tolerances of tests/test_gpu_dispatch.py
(end to end |u| <= 1e-7 rad, |traj| <= 1e-6 m, per iteration with a stop flip explained; c_obs
1e-12 relative); NULL against an all-zero array bitwise; bad entries; entries past a prefix; a
constant margin against a variant with larger safety distances, bitwise (the distances and the
margin are multiples of 2^-20 there, so every sum is exact in either order).

Margin step: the device against the mirror (tests/margin_mirror.py) at the tolerance derived on
the CPU (margin_cases.TOL), off and trouble lanes, split batches, kappa = 0, the cap, mu = NULL.

Rollout: the frog rollout with braking obstacles of tests/test_gpu_imm.py with margin=.
"""
import multiprocessing as mp
import types

import numpy as np
import pytest
import torch

import imm_mirror as IM
import margin_cases as MC
import margin_mirror as MM
import scp_parity as SP
import tracker_accel_cases as TC
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import imm as IMM
from scpqp import manoeuvres as MAN
from scpqp import margin as MG
from scpqp import tracker as TRK
from scpqp import tracker_accel as TRKA
from scpqp.solver import ScpQpSolver, plan_query, unpack_problem
from test_margin_host import CONST_MARGIN, exact_scenario, trouble_lanes

pytestmark = pytest.mark.gpu

ST_INVALID = 2
LEAD, DT = MC.lead_dt()
KAPPA = MM.kappa_for(MC.P_MISS)


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64),
                                                   b.contiguous().view(torch.int64)))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(8) as p:
        yield p


_mirror_cache = {}


def mirror(pool, cid):
    """The mirror's results of a case's problems: computed once, shared by its tests."""
    if cid not in _mirror_cache:
        _mirror_cache[cid] = pool.map(MC.mirror_job, MC.mirror_jobs(cid), chunksize=1)
    return _mirror_cache[cid]


def hp_arg(c, bt, gpu):
    return None if c.hps is None else torch.as_tensor(bt.hp, dtype=torch.int32, device=gpu)


SOLVE_FIELDS = ("u", "traj", "obj", "max_violation", "sum_violations")
COUNT_FIELDS = ("status", "n_scp", "n_ipm", "feasible", "n_polish", "n_refine", "n_warm")


def same_result(a, b, sel=slice(None)):
    return all(_beq(getattr(a, k)[sel], getattr(b, k)[sel]) for k in SOLVE_FIELDS) and all(
        bool(torch.equal(getattr(a, k)[sel], getattr(b, k)[sel])) for k in COUNT_FIELDS)


# ---------------------------------------------------------------------------
# 1. the solver input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", MC.IDS)
def test_solve_and_evaluate_match_the_mirror(gpu, pool, cid):
    c = MC.by_id(cid)
    sc, bt, mg = MC.inputs(c)
    nV, nO = sc.nVeh, sc.nObst
    assert plan_query(nV, nO, c.hp_max, c.hps is not None)["kernel"] == c.kernel
    ref = mirror(pool, cid)
    S = ScpQpSolver(sc, max_batch=MC.N_PROBLEMS, hp_max=bt.hp_max)
    hp = hp_arg(c, bt, gpu)
    out = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, trace=True, obst_margin=mg)
    torch.cuda.synchronize()
    eu = et = 0.0
    flips = 0
    for b, r in enumerate(ref):
        H = int(bt.hp[b])
        ub, tb = unpack_problem(out, b, nV, H)
        cmp_ = SP.compare(_np(ub), _np(tb), int(out.n_scp[b].item()),
                          SP.device_trace(out, b, nV, nO, H, bt.hp_max), r, nV, H,
                          what=f"{cid}[{b}] (Hp {H})")
        eu, et = max(eu, cmp_["u_err"]), max(et, cmp_.get("traj_err", 0.0))
        flips += cmp_["mismatch"]
    print(f"margin_parity {cid}: worst |u| error {eu:.2e} rad, |traj| error {et:.2e} m, {flips} "
          f"stop flips explained; n_scp device {out.n_scp.tolist()} mirror {[r.n_scp for r in ref]}")
    # the evaluation of the mirror's u: c_obs, violations, feasibility
    u_ref = np.zeros((MC.N_PROBLEMS, nV * bt.hp_max))
    for b, r in enumerate(ref):
        u_ref[b, :r.u.size] = r.u
    ev = S.evaluate(u_ref, bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, obst_margin=mg)
    worst = 0.0
    for b, r in enumerate(ref):
        H = int(bt.hp[b])
        co = _np(ev["c_obs"][b]).reshape(-1)[:nV * nO * H].reshape(nV, nO, H)
        assert np.array_equal(np.isinf(co), np.isinf(r.c_obs)), (cid, b)
        ok = np.isfinite(r.c_obs)
        if ok.any():     # (one vehicle: the obstacle quirk evaluates no obstacle row, all -inf)
            worst = max(worst, float(np.max(np.abs(co - r.c_obs)[ok])
                                     / max(1.0, np.max(np.abs(r.c_obs[ok])))))
        else:
            assert nV == 1
        assert abs(ev["max_violation"][b].item() - r.max_violation) <= 1e-9 * max(1.0, r.max_violation)
        assert bool(ev["feasible"][b].item()) == r.feasible, (cid, b)
    print(f"margin_parity {cid}: c_obs worst relative error {worst:.2e}")
    assert worst <= 1e-12
    S.close()


@pytest.mark.parametrize("cid", ["frog1x20", "parallel5x10"])
def test_null_and_zero_array_are_bitwise_equal(gpu, cid):
    c = MC.by_id(cid)
    sc, bt, mg = MC.inputs(c)
    S = ScpQpSolver(sc, max_batch=MC.N_PROBLEMS, hp_max=bt.hp_max)
    a = S.solve(bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, trace=True)
    b = S.solve(bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, trace=True, obst_margin=np.zeros_like(mg),
                out=S.alloc_out(MC.N_PROBLEMS, trace=True))
    w = S.solve(bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, obst_margin=mg,
                out=S.alloc_out(MC.N_PROBLEMS))
    torch.cuda.synchronize()
    assert same_result(a, b) and _beq(a.trace, b.trace)
    assert not _beq(a.u, w.u)                              # and the margin is not ignored
    ea = S.evaluate(a.u, bt.x0, bt.u0, bt.ec_noise, obst=bt.obst)
    eb = S.evaluate(a.u, bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, obst_margin=np.zeros_like(mg))
    for k in ea:
        assert _beq(ea[k], eb[k]) if ea[k].dtype == torch.float64 else torch.equal(ea[k], eb[k]), k
    S.close()


def test_bad_entries_invalidate_their_problem_alone(gpu):
    c = MC.by_id("frog1x29_mixed")
    sc, bt, mg = MC.inputs(c)
    nO, Hm = sc.nObst, bt.hp_max
    S = ScpQpSolver(sc, max_batch=MC.N_PROBLEMS, hp_max=Hm)
    hp = hp_arg(c, bt, gpu)
    good = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, obst_margin=mg)
    # an entry past a short problem's prefix: never read (problem 2 runs at Hp 5)
    assert int(bt.hp[2]) == 5
    past = mg.copy()
    past.reshape(MC.N_PROBLEMS, -1)[2, nO * 5:] = np.nan
    res = S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, obst_margin=past,
                  out=S.alloc_out(MC.N_PROBLEMS))
    torch.cuda.synchronize()
    assert same_result(good, res)
    # a NaN, a negative and an inf entry inside the prefixes of problems 1, 4 and 6
    bad = mg.copy()
    flat = bad.reshape(MC.N_PROBLEMS, -1)
    flat[1, nO * int(bt.hp[1]) - 1] = np.nan
    flat[4, 0] = -1e-300
    flat[6, 7] = np.inf
    hit = [1, 4, 6]
    out = S.alloc_out(MC.N_PROBLEMS)
    for k in SOLVE_FIELDS + COUNT_FIELDS:
        getattr(out, k)[hit] = -7                          # a mark nothing of the solve writes
    S.solve(bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, obst_margin=bad, out=out)
    torch.cuda.synchronize()
    rest = [b for b in range(MC.N_PROBLEMS) if b not in hit]
    assert out.status[hit].tolist() == [ST_INVALID] * 3
    for k in ("n_scp", "n_ipm", "n_polish", "n_refine", "n_warm"):
        assert getattr(out, k)[hit].tolist() == [0] * 3, k
    for k in SOLVE_FIELDS:
        assert (getattr(out, k)[hit] == -7.0).all(), k
    assert (out.feasible[hit] == -7).all()
    assert same_result(good, out, rest)
    # the evaluate writes nothing of such a problem either
    ev = S.evaluate(good.u, bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, obst_margin=mg)
    eb = S.evaluate(good.u, bt.x0, bt.u0, bt.ec_noise, hp=hp, obst=bt.obst, obst_margin=bad)
    for k in ev:
        assert _beq(ev[k][rest].double(), eb[k][rest].double()), k
        assert (eb[k][hit] == 0).all(), k                  # as allocated
    S.close()


@pytest.mark.parametrize("cid", ["frog1x20", "parallel5x10"])
def test_constant_margin_is_a_variant_with_larger_distances_bitwise(gpu, cid):
    c = MC.by_id(cid)
    sc, bt, _ = MC.inputs(c)
    m = CONST_MARGIN(sc.nObst)
    base, wide = exact_scenario(sc), exact_scenario(sc, m)
    S = ScpQpSolver(base, max_batch=MC.N_PROBLEMS, hp_max=bt.hp_max, variants=[base, wide])
    const = np.broadcast_to(m[None, :, None], (MC.N_PROBLEMS, sc.nObst, bt.hp_max)).copy()
    zero = np.zeros(MC.N_PROBLEMS, dtype=np.int32)
    a = S.solve(bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, variant=zero, obst_margin=const)
    b = S.solve(bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, variant=zero + 1,
                out=S.alloc_out(MC.N_PROBLEMS))
    plain = S.solve(bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, variant=zero,
                    out=S.alloc_out(MC.N_PROBLEMS))
    torch.cuda.synchronize()
    assert same_result(a, b)
    if c.frog:
        assert not _beq(a.u, plain.u)
    # the margin adds to the problem's own variant: on top of the wide one it is 2 m
    ea = S.evaluate(a.u, bt.x0, bt.u0, bt.ec_noise, obst=bt.obst, variant=zero + 1, obst_margin=const)
    twice = ScpQpSolver(exact_scenario(sc, 2 * m), max_batch=MC.N_PROBLEMS, hp_max=bt.hp_max)
    eb = twice.evaluate(a.u, bt.x0, bt.u0, bt.ec_noise, obst=bt.obst)
    assert _beq(ea["c_obs"], eb["c_obs"]) and _beq(ea["max_violation"], eb["max_violation"])
    twice.close()
    S.close()


# ---------------------------------------------------------------------------
# 2. the margin step
# ---------------------------------------------------------------------------
def device_step(gpu, trk, x, cov, mu, hp, kappa=KAPPA, m_max=MC.M_MAX):
    args = [_dev(a, gpu) for a in (trk, x, cov)]
    return MG.step(*args, None if mu is None else _dev(mu, gpu), LEAD, DT, hp, kappa, m_max,
                   sigma=True)


_mirror_step = {}


def mirror_step(B, nO, hp, M):
    if (B, nO, hp, M) not in _mirror_step:
        _mirror_step[(B, nO, hp, M)] = MM.step(*MC.states(B, nO, hp, M), LEAD, DT, hp, KAPPA, MC.M_MAX)
    return _mirror_step[(B, nO, hp, M)]


@pytest.mark.parametrize("M", MC.MODES)
@pytest.mark.parametrize("B,nO,hp", MC.SHAPES)
def test_margin_step_matches_the_mirror(gpu, B, nO, hp, M):
    trk, x, cov, mu = MC.states(B, nO, hp, M)
    m_d, s_d = device_step(gpu, trk, x, cov, mu, hp)
    m_m, s_m = mirror_step(B, nO, hp, M)
    worst = MC.ratio((_np(m_d), _np(s_d)), (m_m, s_m))
    print(f"M = {M} ({B}, {nO}, {hp}): largest device - mirror ratio {worst:.3e} (TOL {MC.TOL:.3e})")
    assert worst <= MC.TOL
    off = ~(trk != 0).any(axis=(2, 3))
    assert (_np(m_d)[off] == 0).all() and (_np(s_d)[off] == 0).all()
    assert off.sum() == ((m_m == 0).all(-1)).sum()
    # without sigma_out the margins are the same
    only = MG.step(*(_dev(a, gpu) for a in (trk, x, cov, mu)), LEAD, DT, hp, KAPPA, MC.M_MAX)
    assert _beq(only, m_d)


def test_off_lanes_do_not_look_at_their_state(gpu):
    trk, x, cov, mu = (a.copy() for a in MC.states(2, 3, 5, 3))
    base = device_step(gpu, trk, x, cov, mu, 5)
    trk[1, 1] = 0.0
    x[1, 1], cov[1, 1], mu[1, 1] = np.nan, np.inf, -1.0
    m, s = device_step(gpu, trk, x, cov, mu, 5)
    assert (m[1, 1] == 0).all() and (s[1, 1] == 0).all()
    keep = torch.ones(2, 3, dtype=torch.bool, device=gpu)
    keep[1, 1] = False
    assert _beq(m[keep], base[0][keep]) and _beq(s[keep], base[1][keep])


def test_every_kind_of_trouble_is_nan_in_its_own_lane_only(gpu):
    trk, x, cov, mu = (a.copy() for a in MC.states(2, 3, 5, 2))
    base = device_step(gpu, trk, x, cov, mu, 5)
    b, o = 0, 1
    assert torch.isfinite(base[0]).all()
    kinds = trouble_lanes(trk[b, o], x[b, o], cov[b, o], mu[b, o])
    assert len(kinds) == 9
    keep = torch.ones(2, 3, dtype=torch.bool, device=gpu)
    keep[b, o] = False
    for kind, (t, xx, pp, mm) in kinds.items():
        T, X, P, U = trk.copy(), x.copy(), cov.copy(), mu.copy()
        T[b, o], X[b, o], P[b, o], U[b, o] = t, xx, pp, mm
        m, s = device_step(gpu, T, X, P, U, 5)
        assert torch.isnan(m[b, o]).all() and torch.isnan(s[b, o]).all(), kind
        assert _beq(m[keep], base[0][keep]) and _beq(s[keep], base[1][keep]), kind
    # only the upper triangle of P is read
    P = cov.copy()
    P[b, o, 0][np.tril_indices(6, -1)] = np.nan
    m, s = device_step(gpu, trk, x, P, mu, 5)
    assert _beq(m, base[0]) and _beq(s, base[1])


@pytest.mark.parametrize("M", [1, 4])
def test_a_split_batch_gives_what_the_whole_gives(gpu, M):
    B, nO, hp = 12, 22, 10
    trk, x, cov, mu = MC.states(B, nO, hp, M)
    whole = device_step(gpu, trk, x, cov, mu, hp)
    for cut in (5, 11):
        parts = [device_step(gpu, trk[s], x[s], cov[s], mu[s], hp)
                 for s in (slice(0, cut), slice(cut, B))]
        for i in range(2):
            assert _beq(whole[i], torch.cat([p[i] for p in parts])), (cut, i)


def test_kappa_zero_the_cap_and_mu_null(gpu):
    B, nO, hp = 2, 3, 5
    trk, x, cov, mu = MC.states(B, nO, hp, 2)
    free = device_step(gpu, trk, x, cov, mu, hp)
    m0, s0 = device_step(gpu, trk, x, cov, mu, hp, kappa=0.0)
    assert (m0 == 0).all() and _beq(s0, free[1])
    cap = float(free[0][free[0] > 0].median())
    mc, _ = device_step(gpu, trk, x, cov, mu, hp, m_max=cap)
    assert _beq(mc, torch.clamp(free[0], max=cap)) and (mc == cap).any() and (mc < cap).any()
    mz, _ = device_step(gpu, trk, x, cov, mu, hp, m_max=0.0)
    assert (mz == 0).all()
    # M = 1: mu = NULL is mu = 1, with the arrays of the single filter as they are
    trk1, x1, cov1, mu1 = MC.states(B, nO, hp, 1)
    a = device_step(gpu, trk1, x1, cov1, np.where(np.isnan(mu1), mu1, 1.0), hp)
    on = ~np.isnan(mu1[..., 0])
    b = device_step(gpu, trk1[:, :, 0], x1[:, :, 0], cov1[:, :, 0], None, hp)
    sel = torch.as_tensor(on, device=gpu)
    assert _beq(a[0][sel], b[0][sel]) and _beq(a[1][sel], b[1][sel]) and sel.any()
    with pytest.raises(ValueError):
        MG.step(*(_dev(v, gpu) for v in (trk, x, cov)), None, LEAD, DT, hp, KAPPA, 1.0)
    with pytest.raises(ValueError):
        MG.step(*(_dev(v, gpu) for v in (trk, x, cov, mu)), LEAD, DT, hp, -1.0, 1.0)


# ---------------------------------------------------------------------------
# 3. rollout: the frog rollout with braking obstacles of tests/test_gpu_imm.py
# ---------------------------------------------------------------------------
STEPS = TC.FROG_STEPS


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(hist=[{k: v.clone() for k, v in h.items()
                                        if isinstance(v, torch.Tensor)} for h in cl.history],
                                 metrics=cl.metrics(), control=cl.control.clone())


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B, nO = 4, sc.nObst
    x_init = _x_init(sc, B)
    rows, brake = TC.frog_inputs(sc, B)
    exact = np.zeros((B, nO, 3))
    bank = tuple(a.numpy() for a in IMM.bank(exact, device="cpu"))
    trka = TRKA.matched(exact, device="cpu").numpy()
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("imm", dict(imm=bank)), ("imm_zero", dict(imm=bank, margin=(0.0, 1.0))),
                     ("imm_margin", dict(imm=bank, margin=(KAPPA, 1.0))),
                     ("trka", dict(tracker_accel=trka)),
                     ("trka_zero", dict(tracker_accel=trka, margin=(0.0, 1.0))),
                     ("trka_margin", dict(tracker_accel=trka, margin=(KAPPA, 1.0)))):
        cl.reset(x_init, seed=1, obstacles=rows, manoeuvres=brake, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, rows=rows, brake=brake, bank=bank,
                                trka=trka, runs=runs)
    cl.close()


@pytest.mark.parametrize("kind", ["imm", "trka"])
def test_rollout_with_zero_kappa_is_the_rollout_without_a_margin(rollouts, kind):
    a, b = rollouts.runs[kind], rollouts.runs[kind + "_zero"]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert set(b.hist[i]) - set(a.hist[i]) == {"obst_margin"}
        assert (b.hist[i]["obst_margin"] == 0).all()
        for k in a.hist[i]:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert torch.equal(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _beq(a.control, b.control)
    for k, v in a.metrics.items():
        assert torch.equal(v, b.metrics[k]), k


def test_rollout_hands_the_solve_what_the_margin_step_wrote(rollouts, gpu):
    ro, sc = rollouts, rollouts.sc
    lead = sc.delay_x + sc.dt + sc.delay_u
    rows, man = _dev(ro.rows, gpu), _dev(ro.brake, gpu)
    trk, sw = (_dev(a, gpu) for a in ro.bank)
    M = trk.shape[2]
    st = IMM.alloc(ro.B, sc.nObst, M, gpu)
    hist = ro.runs["imm_margin"].hist
    g0 = 0
    for i, rec in enumerate(hist):
        g1 = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x)
        snap = MAN.state(rows, man, g1 * sc.tick_length)
        ob, _, _, _ = IMM.step(snap, None, 0, i, 0, trk, sw, 0.0, (g1 - g0) * sc.tick_length, lead,
                               sc.dt, sc.Hp, *st)
        g0 = g1
        mg = MG.step(trk, *st, lead, sc.dt, sc.Hp, KAPPA, 1.0)
        assert _beq(rec["obst"], ob) and _beq(rec["obst_margin"], mg), i
        assert tuple(mg.shape) == (ro.B, sc.nObst, sc.Hp)
        assert torch.isfinite(mg).all() and (mg >= 0).all() and (mg <= 1.0).all()
        assert (rec["status"] & 0xff != ST_INVALID).all(), i
    assert (hist[-1]["obst_margin"] > 0).any()
    for kind in ("imm", "trka"):
        for rec in ro.runs[kind + "_margin"].hist:
            assert (rec["status"] & 0xff != ST_INVALID).all()


def test_rollout_solves_with_the_margin(rollouts, gpu):
    """One step from a start 8 m further along the lane (where obstacle rows bind at once, as in
    margin_cases' frog 1 x 10): the record is what a hand call of the solve with the recorded
    margin gives, and not what one without it gives."""
    ro, sc = rollouts, rollouts.sc
    x_init = ro.x_init.copy()
    x_init[:, :, 0] += 8.0
    ro.cl.reset(x_init, seed=1, obstacles=ro.rows, manoeuvres=ro.brake, imm=ro.bank,
                margin=(KAPPA, 1.0))
    ro.cl.run(1)
    rec = ro.cl.history[0]
    assert (rec["obst_margin"] > 0).any()
    S = ScpQpSolver(sc, max_batch=ro.B, hp_max=sc.Hp)
    out = S.solve(rec["x0"], rec["u0"], rec["ec_noise"], obst=rec["obst"],
                  obst_margin=rec["obst_margin"])
    without = S.solve(rec["x0"], rec["u0"], rec["ec_noise"], obst=rec["obst"],
                      out=S.alloc_out(ro.B))
    torch.cuda.synchronize()
    assert _beq(out.traj, rec["traj"]) and torch.equal(out.n_scp, rec["n_scp"])
    assert not _beq(without.traj, rec["traj"])
    S.close()


def test_reset_refuses_a_margin_without_a_six_state_tracker(rollouts):
    ro, cl = rollouts, rollouts.cl
    trk5 = TRK.matched(np.zeros((ro.B, ro.sc.nObst, 3)), device="cpu").numpy()
    for kw in (dict(), dict(tracker=trk5)):
        with pytest.raises(ValueError, match="tracker_accel= or imm="):
            cl.reset(ro.x_init, seed=1, obstacles=ro.rows, margin=(1.0, 1.0), **kw)
    for bad in ((-1.0, 1.0), (1.0, float("inf")), 2.0):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, obstacles=ro.rows, tracker_accel=ro.trka, margin=bad)
    cl.reset(ro.x_init, seed=1, obstacles=ro.rows, manoeuvres=ro.brake, tracker_accel=ro.trka,
             margin=(1.0, 1.0))
