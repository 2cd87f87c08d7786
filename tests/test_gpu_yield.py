"""Right of way and graded braking on the GPU (include/scpqp_yield.h).

Step: every case of tests/yield_cases.py against the mirror (tests/yield_mirror.py): k_conf,
k_any and who exactly, a_cmd, clear and d_stop at the tolerance derived on the CPU
(yield_cases.TOL); the reduction to ``governor.step``, bitwise on every case; off lanes, lane
isolation, split batches, NULL outputs and non-finite plans.

Rollout: reducing rows against ``governor=`` bitwise on ``governor_cases.stop_scene`` and on
four steps of c2; off rows against ``right_of_way=None``; the crossing scene of
``yield_cases.crossing_scene`` with equal and with distinct ranks.
"""
import types

import numpy as np
import pytest
import torch

import governor_cases as GC
import yield_cases as YC
import yield_mirror as YM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import governor as GOV
from scpqp import obstacles as OB
from scpqp import yielding as YLD

pytestmark = pytest.mark.gpu

INF = float("inf")
F_OUT, I_OUT = (0, 2, 5), (1, 3, 4)        # a_cmd, clear, d_stop; k_conf, k_any, who


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64),
                                                   b.contiguous().view(torch.int64)))


def _dev(a, gpu, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _np(t):
    return t.cpu().numpy()


def _args(gpu, cid, d, sel):
    g = lambda k, dt=torch.float64: None if d[k] is None else _dev(d[k][sel], gpu, dt)
    return (g("x0"), g("traj"), g("obst"), g("margin"), g("dreq_obs"), g("dreq_veh"), YC.T_HOLD,
            YC.T_BACK), dict(hp=g("hp", torch.int32), hp_max=YC.by_id(cid).hp_max)


def device_step(gpu, cid, d=None, sel=slice(None), diag=True, rows=None):
    """The case (or ``d``, a changed copy of its inputs; ``sel``: a slice of the batch; ``rows``:
    other rows) on the device."""
    d = YC.inputs(cid) if d is None else d
    args, kw = _args(gpu, cid, d, sel)
    rows = d["rows"] if rows is None else rows
    return YLD.step(_dev(rows[sel], gpu), *args, diag=diag, **kw)


def changed(cid, **over):
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in YC.inputs(cid).items()}
    d.update(over)
    return d


def same(a, b, sel=None):
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    return all(_beq(pick(a[i]), pick(b[i])) for i in F_OUT) \
        and all(bool(torch.equal(pick(a[i]), pick(b[i]))) for i in I_OUT)


# ---------------------------------------------------------------------------
# 1. the step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", YC.IDS)
def test_step_matches_the_mirror(gpu, cid):
    out = device_step(gpu, cid)
    torch.cuda.synchronize()
    m = YC.mirror(cid)
    for i in I_OUT:
        assert np.array_equal(_np(out[i]), m[i]), i
    worst = YC.ratio([_np(t) for t in out], m, cid)
    print(f"yield {cid}: largest device - mirror ratio {worst:.3e} (TOL {YC.TOL:.3e})")
    assert worst <= YC.TOL
    # in a lane that is neither off nor bad d_stop is +inf exactly where no conflict counts,
    # and k_any is never later than k_conf
    k, ka, ds = _np(out[1]), _np(out[3]), _np(out[5])
    live = ~np.isnan(m[2])
    assert live.any() and ((ds == INF) == (k == -1))[live].all() and np.isnan(ds[~live]).all()
    assert ((k < 0) | ((ka >= 0) & (ka <= k))).all()


@pytest.mark.parametrize("cid", YC.IDS)
def test_reduction_to_the_governor_is_bitwise(gpu, cid):
    """Equal ranks, A_EASE = A_BRAKE, S_STAND = 0: a_cmd, k_conf and clear of governor.step, bit
    for bit, and k_any = k_conf."""
    d = YC.inputs(cid)
    rows, grows = YC.reducing(cid)
    args, kw = _args(gpu, cid, d, slice(None))
    y = YLD.step(_dev(rows, gpu), *args, **kw)
    g = GOV.step(_dev(grows, gpu), *args, **kw)
    assert _beq(y[0], g[0]) and torch.equal(y[1], g[1]) and _beq(y[2], g[2])
    assert torch.equal(y[3], y[1])
    only = YLD.step(_dev(rows, gpu), *args, diag=False, **kw)
    assert _beq(only[0], g[0])


def test_off_lanes_copy_the_acceleration_bitwise(gpu):
    cid = "5x2x10"
    d = changed(cid)
    base = device_step(gpu, cid)
    # rows that are valid in every vehicle, so that an off row changes only who counts
    assert d["pattern"][2] == "descending" and d["pattern"][3] == "ties"
    off = [(2, 0), (2, 3), (3, 2)]
    for b, v in off:
        d["rows"][b, v] = 0.0
    d["rows"][2, 3, YM.A_EASE] = -0.0
    x0 = torch.as_tensor(d["x0"])
    x0[2, 0, 4] = -0.0
    x0[2, 3] = float("nan")
    x0.view(torch.int64)[3, 2, 4] = 0x7FF8_0000_DEAD_BEEF          # a NaN with a payload
    d["x0"] = x0.numpy()
    out = device_step(gpu, cid, d)
    xd = _dev(d["x0"], gpu)
    for b, v in off:
        assert _beq(out[0][b, v].reshape(1), xd[b, v, 4].reshape(1))
        assert out[1][b, v] == -1 and out[3][b, v] == -1 and out[4][b, v] == -1
        assert torch.isnan(out[2][b, v]) and torch.isnan(out[5][b, v])
    rest = [b for b in range(16) if b not in (2, 3)]
    assert same(out, base, rest)
    # an all-off batch reads nothing but x0[..., 4]: canaries everywhere else
    d = changed(cid)
    d["rows"][:] = 0.0
    for key in ("traj", "obst", "margin", "dreq_obs", "dreq_veh"):
        d[key][:] = np.nan
    d["x0"][..., :4] = np.nan
    out = device_step(gpu, cid, d)
    assert _beq(out[0], _dev(d["x0"], gpu)[..., 4])
    assert all((out[i] == -1).all() for i in I_OUT)
    assert torch.isnan(out[2]).all() and torch.isnan(out[5]).all()


def test_lane_isolation(gpu):
    cid = "5x2x10"
    inp = YC.inputs(cid)
    base = device_step(gpu, cid)
    B, nV = base[0].shape
    # one lane's own tuning: that lane only (A_BRAKE, BAND and A_EASE are not asked of others)
    d = changed(cid)
    assert inp["pattern"][3] == "ties"
    d["rows"][3, 2, YM.A_BRAKE] += 0.5
    d["rows"][3, 2, YM.BAND] += 4.0                          # its neighbours at 6 m now conflict
    got = device_step(gpu, cid, d)
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[3, 2] = False
    assert same(got, base, keep) and got[3][3, 2] == 0 and base[3][3, 2] == -1
    # one lane's rank: its own lane and, through rule 2, the vehicles of its realisation only
    d = changed(cid)
    d["rows"][3, 2, YM.PRIO] = 9.0
    got = device_step(gpu, cid, d)
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[3] = False
    assert same(got, base, keep)
    # a bad lane writes its own outputs and disturbs the others only in that it is now yielded
    # to (rule 2 (a)).  Realisation 14 ("zero": descending ranks, nothing planted but the pair
    # at step 1) with vehicle 0 looking over its horizon: it outranks vehicle 1 and does not yield
    d0 = changed(cid)
    assert inp["pattern"][14] == "zero" and inp["kind"][14] == "clamp"
    d0["rows"][14, 0, YM.LOOK] = 10
    base0 = device_step(gpu, cid, d0)
    assert base0[3][14, 0] == 1 and base0[1][14, 0] == -1 and base0[4][14, 0] == -1
    d = changed(cid, rows=d0["rows"].copy())
    d["rows"][14, 1, YM.PRIO] = 0.5
    d["x0"][9, 3, 3] = np.nan                                # a bad state: its row is not bad
    got = device_step(gpu, cid, d)
    m = YM.step(d["rows"], d["x0"], d["traj"], d["obst"], d["margin"], d["hp"], d["dreq_obs"],
                d["dreq_veh"], YC.T_HOLD, YC.T_BACK, 10)
    for b, v in ((14, 1), (9, 3)):
        assert torch.isnan(got[0][b, v]) and torch.isnan(got[2][b, v]) and torch.isnan(got[5][b, v])
        assert got[1][b, v] == -2 and got[3][b, v] == -2 and got[4][b, v] == -2
    for i in I_OUT:
        assert np.array_equal(_np(got[i]), m[i]), i
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[14, :2] = False                                     # the bad lane, and who yields to it
    keep[9, 3] = False                                       # S_STAND = 0 there: nobody asks its speed
    assert same(got, base0, keep)
    assert got[1][14, 0] == 1 and got[4][14, 0] == 2 + 1     # who = n_obst + w
    # canaries: the C entry point on output buffers one realisation longer than the batch of
    # 15 (75 lanes: the last workgroup holds groups past the batch).  Every lane of the batch is
    # written with what the whole batch gave, and the neighbour past it keeps its canaries
    from scpqp.plant import _ptr, _stream
    n = 15
    (x0, traj, obst, margin, do, dv, th, tb), _ = _args(gpu, cid, inp, slice(0, n))
    rows = _dev(inp["rows"][:n], gpu)
    fl = [torch.full((n + 1, nV), -7.25, dtype=torch.float64, device=gpu) for _ in range(3)]
    it = [torch.full((n + 1, nV), -77, dtype=torch.int32, device=gpu) for _ in range(3)]
    lib = LB.load()
    LB.check(lib.scpqp_yield_step(nV, 2, 10, n, th, tb, _ptr(x0), _ptr(traj), _ptr(obst),
                                  _ptr(margin), None, _ptr(do), _ptr(dv), _ptr(rows), _ptr(fl[0]),
                                  _ptr(it[0]), _ptr(it[1]), _ptr(it[2]), _ptr(fl[1]), _ptr(fl[2]),
                                  _stream(gpu)), lib)
    torch.cuda.synchronize()
    out = (fl[0], it[0], fl[1], it[1], it[2], fl[2])         # the order of yielding.step
    assert same([t[:n] for t in out], base, slice(0, n))
    assert all((t[n] == -7.25).all() for t in fl) and all((t[n] == -77).all() for t in it)


@pytest.mark.parametrize("cid", ["5x2x10", "3x2x30_mixed", "16x32x64"])
def test_a_split_batch_gives_what_the_whole_gives(gpu, cid):
    whole = device_step(gpu, cid)
    B = whole[0].shape[0]
    for cut in (1, B // 2 + 1):
        parts = [device_step(gpu, cid, sel=s) for s in (slice(0, cut), slice(cut, B))]
        for i in range(6):
            cat = torch.cat([p[i] for p in parts])
            assert torch.equal(cat, whole[i]) if i in I_OUT else _beq(cat, whole[i]), (cut, i)


@pytest.mark.parametrize("cid", ["1x0x3", "5x2x10_nomargin", "16x32x64"])
def test_null_outputs_leave_the_command_alone(gpu, cid):
    full = device_step(gpu, cid)
    only = device_step(gpu, cid, diag=False)
    assert all(t is None for t in only[1:]) and _beq(only[0], full[0])


def test_non_finite_plans(gpu):
    cid = "5x2x10"
    d = changed(cid)
    B, nV = d["rows"].shape[:2]
    # realisations 0 and 8 are clear but for the planted pair; take that out as well
    assert d["kind"][0] == "clear" and d["kind"][8] == "clear"
    g = GC.inputs(cid)
    for b in (0, 8):
        d["traj"][b] = g["traj"][b]
        d["rows"][b, :, YM.LOOK] = 4
        d["rows"][b, :, YM.J_MAX] = INF
        d["rows"][b, :, YM.PRIO] = nV - 1 - np.arange(nV)   # descending: vehicle 0 on top
        d["rows"][b, :, YM.S_STAND] = 0.0
        d["x0"][b, :, 3] = 4.0
    plain = device_step(gpu, cid, d)
    assert (plain[1][[0, 8]] == -1).all() and (plain[3][[0, 8]] == -1).all()
    e = changed(cid, rows=d["rows"], x0=d["x0"], traj=d["traj"].copy())
    e["traj"][0, 2, 1, 4] = np.nan                           # the lowest rank of b = 0 at step 2
    e["obst"][8, 1, 0, 3] = np.nan                           # obstacle 1 of b = 8 at step 3
    got = device_step(gpu, cid, e)
    # what is not a number counts whatever the ranks: every vehicle yields to vehicle 4
    assert got[1][0].tolist() == [2] * nV and got[3][0].tolist() == [2] * nV
    # who = n_obst + w; in vehicle 4's own lane every pair of step 2 is not a number: obstacle 0
    assert got[4][0].tolist() == [2 + 4] * 4 + [0]
    assert got[1][8].tolist() == [3] * nV and got[4][8].tolist() == [1] * nV
    for b in (0, 8):
        assert (got[2][b] == -INF).all()
    # d_stop ends at the last point before the conflict: finite in every lane
    assert torch.isfinite(got[5][0, :4]).all() and torch.isfinite(got[5][8]).all()
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[[0, 8]] = False
    assert same(got, plain, keep)
    mir = YM.step(e["rows"], e["x0"], e["traj"], e["obst"], e["margin"], e["hp"], e["dreq_obs"],
                  e["dreq_veh"], YC.T_HOLD, YC.T_BACK, 10)
    for i in I_OUT:
        assert np.array_equal(_np(got[i]), mir[i]), i
    assert (np.isnan(_np(got[0])) == np.isnan(mir[0])).all()
    # a plan start that is not a number: d_stop is not finite, a_cmd is full braking
    e2 = changed(cid, rows=e["rows"], x0=e["x0"].copy(), traj=e["traj"])
    e2["x0"][0, 1, 0] = np.nan
    got2 = device_step(gpu, cid, e2)
    assert got2[1][0, 1] == 2 and torch.isnan(got2[5][0, 1])
    assert got2[0][0, 1] == -e2["rows"][0, 1, YM.A_BRAKE]   # s = 4: the stop rule is not near
    # the same entries past LOOK are ignored
    e = changed(cid, rows=d["rows"], x0=d["x0"], traj=d["traj"].copy())
    e["traj"][0, 4, 1, 4] = np.nan                           # step 4 = LOOK: not examined
    e["obst"][8, 1, 0, 4:] = np.nan
    e["margin"][8, 0, 4:] = np.nan
    assert same(device_step(gpu, cid, e), plain)


def test_python_side_refuses_what_does_not_fit(gpu):
    cid = "5x2x10"
    d = YC.inputs(cid)
    t = {k: _dev(v, gpu) for k, v in d.items() if isinstance(v, np.ndarray) and k != "hp"}
    args = lambda **o: [o.get(k, t[k]) for k in ("rows", "x0", "traj", "obst", "margin",
                                                 "dreq_obs", "dreq_veh")]
    YLD.step(*args(), 0.4, 0.03)
    for o in (dict(rows=t["rows"].cpu()), dict(rows=t["rows"][..., :7].contiguous()),
              dict(x0=t["x0"][:, :4]), dict(traj=t["traj"][:, :9]),
              dict(dreq_veh=t["dreq_veh"][:3]), dict(margin=t["margin"].float())):
        with pytest.raises(ValueError):
            YLD.step(*args(**o), 0.4, 0.03)
    for th, tb in ((0.0, 0.03), (0.4, -0.01), (INF, 0.0)):
        with pytest.raises(RuntimeError, match="t_hold|t_back"):
            YLD.step(*args(), th, tb)


# ---------------------------------------------------------------------------
# 2. rollout
# ---------------------------------------------------------------------------
def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl):
    return types.SimpleNamespace(hist=[{k: v.clone() for k, v in h.items()
                                        if isinstance(v, torch.Tensor)} for h in cl.history],
                                 metrics=cl.metrics(), control=cl.control.clone(),
                                 state=cl.state.clone())


def _same_runs(a, b, extra=()):
    """Records, control, state and metrics bit for bit; ``extra``: the keys only b has."""
    assert len(a.hist) == len(b.hist)
    for i in range(len(a.hist)):
        assert set(b.hist[i]) - set(a.hist[i]) == set(extra) and set(a.hist[i]) <= set(b.hist[i])
        for k in a.hist[i]:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert torch.equal(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _beq(a.control, b.control) and _beq(a.state, b.state)
    for k, v in a.metrics.items():
        assert torch.equal(v, b.metrics[k]), k


NEW_KEYS = ("gov_k_any", "gov_who", "gov_d_stop")


def test_rollout_with_reducing_rows_is_the_governed_rollout_on_the_stop_scene(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc, x_init, kw = GC.stop_scene()
    B = GC.STOP_B
    obst = OB.nominal(sc, B, device=gpu)
    gov = GOV.rows(B, 1, device=gpu, **kw)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = []
    for extra in (dict(governor=gov), dict(right_of_way=YLD.from_governor(gov, 0))):
        cl.reset(x_init, obstacles=obst, **extra)
        cl.run(GC.STOP_STEPS)
        runs.append(_snapshot(cl))
    _same_runs(*runs, extra=NEW_KEYS)
    last = runs[1].hist[-1]
    assert (runs[1].metrics["first_collision_tick"] < 0).all()
    assert (runs[1].hist[0]["gov_who"] == 0).all() and (runs[1].hist[0]["gov_d_stop"] == 0).all()
    assert last["gov_k_any"].dtype == torch.int32
    # passing both is refused, and so are rows that do not fit; nothing is launched
    with pytest.raises(ValueError, match="one of"):
        cl.reset(x_init, obstacles=obst, governor=gov, right_of_way=YLD.from_governor(gov, 0))
    with pytest.raises(ValueError, match=r"\[B, nVeh, 10\]"):
        cl.reset(x_init, obstacles=obst, right_of_way=gov)
    bad = YLD.from_governor(gov, 0)
    bad[1, 0, YM.A_EASE] = 5.0
    with pytest.raises(ValueError, match="a_ease"):
        cl.reset(x_init, obstacles=obst, right_of_way=bad)
    assert len(cl.history) == GC.STOP_STEPS
    cl.close()


def test_rollout_on_c2_reducing_rows_and_off_rows(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(4, Hp=20)
    B, steps = 4, 4
    x_init = _x_init(sc, B)
    gov = GOV.rows(B, 4, v_ref=4.0, a_acc=1.0, a_brake=3.0, k_v=0.5, look=20, band=2.0, device=gpu)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, extra in (("governed", dict(governor=gov)),
                        ("reducing", dict(right_of_way=YLD.from_governor(gov, 5))),
                        ("free", dict()), ("off", dict(right_of_way=YLD.off(B, 4, device=gpu)))):
        cl.reset(x_init, seed=1, **extra)
        cl.run(steps)
        runs[name] = _snapshot(cl)
    cl.close()
    _same_runs(runs["governed"], runs["reducing"], extra=NEW_KEYS)
    _same_runs(runs["free"], runs["off"])
    assert all("accel_cmd" not in h for h in runs["off"].hist)
    # the comparison is not an empty one: the governed run saw conflicts and differs from the free
    kc = torch.stack([h["gov_k_conf"] for h in runs["reducing"].hist])
    print("c2 reducing rows: share of lanes with a conflict", float((kc >= 0).float().mean()))
    assert (kc >= 0).any() and not _beq(runs["governed"].state, runs["free"].state)


@pytest.fixture(scope="module")
def crossing(gpu):
    from scpqp.rollout import ClosedLoopBatch
    scs, variant_of, x_init, ranks = YC.crossing_scene()
    B = YC.CROSS_B
    rows = YLD.from_governor(GOV.rows(B, 2, device=gpu, **YC.CROSS_KW), ranks)
    cl = ClosedLoopBatch(scs[0], B, device=gpu, keep_path=True, metrics=True, variants=scs,
                         variant_of=variant_of)
    cl.reset(x_init, right_of_way=rows)
    cl.run(YC.CROSS_STEPS)
    run = _snapshot(cl)
    torch.cuda.synchronize()
    yield types.SimpleNamespace(scs=scs, variant_of=variant_of, ranks=ranks, rows=rows, run=run)
    cl.close()


def test_crossing_with_equal_and_with_distinct_ranks(crossing):
    """What follows from the definition is asserted; collisions, progress and speeds of the
    runs are printed, not asserted."""
    run, ranks = crossing.run, crossing.ranks
    stack = lambda k: torch.stack([h[k] for h in run.hist])          # [steps, B, 2]
    kc, ka, who, acc = stack("gov_k_conf"), stack("gov_k_any"), stack("gov_who"), stack("accel_cmd")
    status = stack("status")
    speed = torch.stack([h["path"][:, :, -1, 3] for h in run.hist])
    for b, (variant, r0, r1) in enumerate(YC.CROSS_RUNS):
        print(f"crossing b={b} variant {variant} ranks ({r0}, {r1}): first collision tick "
              f"{int(run.metrics['first_collision_tick'][b])}, min gap "
              f"{float(run.metrics['min_gap_veh'][b].min()):.3f} m")
        for v in range(2):
            print(f"  vehicle {v}: k_conf {kc[:, b, v].tolist()} k_any {ka[:, b, v].tolist()} "
                  f"who {who[:, b, v].tolist()}")
            print(f"    accel_cmd {[round(x, 3) for x in acc[:, b, v].tolist()]} speed "
                  f"{[round(x, 3) for x in speed[:, b, v].tolist()]} x, y at the end "
                  f"{[round(x, 2) for x in run.state[b, v, :2].tolist()]}")
    print("  status words", sorted(set(status.flatten().tolist())))
    # equal ranks: a step in which both vehicles yield (what makes the scene relevant)
    for b in (0, 1):
        assert ranks[b, 0] == ranks[b, 1]
        assert ((kc[:, b, 0] >= 0) & (kc[:, b, 1] >= 0)).any(), b
    # distinct ranks: the higher-ranked vehicle never yields to a vehicle, while the other is
    # in its way in at least one step
    for b in (2, 3):
        hi = int(np.argmax(ranks[b]))
        assert ranks[b, hi] > ranks[b, 1 - hi]
        assert (who[:, b, hi] < 0).all() and (kc[:, b, hi] == -1).all(), b     # no obstacle here
        assert (ka[:, b, hi] >= 0).any(), b
    # every status word is one the governor's section of DESIGN lists
    assert set(status.flatten().tolist()) <= {0, LB.FL_POLISH_REJECTED}
    assert ((status & 0xFF) != LB.ST_NUMERIC).all()


def test_crossing_records_what_the_step_and_the_mirror_give(crossing, gpu):
    scs, run = crossing.scs, crossing.run
    sc = scs[0]
    dreq = YLD.required(sc, scs, crossing.variant_of, device=gpu)
    keys = ("accel_cmd", "gov_k_conf", "gov_clear", "gov_k_any", "gov_who", "gov_d_stop")
    for i, rec in enumerate(run.hist):
        out = YLD.step(crossing.rows, rec["x0"], rec["traj"], None, None, *dreq, sc.dt, sc.delay_u)
        for k, t in zip(keys, out):
            assert torch.equal(t, rec[k]) if t.dtype == torch.int32 else _beq(t, rec[k]), (i, k)
        if i:
            assert (rec["x0"][:, :, 4] == run.hist[i - 1]["accel_cmd"]).all(), i
        m = YM.step(_np(crossing.rows), _np(rec["x0"]), _np(rec["traj"]), None, None, None, None,
                    _np(dreq[1]), sc.dt, sc.delay_u, YC.CROSS_HP)
        for j in I_OUT:
            assert np.array_equal(_np(out[j]), m[j]), (i, j)
