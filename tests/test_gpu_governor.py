"""The speed governor on the GPU (include/scpqp_governor.h).

Governor step: every case of tests/governor_cases.py against the mirror
(tests/governor_mirror.py): k_conf exactly, a_cmd and clear at the tolerance derived on the CPU
(governor_cases.TOL); off lanes, lane isolation, split batches, NULL outputs, bad lanes and
non-finite plans.

Rollout: off rows against ``governor=None`` bitwise on c2 and frog; the scene of
``governor_cases.stop_scene``, in which stopping is the only way out, without and with the
governor.
"""
import types

import numpy as np
import pytest
import torch

import governor_cases as GC
import governor_mirror as GM
from oracle import scp_reference as R
from scpqp import _lib as LB
from scpqp import governor as GOV
from scpqp import obstacles as OB

pytestmark = pytest.mark.gpu

INF = float("inf")


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64),
                                                   b.contiguous().view(torch.int64)))


def _dev(a, gpu, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _np(t):
    return t.cpu().numpy()


def device_step(gpu, cid, d=None, sel=slice(None), diag=True):
    """The case (or ``d``, a changed copy of its inputs; ``sel``: a slice of the batch) on the
    device."""
    c = GC.by_id(cid)
    d = GC.inputs(cid) if d is None else d
    g = lambda k, dt=torch.float64: None if d[k] is None else _dev(d[k][sel], gpu, dt)
    return GOV.step(g("rows"), g("x0"), g("traj"), g("obst"), g("margin"), g("dreq_obs"),
                    g("dreq_veh"), GC.T_HOLD, GC.T_BACK, hp=g("hp", torch.int32),
                    hp_max=c.hp_max, diag=diag)


def changed(cid, **over):
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in GC.inputs(cid).items()}
    d.update(over)
    return d


def same(a, b, sel=None):
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    return _beq(pick(a[0]), pick(b[0])) and bool(torch.equal(pick(a[1]), pick(b[1]))) \
        and _beq(pick(a[2]), pick(b[2]))


# ---------------------------------------------------------------------------
# 1. the governor step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", GC.IDS)
def test_step_matches_the_mirror(gpu, cid):
    a, k, c = device_step(gpu, cid)
    torch.cuda.synchronize()
    m = GC.mirror(cid)
    assert np.array_equal(_np(k), m[1])
    worst = GC.ratio((_np(a), None, _np(c)), m, cid)
    print(f"governor {cid}: largest device - mirror ratio {worst:.3e} (TOL {GC.TOL:.3e})")
    assert worst <= GC.TOL
    # nothing examined: clear = +inf (and the mirror has such lanes in every case)
    det = GC.mirror(cid, details=True)
    none = np.array([[not det[(b, v)]["clearances"] for v in range(m[0].shape[1])]
                     for b in range(m[0].shape[0])])
    assert none.any() and (_np(c)[none] == INF).all() and np.isfinite(_np(c)[~none]).all()


def test_off_lanes_copy_the_acceleration_bitwise(gpu):
    cid = "5x2x10"
    d = changed(cid)
    base = device_step(gpu, cid)
    # off rows in a mixed batch; -0.0 and NaN payloads, and NaN everywhere else in other lanes
    off = [(1, 0), (1, 3), (6, 2), (15, 4)]
    for b, v in off:
        d["rows"][b, v] = 0.0
    d["rows"][1, 3, 2] = -0.0
    x0 = torch.as_tensor(d["x0"])
    x0[1, 0, 4] = -0.0
    x0[1, 3] = float("nan")
    x0.view(torch.int64)[6, 2, 4] = 0x7FF8_0000_DEAD_BEEF          # a NaN with a payload
    d["x0"] = x0.numpy()
    a, k, c = device_step(gpu, cid, d)
    xd = _dev(d["x0"], gpu)
    for b, v in off:
        assert _beq(a[b, v].reshape(1), xd[b, v, 4].reshape(1)) and k[b, v] == -1 \
            and torch.isnan(c[b, v])
    # realisations without a changed lane are what they were
    rest = [b for b in range(16) if b not in (1, 6, 15)]
    assert same((a, k, c), base, rest)
    # an all-off batch reads nothing but x0[..., 4]: canaries everywhere else
    d = changed(cid)
    d["rows"][:] = 0.0
    for key in ("traj", "obst", "margin", "dreq_obs", "dreq_veh"):
        d[key][:] = np.nan
    d["x0"][..., :4] = np.nan
    a, k, c = device_step(gpu, cid, d)
    assert _beq(a, _dev(d["x0"], gpu)[..., 4]) and (k == -1).all() and torch.isnan(c).all()


def test_lane_isolation(gpu):
    cid = "5x2x10"
    base = device_step(gpu, cid)
    B, nV = base[0].shape
    # one lane's row: that lane only
    d = changed(cid)
    d["rows"][3, 2, GM.A_BRAKE] += 0.5
    d["rows"][3, 2, GM.BAND] += 4.0                          # its neighbours at 6 m now conflict
    got = device_step(gpu, cid, d)
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[3, 2] = False
    assert same(got, base, keep) and got[0][3, 2] != base[0][3, 2]
    assert got[1][3, 2] == 0 and base[1][3, 2] == -1
    # one vehicle's plan: its own lane and, through the pair distances, the other vehicles of
    # its realisation; no other realisation
    d = changed(cid)
    assert GC.inputs(cid)["kind"][8] == "clear" and (base[1][8] == -1).all()
    d["traj"][8, 0, :, 2] = d["traj"][8, 0, :, 3] + (0.1, 0.1)     # vehicle 2 onto vehicle 3
    got = device_step(gpu, cid, d)
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[8] = False
    assert same(got, base, keep)
    looks = d["rows"][8, :, GM.LOOK]
    assert looks[2] >= 1 and looks[3] >= 1
    # a pair conflict changes both vehicles of the pair, and they brake
    assert got[1][8, 2] == 0 and got[1][8, 3] == 0
    m = GM.step(d["rows"], d["x0"], d["traj"], d["obst"], d["margin"], d["hp"], d["dreq_obs"],
                d["dreq_veh"], GC.T_HOLD, GC.T_BACK, 10)
    assert np.array_equal(_np(got[1]), m[1])


@pytest.mark.parametrize("cid", ["5x2x10", "3x2x30_mixed", "16x32x64"])
def test_a_split_batch_gives_what_the_whole_gives(gpu, cid):
    whole = device_step(gpu, cid)
    B = whole[0].shape[0]
    for cut in (1, B // 2 + 1):
        parts = [device_step(gpu, cid, sel=s) for s in (slice(0, cut), slice(cut, B))]
        for i in range(3):
            cat = torch.cat([p[i] for p in parts])
            assert torch.equal(cat, whole[i]) if i == 1 else _beq(cat, whole[i]), (cut, i)


@pytest.mark.parametrize("cid", ["1x0x3", "5x2x10_nomargin", "16x32x64"])
def test_null_outputs_leave_the_command_alone(gpu, cid):
    full = device_step(gpu, cid)
    only = device_step(gpu, cid, diag=False)
    assert only[1] is None and only[2] is None and _beq(only[0], full[0])


def test_bad_lanes_and_non_finite_plans(gpu):
    cid = "5x2x10"
    base = device_step(gpu, cid)
    B, nV = base[0].shape
    d = changed(cid)
    bad = {(0, 1): (GM.A_BRAKE, -1e-300), (2, 4): (GM.K_V, np.nan), (5, 0): (GM.LOOK, 2.5),
           (7, 3): (GM.LOOK, 65.0), (9, 2): (GM.V_REF, INF), (11, 1): (GM.J_MAX, -INF)}
    for (b, v), (f, val) in bad.items():
        d["rows"][b, v, f] = val
    d["x0"][12, 3, 3] = np.nan                               # s
    d["x0"][13, 0, 4] = INF                                  # a_now
    lanes = list(bad) + [(12, 3), (13, 0)]
    got = device_step(gpu, cid, d)
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    for b, v in lanes:
        keep[b, v] = False
        assert torch.isnan(got[0][b, v]) and got[1][b, v] == -2 and torch.isnan(got[2][b, v])
    assert same(got, base, keep)
    # a horizon outside its slot is a bad lane in every vehicle of its problem
    cm = "3x2x30_mixed"
    dm = changed(cm)
    dm["hp"][4], dm["hp"][5] = 31, 0
    gm_, bm = device_step(gpu, cm, dm), device_step(gpu, cm)
    assert (gm_[1][4:6] == -2).all() and torch.isnan(gm_[0][4:6]).all()
    keep = torch.ones_like(bm[1], dtype=torch.bool)
    keep[4:6] = False
    assert same(gm_, bm, keep)
    # a NaN in an examined traj or obst entry brakes at that step and does not NaN the lane;
    # the same NaN past LOOK is ignored
    d = changed(cid)
    assert d["kind"][0] == "clear" and d["kind"][8] == "clear"
    d["rows"][0, :, GM.LOOK] = 4
    d["rows"][8, :, GM.LOOK] = 4
    d["rows"][[0, 8], :, GM.J_MAX] = INF
    d["x0"][[0, 8], :, 3] = 4.0
    plain = device_step(gpu, cid, d)
    assert (plain[1][[0, 8]] == -1).all()
    e = changed(cid, rows=d["rows"], x0=d["x0"])
    e["traj"][0, 2, 1, 1] = np.nan                           # vehicle 1 of b = 0 at step 2
    e["obst"][8, 1, 0, 3] = np.nan                           # obstacle 1 of b = 8 at step 3
    got = device_step(gpu, cid, e)
    assert got[1][0].tolist() == [2] * nV                    # every vehicle's pair with vehicle 1
    assert got[1][8].tolist() == [3] * nV
    for b in (0, 8):
        assert (got[2][b] == -INF).all()
        assert _beq(got[0][b], -_dev(d["rows"][b, :, GM.A_BRAKE], gpu))   # s = 4: no stop rule
    keep = torch.ones(B, nV, dtype=torch.bool, device=gpu)
    keep[[0, 8]] = False
    assert same(got, plain, keep)
    e = changed(cid, rows=d["rows"], x0=d["x0"])
    e["traj"][0, 4, 1, 1] = np.nan                           # step 4 = LOOK: not examined
    e["obst"][8, 1, 0, 4:] = np.nan
    e["margin"][8, 0, 4:] = np.nan
    assert same(device_step(gpu, cid, e), plain)


def test_python_side_refuses_what_does_not_fit(gpu):
    cid = "5x2x10"
    d = GC.inputs(cid)
    t = {k: _dev(v, gpu) for k, v in d.items() if isinstance(v, np.ndarray) and k != "hp"}
    args = lambda **o: [o.get(k, t[k]) for k in ("rows", "x0", "traj", "obst", "margin",
                                                 "dreq_obs", "dreq_veh")]
    GOV.step(*args(), 0.4, 0.03)
    # required() without variants has a leading extent of 1: repeated over the batch
    one = GOV.step(*args(dreq_obs=t["dreq_obs"][:1], dreq_veh=t["dreq_veh"][:1]), 0.4, 0.03)
    rep = GOV.step(*args(dreq_obs=t["dreq_obs"][:1].expand(16, -1, -1).contiguous(),
                         dreq_veh=t["dreq_veh"][:1].expand(16, -1, -1).contiguous()), 0.4, 0.03)
    assert same(one, rep)
    for o in (dict(rows=t["rows"].cpu()), dict(x0=t["x0"][:, :4]), dict(traj=t["traj"][:, :9]),
              dict(dreq_veh=t["dreq_veh"][:3]), dict(margin=t["margin"].float())):
        with pytest.raises(ValueError):
            GOV.step(*args(**o), 0.4, 0.03)
    for th, tb in ((0.0, 0.03), (0.4, -0.01), (INF, 0.0)):
        with pytest.raises(RuntimeError, match="t_hold|t_back"):
            GOV.step(*args(), th, tb)


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
                                 metrics=cl.metrics(), control=cl.control.clone())


@pytest.mark.parametrize("name", ["c2", "frog"])
def test_rollout_with_off_rows_is_the_rollout_without_a_governor(gpu, name):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(4, Hp=20) if name == "c2" else R.frog_scenario(Hp=10)
    B, steps = 8, 6
    x_init = _x_init(sc, B)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = []
    for gov in (None, GOV.off(B, sc.nVeh, device=gpu)):
        cl.reset(x_init, seed=1, governor=gov)
        cl.run(steps)
        runs.append(_snapshot(cl))
    a, b = runs
    assert len(a.hist) == len(b.hist) == steps
    for i in range(steps):
        assert set(a.hist[i]) == set(b.hist[i]) and "path" in a.hist[i]
        for k in a.hist[i]:
            if a.hist[i][k].dtype == torch.float64:
                assert _beq(a.hist[i][k], b.hist[i][k]), (i, k)
            else:
                assert torch.equal(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _beq(a.control, b.control)
    for k, v in a.metrics.items():
        assert torch.equal(v, b.metrics[k]), k
    # a refused reset changes nothing and launches nothing
    bad = GOV.off(B, sc.nVeh, device=gpu)
    bad[2, 0, GM.A_BRAKE] = -1.0
    with pytest.raises(ValueError, match="a_brake"):
        cl.reset(x_init, seed=1, governor=bad)
    with pytest.raises(ValueError, match=r"\[B, nVeh, 7\]"):
        cl.reset(x_init, seed=1, governor=GOV.off(B + 1, sc.nVeh, device=gpu))
    assert len(cl.history) == steps
    cl.close()


@pytest.fixture(scope="module")
def stop_runs(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc, x_init, kw = GC.stop_scene()
    B = GC.STOP_B
    rows = OB.nominal(sc, B, device=gpu)
    assert (rows[:, :, LB.OBST_SPEED] == 0).all()
    gov = GOV.rows(B, 1, device=gpu, **kw)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, g in (("free", None), ("governed", gov)):
        cl.reset(x_init, obstacles=rows, governor=g)
        cl.run(GC.STOP_STEPS)
        runs[name] = _snapshot(cl)
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, B=B, runs=runs, kw=kw)
    cl.close()


def test_without_the_governor_every_realisation_collides(stop_runs):
    first = stop_runs.runs["free"].metrics["first_collision_tick"]
    print("stop scene, no governor: first collision ticks", first.tolist())
    assert (first >= 0).all()
    assert all("accel_cmd" not in h for h in stop_runs.runs["free"].hist)


def test_with_the_governor_the_vehicle_stops_in_front_of_the_obstacle(stop_runs):
    ro, sc = stop_runs, stop_runs.sc
    run = ro.runs["governed"]
    first = run.metrics["first_collision_tick"]
    speeds = torch.stack([h["path"][:, :, :, 3] for h in run.hist])        # [steps, B, 1, tps + 1]
    status = torch.stack([h["status"] for h in run.hist])
    print("stop scene, governed: first collision ticks", first.tolist(), "min gap",
          run.metrics["min_gap_obs"].flatten().tolist())
    print("  speed at the end of each step", speeds[:, :, 0, -1].T.tolist())
    print("  accel_cmd", torch.stack([h["accel_cmd"][:, 0] for h in run.hist]).T.tolist())
    print("  k_conf", torch.stack([h["gov_k_conf"][:, 0] for h in run.hist]).T.tolist())
    print("  status words", sorted(set(status.flatten().tolist())))
    assert (first < 0).all()
    assert (speeds >= -1e-12).all()
    assert (speeds[-1, :, :, -1].abs() <= 1e-9).all()
    assert ((status & 0xFF) != LB.ST_NUMERIC).all()
    # the command of step i is the plant's x[4] throughout step i + 1
    for i in range(len(run.hist) - 1):
        acc = run.hist[i + 1]["path"][:, :, :, 4]
        assert (acc == run.hist[i]["accel_cmd"][:, :, None]).all(), i
    # it braked at once (the first plan's first point is a conflict) and then held still
    assert (run.hist[0]["gov_k_conf"] == 0).all()
    assert (run.hist[0]["accel_cmd"] == -ro.kw["a_brake"]).all()
    assert set(run.hist[0]) - set(ro.runs["free"].hist[0]) == {"accel_cmd", "gov_k_conf", "gov_clear"}


def test_rollout_records_what_the_step_gives(stop_runs, gpu):
    ro, sc = stop_runs, stop_runs.sc
    gov = GOV.rows(ro.B, 1, device=gpu, **ro.kw)
    dreq = GOV.required(sc, device=gpu)
    for i, rec in enumerate(ro.runs["governed"].hist):
        a, k, c = GOV.step(gov, rec["x0"], rec["traj"], rec["obst"], None, *dreq, sc.dt,
                           sc.delay_u)
        assert _beq(a, rec["accel_cmd"]) and torch.equal(k, rec["gov_k_conf"]) \
            and _beq(c, rec["gov_clear"]), i
        # the plan starts from the acceleration in force: the previous step's command
        if i:
            prev = ro.runs["governed"].hist[i - 1]["accel_cmd"]
            assert (rec["x0"][:, :, 4] == prev).all(), i


def test_with_a_measurement_delay_the_plan_starts_from_the_command_in_force(gpu):
    """ticks_delay_x = 10: the measured state is 0.1 s old and carries the acceleration of the
    previous step; column 4 of the delay compensation's input is the command in force at the
    step's first tick instead, here under a noisy sensor and the estimator as well."""
    from scpqp import estimator as EST
    from scpqp import sensing as SE
    from scpqp.rollout import ClosedLoopBatch
    sc, x_init, kw = GC.stop_scene(delay_x=0.1)
    assert sc.ticks_delay_x == 10
    B = GC.STOP_B
    rows = OB.nominal(sc, B, device=gpu)
    gov = GOV.rows(B, 1, device=gpu, **kw)
    srows = SE.nominal(B, 1, device=gpu)
    srows[..., SE.FIELDS.index("sig_pos")] = 0.02
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    for extra in (dict(), dict(sensing=srows, sense_seed=3, estimator=EST.matched(srows))):
        cl.reset(x_init, obstacles=rows, governor=gov, **extra)
        hist = cl.run(6)
        for i in range(1, 6):
            prev = hist[i - 1]["accel_cmd"]
            assert (hist[i]["x0"][:, :, 4] == prev).all(), i
            assert (hist[i]["path"][:, :, :, 4] == prev[:, :, None]).all(), i
            # what was measured still carries the acceleration of the step before
            old = hist[i - 1]["path"][:, :, sc.ticks_per_sim - sc.ticks_delay_x, 4]
            if i == 1:
                assert (old == 0).all() and (prev < 0).all()
        assert (hist[0]["accel_cmd"] == -kw["a_brake"]).all()
        status = torch.stack([h["status"] for h in hist])
        assert ((status & 0xFF) != LB.ST_NUMERIC).all()
        assert (cl.metrics()["first_collision_tick"] < 0).all()
    cl.close()
