"""The state estimator on the device (include/scpqp_estimator.h) against the CPU mirror
(tests/estimator_mirror.py): six filter steps with mixed rows, the diagonal known answer, the
off and bad-row rules, the independence of the lanes, recovery after trouble, the statistics of
the innovations, and the rollout.

Shapes (B, n_veh, n_span): (2, 3, 4), no power of two; (43, 6, 8): 258 (b, v) lanes, two
workgroups of 256 with a ragged tail; (1, 1, 0), a step without prediction.  tick = 0.01 s and
h_max = PL.H_MAX.

Tolerance of the device against the mirror, one relative figure for the three outputs:
|dx_i| <= TOL max(1, |x_i|), |dP_ij| <= TOL sqrt(P_ii P_jj), |dnis| <= TOL max(1, nis), and
identical NaN patterns.  The device's tan, atan, sin and cos differ from libm's by a few ulp,
6 steps x 8 ticks x 4 RK4 steps accumulate them, and the device's sums are fused and ordered
differently from numpy's dense products.  Measured on an MI355X against the mirror (the test
prints the figure; DESIGN §7, "State estimator"): the largest ratio is MEASURED_RATIO below,
at (43, 6, 8).  TOL is 16 times that, rounded up to a power of two.

The lost-sensor rollout prints the ratio of the estimate's position error to the held
measurement's; it asserts only "smaller".  Measured on an MI355X: the estimate is
0, 1.6e-4 and 2.8e-4 m off after one, two and three lost steps, the held measurement 1.60,
3.19 and 4.79 m; the largest ratio is 5.9e-5.
"""
import math
import types

import numpy as np
import pytest
import torch

import estimator_mirror as EM
import sensing_mirror as SM
from oracle import scp_reference as R
from scpqp import estimator as EST
from scpqp import plant as PL

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 4), (43, 6, 8), (1, 1, 0)]            # (B, n_veh, n_span)
TICK = 0.01
N_STEPS = 6
MEASURED_RATIO = 3.248e-13        # (2, 3, 4): 2.3e-15; (1, 1, 0): 3.2e-16
TOL = 2.0 ** -37                  # 16 * 3.248e-13 = 5.2e-12 <= 2^-37 = 7.3e-12


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _beq(a, b):
    """Bitwise equality of float64 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _geometry(V):
    lf = [0.34 + 0.01 * v for v in range(V)]
    lr = [0.34 - 0.005 * v for v in range(V)]
    return lf, lr


def _case(B, V, n_span, seed=7):
    """Rows, measurements, commands and the delivery pattern of N_STEPS steps.  Lane g:
    every seventh is off, g % 5 == 1 has Q = 0; delivery cycles with g % 3 through always,
    never after the first step, and a seeded pattern (whose first step may be lost too)."""
    rng = np.random.default_rng(seed + 100 * B + V)
    n = B * V
    g = np.arange(n).reshape(B, V)
    rows = np.empty((B, V, 8))
    rows[..., 0] = rng.uniform(0.02, 0.1, (B, V))
    rows[..., 1] = rng.uniform(0.002, 0.02, (B, V))
    rows[..., 2] = rng.uniform(0.05, 0.2, (B, V))
    rows[..., 3] = rng.uniform(0.001, 0.01, (B, V))
    rows[..., 4:] = rng.uniform(0.0, 1.0, (B, V, 4)) * np.array([0.05, 0.02, 0.1, 0.02])
    rows[g % 5 == 1, 4:] = 0.0
    rows[g % 7 == 3] = 0.0
    base = np.empty((B, V, 6))
    base[..., 0], base[..., 1] = g * 1.5, -g * 0.5
    base[..., 2] = rng.uniform(-3.0, 3.0, (B, V))
    base[..., 3] = rng.uniform(1.0, 8.0, (B, V))
    base[..., 4] = rng.uniform(-0.5, 0.5, (B, V))
    base[..., 5] = rng.uniform(-0.2, 0.2, (B, V))
    sig = np.array([0.05, 0.05, 0.01, 0.1, 0.0, 0.005])
    meas, us, dl = [], [], []
    for s in range(N_STEPS):
        drift = np.zeros((B, V, 6))
        adv = s * n_span * TICK * base[..., 3]
        drift[..., 0], drift[..., 1] = adv * np.cos(base[..., 2]), adv * np.sin(base[..., 2])
        meas.append(base + drift + rng.standard_normal((B, V, 6)) * sig)
        us.append(rng.uniform(-0.2, 0.2, (B, V, n_span)))
        d = np.ones((B, V), dtype=np.int32)
        d[(g % 3 == 1) & (s > 0)] = 0
        pat = rng.integers(0, 2, (B, V)).astype(np.int32)
        d[g % 3 == 2] = pat[g % 3 == 2]
        dl.append(d)
    return rows, meas, us, dl


def _ratio(dev_x, dev_P, dev_nis, mir_x, mir_P, mir_nis):
    """The largest of the three relative differences; NaN patterns must be identical."""
    for d, m in ((dev_x, mir_x), (dev_P, mir_P), (dev_nis, mir_nis)):
        assert (np.isnan(d) == np.isnan(m)).all()
    worst = 0.0
    ok = ~np.isnan(mir_x)
    if ok.any():
        worst = max(worst, float((np.abs(dev_x - mir_x)[ok] / np.maximum(1.0, np.abs(mir_x[ok]))).max()))
    dg = np.sqrt(np.abs(np.einsum("...ii->...i", mir_P)))
    scale = dg[..., :, None] * dg[..., None, :]
    ok = ~np.isnan(mir_P) & (scale > 0)
    if ok.any():
        worst = max(worst, float((np.abs(dev_P - mir_P)[ok] / scale[ok]).max()))
    ok = ~np.isnan(mir_nis)
    if ok.any():
        worst = max(worst, float((np.abs(dev_nis - mir_nis)[ok] / np.maximum(1.0, mir_nis[ok])).max()))
    return worst


# ---------------------------------------------------------------------------
# 1. device against mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,n_span", SHAPES)
def test_six_steps_match_the_mirror(gpu, B, V, n_span):
    lf, lr = _geometry(V)
    P = PL.plant_params(lf, lr)
    rows, meas, us, dl = _case(B, V, n_span)
    x_d, cov_d = EST.alloc(B, V, gpu)
    x_m, cov_m = np.full((B, V, 6), np.nan), np.zeros((B, V, 5, 5))
    rows_d = _dev(rows, gpu)
    worst = 0.0
    seen_update = seen_lost = seen_uninit = False
    for s in range(N_STEPS):
        u = None if n_span == 0 else _dev(us[s], gpu)
        nis_d = EST.step(P, u, TICK, _dev(meas[s], gpu), _dev(dl[s], gpu, torch.int32), rows_d,
                         x_d, cov_d)
        nis_m = EM.step(lf, lr, TICK, None if n_span == 0 else us[s], meas[s], dl[s], rows, x_m,
                        cov_m)
        on = (rows != 0).any(axis=2)
        # the off lanes: the measurement bit for bit, cov as it was allocated
        assert (x_d.cpu().numpy()[~on].view(np.int64) == meas[s][~on].view(np.int64)).all()
        assert (cov_d.cpu().numpy()[~on] == 0).all()
        worst = max(worst, _ratio(x_d.cpu().numpy()[on], cov_d.cpu().numpy()[on],
                                  nis_d.cpu().numpy()[on], x_m[on], cov_m[on], nis_m[on]))
        seen_update |= bool(np.isfinite(nis_m).any())
        seen_lost |= bool((on & (dl[s] == 0) & ~np.isnan(x_m[..., 0])).any())
        seen_uninit |= bool((on & np.isnan(x_m[..., 0])).any())
    print(f"({B}, {V}, {n_span}): largest device - mirror ratio {worst:.3e} (TOL {TOL:.3e})")
    assert seen_update
    if B * V > 6:
        assert seen_lost and seen_uninit          # every path of the lane was taken
    assert worst <= TOL


# ---------------------------------------------------------------------------
# 2. known answer, off rows, NULL delivered
# ---------------------------------------------------------------------------
def test_two_measurements_average_on_the_device(gpu):
    B, V = 3, 2
    lf, lr = _geometry(V)
    P = PL.plant_params(lf, lr)
    rng = np.random.default_rng(3)
    rows = EST.rows(B, V, r_pos=rng.uniform(0.01, 0.1, (B, V)), r_heading=0.01, r_speed=0.1,
                    r_steer=rng.uniform(0.001, 0.01, (B, V)), device=gpu)
    m1 = rng.uniform(-3, 3, (B, V, 6))
    m2 = m1 + rng.uniform(-0.1, 0.1, (B, V, 6))
    x, cov = EST.alloc(B, V, gpu)
    nis = EST.step(P, None, TICK, _dev(m1, gpu), None, rows, x, cov)
    assert _beq(x, _dev(m1, gpu)) and torch.isnan(nis).all()
    r = np.stack([EM.r_diag(row) for row in rows.cpu().numpy().reshape(-1, 8)]).reshape(B, V, 5)
    assert (cov.cpu().numpy() == np.einsum("...i,ij->...ij", r, np.eye(5))).all()
    # NULL delivered and an array of ones are the same call
    x1, cov1 = x.clone(), cov.clone()
    nis1 = EST.step(P, None, TICK, _dev(m2, gpu), torch.ones((B, V), dtype=torch.int32, device=gpu),
                    rows, x1, cov1)
    nis = EST.step(P, None, TICK, _dev(m2, gpu), None, rows, x, cov)
    assert _beq(x, x1) and _beq(cov, cov1) and _beq(nis, nis1)
    xh, ch, nh = x.cpu().numpy(), cov.cpu().numpy(), nis.cpu().numpy()
    want = 0.5 * (m1 + m2)
    assert (np.abs(xh - want)[..., EM.IDX] <= 1e-13 * np.maximum(1.0, np.abs(want[..., EM.IDX]))).all()
    assert (xh[..., 4] == m2[..., 4]).all()
    diag = np.einsum("...ii->...i", ch)
    assert (np.abs(diag - r / 2) <= 1e-13 * r / 2).all()
    assert (ch - np.einsum("...i,ij->...ij", diag, np.eye(5)) == 0).all()
    want_nis = ((m2 - m1)[..., EM.IDX] ** 2 / (2 * r)).sum(-1)
    assert (np.abs(nh - want_nis) <= 1e-13 * want_nis).all()


def test_off_rows_copy_the_measurement_and_leave_cov(gpu):
    B, V, n_span = 43, 6, 8
    P = PL.plant_params(*_geometry(V))
    rng = np.random.default_rng(5)
    m = rng.standard_normal((B, V, 6))
    m[0, 0, 1], m[1, 2, 3], m[2, 1, 0] = -0.0, math.nan, math.inf     # passed through as they are
    x = _dev(rng.standard_normal((B, V, 6)), gpu)
    cov0 = _dev(rng.standard_normal((B, V, 5, 5)), gpu)
    cov = cov0.clone()
    u = _dev(rng.uniform(-0.2, 0.2, (B, V, n_span)), gpu)
    dl = _dev(rng.integers(0, 2, (B, V)), gpu, torch.int32)
    nis = EST.step(P, u, TICK, _dev(m, gpu), dl, EST.off(B, V, gpu), x, cov)
    assert _beq(x, _dev(m, gpu)) and _beq(cov, cov0) and torch.isnan(nis).all()


# ---------------------------------------------------------------------------
# 3. split batch, lane independence, bad rows, recovery
# ---------------------------------------------------------------------------
def _run(P, rows, meas, us, dl, gpu, lo=0, hi=None, steps=3, state=None):
    B, V = rows[lo:hi].shape[:2]
    x, cov = EST.alloc(B, V, gpu) if state is None else (state[0].clone(), state[1].clone())
    out = []
    rows_d = _dev(rows[lo:hi], gpu)
    for s in range(steps):
        nis = EST.step(P, _dev(us[s][lo:hi], gpu), TICK, _dev(meas[s][lo:hi], gpu),
                       _dev(dl[s][lo:hi], gpu, torch.int32), rows_d, x, cov)
        out.append((x.clone(), cov.clone(), nis.clone()))
    return out


def test_a_split_batch_gives_what_the_whole_gives(gpu):
    B, V, n_span = 43, 6, 8
    P = PL.plant_params(*_geometry(V))
    case = _case(B, V, n_span)
    whole = _run(P, *case, gpu)
    a, b = _run(P, *case, gpu, 0, 20), _run(P, *case, gpu, 20, B)
    for s, w in enumerate(whole):
        for k in range(3):
            assert _beq(w[k], torch.cat([a[s][k], b[s][k]])), (s, k)


BAD = [(0, math.nan), (6, math.inf), (1, -1e-3), (7, -1e-300), (2, 0.0), (0, 0.0)]


def test_changing_the_last_row_changes_only_its_lane(gpu):
    B, V, n_span = 43, 6, 8
    P = PL.plant_params(*_geometry(V))
    rows, meas, us, dl = _case(B, V, n_span)
    rows[-1, -1] = [0.05, 0.01, 0.1, 0.005, 0.02, 0.01, 0.05, 0.01]
    for d in dl:
        d[-1, -1] = 1
    base = _run(P, rows, meas, us, dl, gpu)
    other = rows.copy()
    other[-1, -1, 0] = 0.08
    got = _run(P, other, meas, us, dl, gpu)
    for s in range(len(base)):
        for k in range(3):
            w, g = base[s][k].flatten(0, 1), got[s][k].flatten(0, 1)
            assert _beq(w[:-1], g[:-1]), (s, k)
        if s:
            assert not _beq(base[s][0][-1, -1], got[s][0][-1, -1])
    # every kind of bad row: NaN in its own lane, bitwise the same everywhere else
    for f, val in BAD:
        bad = rows.copy()
        bad[-1, -1, f] = val
        assert EM.is_bad_row(bad[-1, -1])
        got = _run(P, bad, meas, us, dl, gpu)
        for s in range(len(base)):
            for k in range(3):
                w, g = base[s][k].flatten(0, 1), got[s][k].flatten(0, 1)
                assert _beq(w[:-1], g[:-1]), (f, s, k)
                assert torch.isnan(g[-1]).all(), (f, s, k)


def test_a_lane_turned_nan_recovers_on_its_next_measurement(gpu):
    B, V, n_span = 2, 3, 4
    lf, lr = _geometry(V)
    P = PL.plant_params(lf, lr)
    rows = EST.rows(B, V, device=gpu)
    rng = np.random.default_rng(9)
    m = _dev(rng.uniform(-1, 1, (B, V, 6)) + np.array([0, 0, 0, 4, 0, 0]), gpu)
    u = _dev(rng.uniform(-0.2, 0.2, (B, V, n_span)), gpu)
    x, cov = EST.alloc(B, V, gpu)
    EST.step(P, None, TICK, m, None, rows, x, cov)
    good = (x.clone(), cov.clone())
    cov[1, 2] = -torch.eye(5, dtype=torch.float64, device=gpu)       # no Cholesky of S
    x[0, 1, 3] = math.inf                                              # a non-finite prediction
    nis = EST.step(P, u, TICK, m, None, rows, x, cov)
    for b, v in ((1, 2), (0, 1)):
        assert torch.isnan(x[b, v]).all() and torch.isnan(cov[b, v]).all() and math.isnan(nis[b, v])
    ref = (good[0].clone(), good[1].clone())
    nis_ref = EST.step(P, u, TICK, m, None, rows, *ref)
    keep = torch.ones((B, V), dtype=torch.bool, device=gpu)
    keep[1, 2] = keep[0, 1] = False
    assert _beq(x[keep], ref[0][keep]) and _beq(cov[keep], ref[1][keep]) and _beq(nis[keep], nis_ref[keep])
    # lost: stays NaN; delivered: the lane initialises itself again
    lost = torch.zeros((B, V), dtype=torch.int32, device=gpu)
    nis = EST.step(P, u, TICK, m, lost, rows, x, cov)
    assert torch.isnan(x[1, 2]).all() and torch.isnan(x[0, 1]).all()
    nis = EST.step(P, u, TICK, m, None, rows, x, cov)
    r = EM.r_diag(rows[0, 0].cpu().numpy())
    for b, v in ((1, 2), (0, 1)):
        assert _beq(x[b, v], m[b, v]) and math.isnan(nis[b, v])
        assert (cov[b, v].cpu().numpy() == np.diag(r)).all()


# ---------------------------------------------------------------------------
# 4. statistics: the CPU consistency inputs on the device
# ---------------------------------------------------------------------------
def test_innovations_are_consistent_on_the_device(gpu):
    B, V = 250, 6
    N = B * V
    truth, u, meas, rows = EM.consistency_inputs(N)
    P = PL.plant_params([EM.CONS_LF] * V, [EM.CONS_LR] * V)
    rows_d = _dev(rows.reshape(B, V, 8), gpu)
    x, cov = EST.alloc(B, V, gpu)
    every = []
    for s in range(EM.CONS_STEPS + 1):
        us = None if s == 0 else _dev(np.broadcast_to(u[s - 1], (B, V, EM.CONS_SPAN)), gpu)
        nis = EST.step(P, us, EM.CONS_TICK, _dev(meas[s].reshape(B, V, 6), gpu), None, rows_d, x, cov)
        if s:
            every.append(nis.cpu().numpy())
    every = np.array(every)
    assert np.isfinite(every).all() and every.size == 9000
    mean, bound, rms_est, rms_meas = EM.consistency_verdict(
        every, x.cpu().numpy().reshape(N, 6), truth[-1], meas[-1])
    print(f"mean NIS {mean:.3f} (|mean - 5| <= {bound:.3f}); RMS position error {rms_est:.4f} m "
          f"of the estimate, {rms_meas:.4f} m of the measurement")
    assert abs(mean - 5.0) <= bound
    assert rms_est < rms_meas


# ---------------------------------------------------------------------------
# 5. rollout: circle, 2 vehicles, Hp 10, B = 4, 3 steps, noise seed 1 (the small fixture of
#    tests/test_gpu_sensing.py)
# ---------------------------------------------------------------------------
STEPS = 3
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "u_tick")
SENSE_SEED = 31


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(cl, keys=KEYS):
    return types.SimpleNamespace(
        hist=[{k: h[k].clone() for k in keys + ("x_meas", "delivered", "x_est", "nis") if k in h}
              for h in cl.history], metrics=cl.metrics(), control=cl.control.clone())


def _circle_rows(sc, B):
    rows = SM.nominal_rows(B, sc.nVeh)
    rows[..., SM.SIG_POS] = 0.05
    rows[1, :, SM.P_DROP] = 1.0
    rows[2, :, SM.LAG] = sc.ticks_per_sim - sc.ticks_delay_x
    return rows


def _est_rows(B, V):
    rows = EST.rows(B, V, r_pos=0.05, r_heading=1e-3, r_speed=1e-3, r_steer=1e-3,
                    device="cpu").numpy()
    rows[3, 0] = 0.0                   # one lane without a filter among lanes with one
    return rows


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(2, Hp=10)
    B = 4
    x_init = _x_init(sc, B)
    rows = _circle_rows(sc, B)
    est = _est_rows(B, sc.nVeh)
    off = np.zeros((B, sc.nVeh, 8))
    sense = dict(sensing=rows, sense_seed=SENSE_SEED)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("plain", {}), ("plain_none", dict(estimator=None)),
                     ("plain_off", dict(estimator=off)), ("plain_est", dict(estimator=est)),
                     ("noisy", sense), ("noisy_off", dict(estimator=_dev(off, gpu), **sense)),
                     ("noisy_est", dict(estimator=est, **sense))):
        cl.reset(x_init, seed=1, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, sensing=rows[o:o + 2],
                   sense_seed=SENSE_SEED, estimator=est[o:o + 2])
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, rows=rows, est=est, runs=runs)
    cl.close()


@pytest.mark.parametrize("base,same", [("plain", "plain_none"), ("plain", "plain_off"),
                                       ("noisy", "noisy_off")])
def test_rollout_without_a_filter_is_the_rollout_of_before(rollouts, base, same):
    a, b = rollouts.runs[base], rollouts.runs[same]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert "x_est" not in a.hist[i] and "nis" not in a.hist[i]
        for k in KEYS + (("x_meas", "delivered") if base == "noisy" else ()):
            assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
        if same.endswith("off"):
            assert _beq(b.hist[i]["x_est"], b.hist[i]["x_meas"]), i
            assert torch.isnan(b.hist[i]["nis"]).all()
        else:
            assert "x_est" not in b.hist[i]
    assert _eq(a.control.view(torch.int64), b.control.view(torch.int64))
    for k, v in a.metrics.items():
        assert _eq(v, b.metrics[k]), k


@pytest.mark.parametrize("name", ["plain_est", "noisy_est"])
def test_rollout_records_what_step_gives(rollouts, gpu, name):
    ro, sc, cl = rollouts, rollouts.sc, rollouts.cl
    run = ro.runs[name]
    tps, tdx, total = sc.ticks_per_sim, sc.ticks_delay_x, sc.ticks_total
    rows = _dev(ro.est, gpu)
    x, cov = EST.alloc(ro.B, sc.nVeh, gpu)
    horizon = sc.delay_x + sc.dt + sc.delay_u
    g0 = 0
    for i, rec in enumerate(run.hist):
        g1 = max(0, i * tps - tdx)
        u_span = None
        if g1 > g0:
            idx = [min(total, j + 1) for j in range(g0 + 1, g1 + 1)]
            u_span = run.control[:, :, torch.as_tensor(idx, device=gpu)].contiguous()
            assert not torch.isnan(u_span).any()             # every command was already issued
        nis = EST.step(cl.params, u_span, sc.tick_length, rec["x_meas"], rec.get("delivered"), rows,
                       x, cov, h_max=cl.h_max)
        g0 = g1
        assert _beq(rec["x_est"], x) and _beq(rec["nis"], nis), i
        # the estimate, not the measurement, is what the delay compensation starts from
        x0, _ = PL.delay_compensate(cl.params, rec["x_est"], rec["u0"], horizon, h_max=cl.h_max,
                                    device=gpu, rng=PL.NoiseStream(1, PL.SIGMA_NOISE, i, 0))
        assert _eq(rec["x0"], x0), i
        # the lane without a filter keeps its measurement
        assert _beq(rec["x_est"][3, 0], rec["x_meas"][3, 0])
    # x_meas stays what the sensor gave
    if name == "noisy_est":
        assert _beq(run.hist[0]["x_meas"], ro.runs["noisy"].hist[0]["x_meas"])
    last = run.hist[-1]
    assert torch.isfinite(last["nis"][0]).all() and not _beq(last["x_est"][0], last["x_meas"][0])


def test_rollout_with_an_estimator_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["noisy_est"].hist):
        for k in KEYS + ("x_meas", "delivered", "x_est", "nis"):
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            if whole[k].dtype == torch.float64:
                assert _beq(whole[k], parts), (i, k)
            else:
                assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["noisy_est"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_reset_refuses_a_bad_estimator_before_anything_is_launched(rollouts, gpu):
    ro, cl = rollouts, rollouts.cl
    cl.reset(ro.x_init, seed=1, estimator=ro.est)
    cl.run(1)
    n_hist, i = len(cl.history), cl.i
    state, rows_before = cl.state.clone(), cl.est_rows.clone()
    x_before, cov_before = cl.est_x.clone(), cl.est_cov.clone()
    good = ro.est
    neg, zero_r, nan = good.copy(), good.copy(), good.copy()
    neg[2, 1, 6] = -0.1
    zero_r[1, 0, 1] = 0.0
    nan[0, 0, 4] = math.nan
    for bad in (good[:2], good[:, :1], good[..., :7], neg, torch.as_tensor(neg), zero_r, nan):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, estimator=bad)
    with pytest.raises(ValueError, match=r"rows\[2, 1\]: q_speed must be >= 0"):
        cl.reset(ro.x_init, seed=1, estimator=neg)
    with pytest.raises(ValueError, match=r"rows\[1, 0\]: r_heading must be > 0"):
        cl.reset(ro.x_init, seed=1, estimator=zero_r)
    assert len(cl.history) == n_hist and cl.i == i           # the refused resets changed nothing
    assert _eq(cl.state, state) and _eq(cl.est_rows, rows_before)
    assert _beq(cl.est_x, x_before) and _beq(cl.est_cov, cov_before)


# ---------------------------------------------------------------------------
# 6. a lost sensor: the estimate against the held measurement
# ---------------------------------------------------------------------------
def test_with_a_lost_sensor_the_estimate_beats_the_held_measurement(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(2, Hp=10)
    B, steps = 2, 4
    tps, tdx = sc.ticks_per_sim, sc.ticks_delay_x
    sense = SM.nominal_rows(B, sc.nVeh)
    sense[..., SM.P_DROP] = 1.0                   # exact sigmas; every step after the first is lost
    est = EST.matched(sense, device=gpu)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True)
    cl.reset(_x_init(sc, B), sensing=sense, sense_seed=SENSE_SEED, estimator=est)
    hist = cl.run(steps)
    worst = 0.0
    for i in range(1, steps):
        rec = hist[i]
        assert (rec["delivered"] == 0).all()
        assert _beq(rec["x_meas"], hist[0]["x_meas"])                    # held since step 0
        true = hist[i - 1]["path"][:, :, tps - min(tdx, i * tps), 0:2]  # the realised state there
        e_est = (rec["x_est"][..., 0:2] - true).norm(dim=-1)
        e_held = (rec["x_meas"][..., 0:2] - true).norm(dim=-1)
        print(f"step {i}: position error of the estimate {e_est.max().item():.3e} m, of the held "
              f"measurement {e_held.min().item():.3f} m, ratio {(e_est / e_held).max().item():.3e}")
        worst = max(worst, (e_est / e_held).max().item())
        assert (e_est < e_held).all(), i
    print(f"lost sensor: largest estimate / held position-error ratio {worst:.3e}")
    cl.close()
