"""The sensing truth on the device (include/scpqp_sensing.h): the measurement and the sensed
obstacle prediction against the CPU mirror (tests/sensing_mirror.py), the nominal and bad-row
rules, the independence of the lanes, the sampler, the statistics of the draws, and the rollout.

Shapes (B, n_veh, n_ticks): (2, 3, 4), no power of two; (43, 6, 40): 258 (b, v) lanes, two
workgroups of 256 with a ragged tail; (1, 1, 0), the step-0 form.  Obstacle shapes
(B, n_obst, hp) are (2, 3, 4) and (5, 22, 10), as in tests/test_gpu_obstacles.py.

Tolerance of a value with noise: 64 * 2^-52 * 10 * sigma (the normal-draw tolerance of
tests/test_gpu_noise.py::test_raw_draws_match_the_mirror, scaled by the sigma) plus one
rounding of the value, 2^-53 |value| (half a unit in its last place).  Values without noise
are compared bitwise.  The sensed obstacle prediction propagates the three draws through the
straight line  step * cos h + x,  step = T s,  T = (k + 1) dt + lead:  the draw tolerance
times (sig_pos + T |s| sig_heading + T sig_speed), plus the 1e-12 m that
tests/test_gpu_obstacles.py allows the pose and the line themselves.

Measured on an MI355X (the tests print the figures; DESIGN §7, "Sensing truth"): the largest
|device - mirror| / sigma of a noisy field is 6.6e-15 over six epochs at (43, 6, 40) and 0 at
the two small shapes; the sensed prediction differs from the mirror by 1.4e-14 m at
(5, 22, 10); the sampler's NORMAL fields by 1.4e-17 (sig_pos) and 6.9e-18 (bias_heading).
"""
import math
import types

import numpy as np
import pytest
import torch

import obstacle_mirror as OM
import sensing_mirror as SM
from oracle import scp_reference as R
from scpqp import obstacles as OB
from scpqp import plant as PL
from scpqp import sensing as SE

pytestmark = pytest.mark.gpu

ATOL = 64 * 2.0 ** -52 * 10               # of one standard-normal draw
SHAPES = [(2, 3, 4), (43, 6, 40), (1, 1, 0)]          # (B, n_veh, n_ticks)
OSHAPES = [(2, 3, 4), (5, 22, 10)]                    # (B, n_obst, hp)
T_MEAS, LEAD, DT = 1.6, 0.43, 0.4
SEED = 0x123456789ABCDEF


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _dev(a, gpu, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def _k_meas(n_ticks):
    return max(0, n_ticks - 3)


def _path(B, V, n_ticks, seed=3):
    """States inside +-50 m, headings over the circle, speeds 0..10 m/s, steering +-0.3 rad."""
    rng = np.random.default_rng(seed)
    K = n_ticks + 1
    x = rng.uniform(-50, 50, (B, V, K, 6))
    x[..., 2] = rng.uniform(-math.pi, math.pi, (B, V, K))
    x[..., 3] = rng.uniform(0, 10, (B, V, K))
    x[..., 5] = rng.uniform(-0.3, 0.3, (B, V, K))
    return x


def _noisy_rows(B, V):
    """Per lane its own sigmas (one field in four exactly 0), offset and scale; P_DROP cycles
    through 0, 1 and 0.5 and LAG through 0, 3 and 100 (beyond every k_meas used here); every
    seventh lane is nominal."""
    rng = np.random.default_rng(8)
    r = np.zeros((B, V, 8))
    r[..., 0] = rng.uniform(0.03, 0.08, (B, V))
    r[..., 1] = rng.uniform(0.005, 0.02, (B, V))
    r[..., 2] = rng.uniform(0.05, 0.2, (B, V))
    r[..., 3] = rng.uniform(0.001, 0.004, (B, V))
    n = np.arange(B * V).reshape(B, V)
    for f in range(4):
        r[..., f] = np.where(n % 4 == f, 0.0, r[..., f])
    r[..., 4] = rng.uniform(-0.03, 0.03, (B, V))
    r[..., 5] = rng.uniform(0.95, 1.05, (B, V))
    r[..., 6] = np.choose(n % 3, [0.0, 1.0, 0.5])
    r[..., 7] = np.choose((n // 3) % 3, [0.0, 3.0, 100.0])
    r[n % 7 == 5] = SM.NOMINAL
    return r


def _obstacle_rows(B, nO, seed=5):
    """Turning obstacle rows inside +-60 m (those of tests/test_gpu_obstacles.py): headings over
    the circle, speeds 0..3 m/s, turn rates +-0.5 rad/s, one in eight exactly straight."""
    rng = np.random.default_rng(seed)
    r = np.zeros((B, nO, 7))
    r[..., 0:2] = rng.uniform(-60, 60, (B, nO, 2))
    r[..., 2] = rng.uniform(-math.pi, math.pi, (B, nO))
    r[..., 3] = rng.uniform(0.0, 3.0, (B, nO))
    r[..., 4] = rng.uniform(0.5, 4.0, (B, nO))
    r[..., 5] = rng.uniform(0.5, 2.0, (B, nO))
    r[..., 6] = rng.uniform(-0.5, 0.5, (B, nO))
    n = np.arange(B * nO).reshape(B, nO)
    r[..., 6] = np.where(n % 8 == 3, 1e-5, np.where(n % 8 == 6, 0.0, r[..., 6]))
    return r


def _held(B, V, gpu, value=math.nan):
    return torch.full((B, V, 6), value, dtype=torch.float64, device=gpu)


def _measure(x, k, rows, seed, epoch, b_off, held, gpu):
    """The device's measurement and delivered flags as numpy arrays; held: a device tensor."""
    deliv = torch.full(tuple(rows.shape[:2]), -7, dtype=torch.int32, device=gpu)
    out = SE.measure(_dev(x, gpu), k, _dev(rows, gpu), seed, epoch, b_off, held, deliv)
    return out, deliv


def _value_tol(want, sigma):
    return ATOL * sigma + 2.0 ** -53 * np.abs(want)


# ---------------------------------------------------------------------------
# 1. nominal rows are bitwise copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B, V, n_ticks", SHAPES)
def test_nominal_rows_copy_the_measured_tick_bitwise(gpu, B, V, n_ticks):
    x = _path(B, V, n_ticks)
    k = _k_meas(n_ticks)
    x[:, :, k, 4] = -0.0                                   # the sign of a zero survives
    x[0, 0, k, 0] = -0.0
    rows = SE.nominal(B, V, device=gpu)
    assert np.array_equal(rows.cpu().numpy(), SM.nominal_rows(B, V))
    held = _held(B, V, gpu)
    out, deliv = _measure(x, k, rows.cpu().numpy(), SEED, 4, 0, held, gpu)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(x[:, :, k]))
    assert np.signbit(out.cpu().numpy()[:, :, 4]).all()
    assert np.array_equal(_bits(held.cpu().numpy()), _bits(x[:, :, k]))
    assert deliv.cpu().numpy().tolist() == np.ones((B, V), int).tolist()
    # a state [B, V, 6] is the step-0 form of the same call
    if n_ticks == 0:
        again = SE.measure(_dev(x[:, :, 0], gpu), 0, rows, SEED, 4, 0, _held(B, V, gpu))
        assert _eq(again, out)


@pytest.mark.parametrize("B, nO, hp", OSHAPES)
def test_zero_osense_rows_are_the_exact_prediction_bitwise(gpu, B, nO, hp):
    rows = _dev(_obstacle_rows(B, nO), gpu)
    zero = torch.zeros((B, nO, 3), dtype=torch.float64, device=gpu)
    got = SE.predict_sensed(rows, zero, SEED, 2, 0, T_MEAS, LEAD, DT, hp)
    assert _eq(got, OB.predict(rows, T_MEAS, LEAD, DT, hp)) and not torch.isnan(got).any()
    assert tuple(SE.predict_sensed(rows[:0], zero[:0], SEED, 2, 0, T_MEAS, LEAD, DT, hp).shape) \
        == (0, nO, 2, hp)


# ---------------------------------------------------------------------------
# 2. noisy rows against the mirror
# ---------------------------------------------------------------------------
SIGMA_OF_STATE = {0: SM.SIG_POS, 1: SM.SIG_POS, 2: SM.SIG_HEADING, 3: SM.SIG_SPEED, 5: SM.SIG_STEER}


@pytest.mark.parametrize("B, V, n_ticks", SHAPES)
def test_noisy_rows_match_the_mirror_over_six_epochs(gpu, B, V, n_ticks):
    rows = _noisy_rows(B, V)
    assert not any(SM.bad_row(r) for r in rows.reshape(-1, 8))
    k, b_off = _k_meas(n_ticks), 1000
    held_d, held_m = _held(B, V, gpu), np.full((B, V, 6), np.nan)
    worst, lost_seen = 0.0, 0
    sig = np.stack([rows[..., SIGMA_OF_STATE.get(j, 0)] if j != 4 else np.zeros((B, V))
                    for j in range(6)], axis=-1)              # [B, V, 6] the sigma of each state
    for epoch in range(6):
        x = _path(B, V, n_ticks, seed=100 + epoch)
        before = held_d.clone()
        out, deliv = _measure(x, k, rows, SEED, epoch, b_off, held_d, gpu)
        want, want_deliv = SM.measure(x, k, rows, SEED, epoch, b_off, held_m)
        got, d = out.cpu().numpy(), deliv.cpu().numpy()
        assert np.array_equal(d, want_deliv), epoch           # u2 is exact in fp64
        if epoch == 0:
            assert d.all()                                    # NaN in x_held: always delivered
        lost = d == 0
        lost_seen += int(lost.sum())
        # a lost measurement is the held one, which stays; a delivered one becomes the held one
        assert _eq(out[torch.as_tensor(lost, device=gpu)], before[torch.as_tensor(lost, device=gpu)])
        assert _eq(held_d, torch.where(torch.as_tensor(lost, device=gpu)[..., None], before, out))
        exact = sig == 0.0
        assert np.array_equal(_bits(got)[exact], _bits(want)[exact]), epoch
        err = np.abs(got - want)
        assert (err <= _value_tol(want, sig)).all(), (epoch, err.max())
        worst = max(worst, float((err / np.maximum(sig, 1e-300))[~exact].max()) if (~exact).any() else 0.0)
    print(f"({B}, {V}, {n_ticks}): max |device - mirror| / sigma of a noisy field = {worst:.3e} "
          f"(draw tolerance {ATOL:.3e}); {lost_seen} lost measurements in 6 epochs")
    if B * V >= 9:
        assert lost_seen > 0 and {0.0, 0.5, 1.0} <= set(np.unique(rows[..., SM.P_DROP]))


@pytest.mark.parametrize("B, V, n_ticks", SHAPES)
def test_the_lag_is_read(gpu, B, V, n_ticks):
    """Rows that are only late take the arithmetic path with every sigma 0: x + 0 * z = x for
    x != 0, so the measurement is the earlier tick, bitwise."""
    x = _path(B, V, n_ticks)
    assert (x != 0.0).all()
    k = _k_meas(n_ticks)
    rows = SM.nominal_rows(B, V)
    n = np.arange(B * V).reshape(B, V)
    rows[..., SM.LAG] = np.choose(n % 3, [3.0, 1e9, 1.0])
    out, deliv = _measure(x, k, rows, SEED, 0, 0, _held(B, V, gpu), gpu)
    src = np.maximum(0, k - np.choose(n % 3, [3, 10 ** 9, 1]))
    want = np.take_along_axis(x, src[:, :, None, None], axis=2)[:, :, 0]
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and deliv.cpu().numpy().all()
    got_m, _ = SM.measure(x, k, rows, SEED, 0, 0, np.full((B, V, 6), np.nan))
    assert np.array_equal(_bits(got_m), _bits(want))


@pytest.mark.parametrize("B, nO, hp", OSHAPES)
def test_sensed_prediction_matches_the_mirror(gpu, B, nO, hp):
    rows = _obstacle_rows(B, nO)
    rng = np.random.default_rng(4)
    osense = np.stack([rng.uniform(0.05, 0.2, (B, nO)), rng.uniform(0.01, 0.05, (B, nO)),
                       rng.uniform(0.05, 0.3, (B, nO))], axis=-1)
    n = np.arange(B * nO).reshape(B, nO)
    osense[n % 5 == 1] = 0.0                                  # exact sensors in between
    osense[n % 5 == 2, 1:] = 0.0                              # position noise only
    epoch, b_off = 3, 77
    got = SE.predict_sensed(_dev(rows, gpu), _dev(osense, gpu), SEED, epoch, b_off, T_MEAS, LEAD, DT,
                            hp).cpu().numpy()
    want = SM.predict_sensed(rows, osense, SEED, epoch, b_off, T_MEAS, LEAD, DT, hp)
    T = ((np.arange(hp) + 1) * DT + LEAD)[None, None, None, :]
    s = np.abs(rows[..., OM.SPEED])[..., None, None] + 10 * osense[..., 2, None, None]
    tol = ATOL * (osense[..., 0, None, None] + T * s * osense[..., 1, None, None]
                  + T * osense[..., 2, None, None]) + 1e-12
    err = np.abs(got - want)
    print(f"({B}, {nO}, {hp}): max |device - mirror| of the sensed prediction = {err.max():.3e} m "
          f"(smallest tolerance {tol.min():.3e})")
    assert (err <= tol).all()
    exact = OB.predict(_dev(rows, gpu), T_MEAS, LEAD, DT, hp).cpu().numpy()
    assert np.array_equal(_bits(got[n % 5 == 1]), _bits(exact[n % 5 == 1]))
    moved = np.abs(got - exact)[n % 5 != 1]
    assert moved.reshape(len(moved), -1).max(axis=1).min() > 1e-6     # every noisy sensor is read
    # another epoch draws again; the same epoch does not
    again = SE.predict_sensed(_dev(rows, gpu), _dev(osense, gpu), SEED, epoch + 1, b_off, T_MEAS,
                              LEAD, DT, hp).cpu().numpy()
    assert np.abs(again - got)[n % 5 != 1].max() > 1e-6
    # a bad osense row or a bad obstacle row: NaN in its block only
    bad_o, bad_r = osense.copy(), rows.copy()
    bad_o[B - 1, nO - 2, 1] = -0.01
    bad_o[0, 0, 2] = math.nan
    bad_r[B - 1, nO - 1, OM.WIDTH] = -1.0
    res = SE.predict_sensed(_dev(bad_r, gpu), _dev(bad_o, gpu), SEED, epoch, b_off, T_MEAS, LEAD, DT,
                            hp).cpu().numpy()
    ok = np.ones((B, nO), bool)
    ok[B - 1, nO - 2] = ok[0, 0] = ok[B - 1, nO - 1] = False
    assert np.isnan(res[~ok]).all() and np.array_equal(_bits(res[ok]), _bits(got[ok]))
    assert np.isnan(SM.predict_sensed(bad_r, bad_o, SEED, epoch, b_off, T_MEAS, LEAD, DT, hp)[~ok]).all()


# ---------------------------------------------------------------------------
# 3. lanes are independent
# ---------------------------------------------------------------------------
def _run_epochs(x_list, k, rows, b_off, gpu, held0=math.nan):
    B, V = rows.shape[:2]
    held = _held(B, V, gpu, held0)
    outs, delivs = [], []
    for epoch, x in enumerate(x_list):
        out, deliv = _measure(x, k, rows, SEED, epoch, b_off, held, gpu)
        outs.append(out)
        delivs.append(deliv)
    return torch.stack(outs), torch.stack(delivs), held


def test_a_split_batch_measures_what_the_whole_does(gpu):
    B, V, n_ticks = SHAPES[1]
    rows = _noisy_rows(B, V)
    xs = [_path(B, V, n_ticks, seed=200 + e) for e in range(3)]
    k = _k_meas(n_ticks)
    whole = _run_epochs(xs, k, rows, 5, gpu)
    cut = 21
    lo = _run_epochs([x[:cut] for x in xs], k, rows[:cut], 5, gpu)
    hi = _run_epochs([x[cut:] for x in xs], k, rows[cut:], 5 + cut, gpu)
    # outputs [epoch, B, V, 6], delivered [epoch, B, V], x_held [B, V, 6]
    assert _eq(whole[0].view(torch.int64), torch.cat([lo[0], hi[0]], dim=1).view(torch.int64))
    assert _eq(whole[1], torch.cat([lo[1], hi[1]], dim=1))
    assert _eq(whole[2].view(torch.int64), torch.cat([lo[2], hi[2]], dim=0).view(torch.int64))
    assert (whole[1] == 0).any() and (whole[1] == 1).any()
    # the offset is read: the second half at offset 5 draws something else
    other = _run_epochs([x[cut:] for x in xs], k, rows[cut:], 5, gpu)
    assert not _eq(other[0], hi[0])


def test_changing_the_last_row_changes_only_its_lane(gpu):
    B, V, n_ticks = SHAPES[1]
    rows = _noisy_rows(B, V)
    rows[B - 1, V - 1] = [0.05, 0.01, 0.1, 0.002, 0.0, 1.0, 0.0, 0.0]
    xs = [_path(B, V, n_ticks, seed=300 + e) for e in range(2)]
    k = _k_meas(n_ticks)
    base = _run_epochs(xs, k, rows, 0, gpu)
    other = rows.copy()
    other[B - 1, V - 1] = [0.08, 0.02, 0.0, 0.004, 0.01, 1.02, 0.0, 2.0]
    res = _run_epochs(xs, k, other, 0, gpu)
    keep = torch.ones((B, V), dtype=torch.bool, device=gpu)
    keep[B - 1, V - 1] = False
    assert _eq(res[0][:, keep].view(torch.int64), base[0][:, keep].view(torch.int64))
    assert _eq(res[1][:, keep], base[1][:, keep])
    assert _eq(res[2][keep].view(torch.int64), base[2][keep].view(torch.int64))
    assert not _eq(res[0][:, ~keep], base[0][:, ~keep])


# ---------------------------------------------------------------------------
# 4. bad rows, one per rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("field, value", [(SM.SIG_HEADING, math.nan), (SM.SIG_POS, -1e-3),
                                          (SM.P_DROP, 1.5), (SM.LAG, 0.5), (SM.LAG, -1.0)])
def test_a_bad_row_is_nan_and_alone(gpu, field, value):
    B, V, n_ticks = SHAPES[1]
    rows = _noisy_rows(B, V)
    xs = [_path(B, V, n_ticks, seed=400 + e) for e in range(2)]
    k = _k_meas(n_ticks)
    base = _run_epochs(xs, k, rows, 0, gpu, held0=123.0)     # x_held finite: the NaN is written
    assert not torch.isnan(base[0]).any() and not torch.isnan(base[2]).any()
    b, v = B - 1, V - 2                                      # lane 256: the second-to-last
    assert b * V + v == B * V - 2
    rows[b, v, field] = value
    assert SM.bad_row(rows[b, v])
    res = _run_epochs(xs, k, rows, 0, gpu, held0=123.0)      # returns 0: no exception
    ok = torch.ones((B, V), dtype=torch.bool, device=gpu)
    ok[b, v] = False
    assert torch.isnan(res[0][:, b, v]).all() and torch.isnan(res[2][b, v]).all()
    assert (res[1][:, b, v] == 0).all()
    assert _eq(res[0][:, ok].view(torch.int64), base[0][:, ok].view(torch.int64))
    assert _eq(res[1][:, ok], base[1][:, ok])
    assert _eq(res[2][ok].view(torch.int64), base[2][ok].view(torch.int64))
    want, want_d = SM.measure(xs[0], k, rows, SEED, 0, 0, np.full((B, V, 6), 123.0))
    assert np.isnan(want[b, v]).all() and want_d[b, v] == 0


# ---------------------------------------------------------------------------
# 5. the sampler against the mirror
# ---------------------------------------------------------------------------
def _dists(n_veh, seed, b_offset=0):
    d = SE.SenseDist(n_veh, seed, b_offset)
    d.normal("sig_pos", 0.02, 0.02, 0.08, mean=0.05).uniform("sig_heading", 0.01, 0.002, 0.018, mean=0.01)
    d.fixed("sig_speed", np.linspace(0.05, 0.1, n_veh)).normal("bias_heading", 0.02)
    d.fixed("scale_speed", 1.03).uniform("p_drop", 0.4, 0.0, 0.5, mean=0.3)
    d.uniform("lag", 3.0, 0.0, 5.0, mean=2.0)
    m = SM.Dist(n_veh, seed, b_offset)
    m.set(SM.SIG_POS, SM.NORMAL, 0.02, 0.02, 0.08, mean=0.05)
    m.set(SM.SIG_HEADING, SM.UNIFORM, 0.01, 0.002, 0.018, mean=0.01)
    m.set(SM.SIG_SPEED, SM.FIXED, 0.0, mean=np.linspace(0.05, 0.1, n_veh))
    m.set(SM.BIAS_HEADING, SM.NORMAL, 0.02).set(SM.SCALE_SPEED, SM.FIXED, 0.0, mean=1.03)
    m.set(SM.P_DROP, SM.UNIFORM, 0.4, 0.0, 0.5, mean=0.3).set(SM.LAG, SM.UNIFORM, 3.0, 0.0, 5.0, mean=2.0)
    return d, m


def test_sampler_matches_the_mirror(gpu):
    """FIXED and UNIFORM fields bitwise (the uniform is exact, mean + spread * xi is two
    roundings on both sides, and rint of equal numbers is equal); NORMAL fields within the
    draw tolerance times the spread plus one rounding of the value."""
    seed, b_off, B, nV = SEED, 1000, 64, 6
    d, m = _dists(nV, seed, b_off)
    got = d.sample(B, device=gpu).cpu().numpy()
    want = SM.sample(m, B)
    assert got.shape == want.shape == (B, nV, 8)
    for f in (SM.SIG_HEADING, SM.SIG_SPEED, SM.SIG_STEER, SM.SCALE_SPEED, SM.P_DROP, SM.LAG):
        assert np.array_equal(_bits(got[..., f]), _bits(want[..., f])), f
    assert np.all(got[..., SM.SCALE_SPEED] == 1.03) and np.all(got[..., SM.SIG_STEER] == 0.0)
    assert np.array_equal(got[..., SM.SIG_SPEED], np.broadcast_to(np.linspace(0.05, 0.1, nV), (B, nV)))
    for f, spread in ((SM.SIG_POS, 0.02), (SM.BIAS_HEADING, 0.02)):
        err = np.abs(got[..., f] - want[..., f])
        print(f"field {SE.FIELDS[f]}: max |device - mirror| = {err.max():.3e} "
              f"(draw tolerance times the spread {ATOL * spread:.3e})")
        assert (err <= _value_tol(want[..., f], spread)).all()
    # LAG is a whole number; clamps are honoured, and reached
    lag = got[..., SM.LAG]
    assert np.array_equal(lag, np.rint(lag)) and set(np.unique(lag)) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    assert got[..., SM.SIG_POS].min() == 0.02 and got[..., SM.SIG_POS].max() == 0.08
    assert got[..., SM.SIG_HEADING].min() == 0.002 and got[..., SM.SIG_HEADING].max() == 0.018
    assert got[..., SM.P_DROP].min() == 0.0 and got[..., SM.P_DROP].max() == 0.5
    SE.validate(got)
    assert not any(SM.bad_row(r) for r in got.reshape(-1, 8))


def test_sampler_does_not_depend_on_the_sharding(gpu):
    d, _ = _dists(6, 99)
    whole = d.sample(6, device=gpu)
    parts = [d.with_offset(o).sample(3, device=gpu) for o in (0, 3)]
    assert _eq(whole, torch.cat(parts))
    assert not _eq(parts[0], parts[1])
    assert not _eq(whole, _dists(6, 100)[0].sample(6, device=gpu))


# ---------------------------------------------------------------------------
# 6. statistics of the draws
# ---------------------------------------------------------------------------
STAT_SEED = 2024


def _stat_bounds(z, lost, p):
    n, nl = z.size, lost.size
    return ((abs(z.mean()), 5 / math.sqrt(n)), (abs(z.var() - 1.0), 5 * math.sqrt(2 / n)),
            (abs(lost.mean() - p), 5 * math.sqrt(p * (1 - p) / nl)))


def test_statistics_of_noise_and_drops(gpu):
    """(B, n_veh) = (512, 8) in one call, SIG_POS = 0.05, P_DROP = 0.3, x_held finite.  The
    standardised position errors of the delivered lanes (n about 5700) have |mean| <= 5 / sqrt n
    and a variance within 1 +- 5 sqrt(2 / n); the lost fraction of the 4096 lanes is within
    5 sqrt(p (1 - p) / n) of p.  The seed 2024 was chosen so that the mirror alone, run on the
    CPU, is inside all three bounds (n = 5758: |mean| 1.4e-3 of 6.6e-2, |var - 1| 1.4e-2 of
    9.3e-2, lost fraction off by 2.9e-3 of 3.6e-2); the test checks that again before it looks
    at the device."""
    B, V, sigma, p, epoch = 512, 8, 0.05, 0.3, 9
    b, v = np.meshgrid(np.arange(B), np.arange(V), indexing="ij")
    z0, z1, _ = SM.calls(STAT_SEED, 0, epoch, SM.SITE_SENSE_DRAW, v, b)
    lost_m = SM.calls(STAT_SEED, 3, epoch, SM.SITE_SENSE_DRAW, v, b)[2] < p
    zm = np.stack([z0, z1], -1)[~lost_m]
    for got, bound in _stat_bounds(zm, lost_m, p):
        assert got <= bound, "the mirror itself is outside: choose another seed"
    rows = SM.nominal_rows(B, V)
    rows[..., SM.SIG_POS], rows[..., SM.P_DROP] = sigma, p
    x = _path(B, V, 1, seed=9)
    held = _held(B, V, gpu, 1e3)
    out, deliv = _measure(x, 1, rows, STAT_SEED, epoch, 0, held, gpu)
    got, d = out.cpu().numpy(), deliv.cpu().numpy()
    lost = d == 0
    assert np.array_equal(lost, lost_m)
    assert (got[lost] == 1e3).all()
    z = (got[..., 0:2] - x[:, :, 1, 0:2])[~lost] / sigma
    res = _stat_bounds(z, lost, p)
    print(f"n = {z.size}: |mean| {res[0][0]:.3e} (bound {res[0][1]:.3e}), |var - 1| {res[1][0]:.3e} "
          f"(bound {res[1][1]:.3e}); lost fraction {lost.mean():.4f}, off by {res[2][0]:.3e} "
          f"(bound {res[2][1]:.3e})")
    for g, bound in res:
        assert g <= bound


# ---------------------------------------------------------------------------
# 7. rollout: circle, 2 vehicles, Hp 10, B = 4, 3 steps, noise seed 1
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
        hist=[{k: h[k].clone() for k in keys + ("x_meas", "delivered", "obst") if k in h}
              for h in cl.history], metrics=cl.metrics())


def _circle_rows(sc, B):
    rows = SM.nominal_rows(B, sc.nVeh)
    rows[..., SM.SIG_POS] = 0.05
    rows[1, :, SM.P_DROP] = 1.0
    rows[2, :, SM.LAG] = sc.ticks_per_sim - sc.ticks_delay_x
    return rows


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(2, Hp=10)
    B = 4
    x_init = _x_init(sc, B)
    rows = _circle_rows(sc, B)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, kw in (("none", {}), ("nominal", dict(sensing=SM.nominal_rows(B, sc.nVeh))),
                     ("noisy", dict(sensing=rows, sense_seed=SENSE_SEED))):
        cl.reset(x_init, seed=1, **kw)
        cl.run(STEPS)
        runs[name] = _snapshot(cl)
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, metrics=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, sensing=rows[o:o + 2], sense_seed=SENSE_SEED)
        half.run(STEPS)
        runs[f"half{o}"] = _snapshot(half)
    half.close()
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, rows=rows, runs=runs)
    cl.close()


def test_rollout_with_nominal_rows_is_the_rollout_without(rollouts):
    a, b = rollouts.runs["none"], rollouts.runs["nominal"]
    assert len(a.hist) == len(b.hist) == STEPS
    for i in range(STEPS):
        assert "x_meas" not in a.hist[i] and "delivered" not in a.hist[i]
        for k in KEYS:
            assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
        assert (b.hist[i]["delivered"] == 1).all()
    for k, v in a.metrics.items():
        assert _eq(v, b.metrics[k]), k


def test_rollout_records_what_measure_gives(rollouts, gpu):
    ro, sc, cl = rollouts, rollouts.sc, rollouts.cl
    hist = ro.runs["noisy"].hist
    tps, tdx = sc.ticks_per_sim, sc.ticks_delay_x
    rows = _dev(ro.rows, gpu)
    held = _held(ro.B, sc.nVeh, gpu)
    horizon = sc.delay_x + sc.dt + sc.delay_u
    for i, rec in enumerate(hist):
        if i == 0:
            again = SE.measure(_dev(ro.x_init, gpu), 0, rows, SENSE_SEED, 0, 0, held)
        else:
            again = SE.measure(hist[i - 1]["path"], tps - tdx, rows, SENSE_SEED, i, 0, held)
        assert _eq(rec["x_meas"].view(torch.int64), again.view(torch.int64)), i
        x0, _ = PL.delay_compensate(cl.params, rec["x_meas"], rec["u0"], horizon, h_max=cl.h_max,
                                    device=gpu, rng=PL.NoiseStream(1, PL.SIGMA_NOISE, i, 0))
        assert _eq(rec["x0"], x0), i
    # P_DROP = 1: the first measurement is held for ever
    assert (hist[0]["delivered"][1] == 1).all()
    for i in (1, 2):
        assert (hist[i]["delivered"][1] == 0).all()
        assert _eq(hist[i]["x_meas"][1], hist[0]["x_meas"][1])
    assert _eq(hist[2]["x_meas"][1], hist[1]["x_meas"][1])
    # LAG = tps - tdx: entry 0 of the previous path, which is the state one step earlier
    for i in (1, 2):
        late = hist[i]["x_meas"][2] - hist[i - 1]["path"][2, :, 0]
        assert late[:, 2:].abs().max().item() == 0.0 and 0 < late[:, :2].abs().max().item() < 0.5
    # the controller acts on what it is told: the realised paths leave the exact-sensing ones
    d = (hist[STEPS - 1]["path"] - ro.runs["none"].hist[STEPS - 1]["path"])[..., 0:2].abs()
    moved = d.flatten(1).max(dim=1).values
    print(f"realised positions move by {moved.tolist()} m after {STEPS} steps of noisy sensing")
    assert (moved > 1e-6).all()


def test_rollout_with_sensing_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["noisy"].hist):
        for k in KEYS + ("x_meas", "delivered"):
            parts = torch.cat([ro.runs["half0"].hist[i][k], ro.runs["half2"].hist[i][k]])
            assert _eq(whole[k], parts), (i, k)
    for k, v in ro.runs["noisy"].metrics.items():
        assert _eq(v, torch.cat([ro.runs["half0"].metrics[k], ro.runs["half2"].metrics[k]])), k


def test_rollout_frog_with_obstacle_sensing(gpu):
    from scpqp.metrics import PathMetrics
    from scpqp.rollout import ClosedLoopBatch
    sc = R.frog_scenario(Hp=10)
    B, steps = 2, 2
    x_init = _x_init(sc, B)
    rows = OB.nominal(sc, B, device=gpu)
    osense = torch.zeros((B, sc.nObst, 3), dtype=torch.float64, device=gpu)
    osense[..., 0] = 0.1
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    with pytest.raises(ValueError, match=r"obstacles\.nominal"):
        cl.reset(x_init, seed=1, obstacle_sensing=osense, sense_seed=SENSE_SEED)
    cl.reset(x_init, seed=1, obstacles=rows, obstacle_sensing=osense, sense_seed=SENSE_SEED)
    cl.run(steps)
    lead = sc.delay_x + sc.dt + sc.delay_u
    pm = PathMetrics(sc, B, gpu)
    pm.reset(B)
    for i, rec in enumerate(cl.history):
        assert "x_meas" not in rec                               # vehicle sensing is off
        t_meas = max(0, i * sc.ticks_per_sim - sc.ticks_delay_x) * sc.tick_length
        again = SE.predict_sensed(rows, osense, SENSE_SEED, i, 0, t_meas, lead, sc.dt, sc.Hp)
        assert _eq(rec["obst"], again), i
        off = (rec["obst"] - OB.predict(rows, t_meas, lead, sc.dt, sc.Hp)).abs().max().item()
        assert off > 1e-3, i
        pm.accumulate(rec["path"], tick0=i * sc.ticks_per_sim, k_first=0 if i == 0 else 1,
                      obstacles=rows)
    # the world keeps the true rows: the gaps are those of the true obstacles on the kept paths
    res = pm.result()
    for k, v in cl.metrics().items():
        assert _eq(v, res[k]), k
    pm.close()
    cl.close()


def test_reset_refuses_bad_sensing_before_anything_is_launched(rollouts, gpu):
    ro, cl, sc = rollouts, rollouts.cl, rollouts.sc
    n_hist, i = len(cl.history), cl.i
    state, rows_before, held = cl.state.clone(), cl.sense_rows.clone(), cl.x_held.clone()
    good = ro.rows
    bad, late = good.copy(), good.copy()
    bad[3, 1, SM.P_DROP] = 1.5
    late[0, 1, SM.LAG] = sc.ticks_per_sim - sc.ticks_delay_x + 1
    for kw in (dict(sensing=good[:2], sense_seed=1), dict(sensing=good[:, :1], sense_seed=1),
               dict(sensing=good[..., :7], sense_seed=1), dict(sensing=bad, sense_seed=1),
               dict(sensing=torch.as_tensor(bad), sense_seed=1), dict(sensing=late, sense_seed=1),
               dict(sensing=good), dict(obstacle_sensing=np.zeros((4, 1, 3)), sense_seed=1)):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, **kw)
    with pytest.raises(ValueError, match=r"rows\[3, 1\]: p_drop"):
        cl.reset(ro.x_init, seed=1, sensing=bad, sense_seed=1)
    max_lag = sc.ticks_per_sim - sc.ticks_delay_x
    with pytest.raises(ValueError, match=rf"rows\[0, 1\]: lag must be <= {max_lag} ticks"):
        cl.reset(ro.x_init, seed=1, sensing=late, sense_seed=1)
    with pytest.raises(ValueError, match="sense_seed"):
        cl.reset(ro.x_init, seed=1, sensing=good)
    with pytest.raises(ValueError, match=r"obstacles\.nominal"):
        cl.reset(ro.x_init, seed=1, obstacle_sensing=np.zeros((4, 1, 3)), sense_seed=1)
    assert len(cl.history) == n_hist and cl.i == i           # the refused resets changed nothing
    assert _eq(cl.state, state) and _eq(cl.sense_rows, rows_before)
    assert _eq(cl.x_held.view(torch.int64), held.view(torch.int64))
