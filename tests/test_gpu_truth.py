"""The plant truth on the device (include/scpqp_truth.h): the plant step with a truth row
per (realisation, vehicle) against the existing plant step, the exact flow and the CPU
mirror (tests/truth_mirror.py); the sampler against the mirror; the rollout.

Shapes are the smallest at which lane indexing, the workgroup boundary and the tail
guard can go wrong: n_veh = 3 (no power of two); B = 8, n_veh = 4, n_ticks = 10 (352
lanes: two workgroups of 256, a ragged tail); B = 1, n_veh = 1, n_ticks = 0."""
import types

import numpy as np
import pytest
import torch

import noise_mirror as NM
import truth_mirror as TM
from oracle import scp_reference as R
from scpqp import plant as PL
from scpqp import truth as TR

pytestmark = pytest.mark.gpu

SIGMA_TEST = 1e-2
H_MAX = PL.H_MAX
TICK = 0.01
SHAPES = [(2, 3, 4), (8, 4, 10), (1, 1, 0)]          # (B, n_veh, n_ticks)


def _params(V):
    return PL.plant_params([0.30 + 0.02 * v for v in range(V)], [0.34 + 0.01 * v for v in range(V)])


def _states(B, V, seed=3):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, V, 6))
    x[..., 0:2] = rng.uniform(-30, 30, (B, V, 2))
    x[..., 2] = rng.uniform(-np.pi, np.pi, (B, V))
    x[..., 3] = rng.uniform(3.0, 4.0, (B, V))
    x[..., 4] = rng.uniform(-0.5, 0.5, (B, V))
    x[..., 5] = rng.uniform(-0.05, 0.05, (B, V))
    return x


def _commands(B, V, K, seed=1):
    """Up to 0.078 rad, and away from -0.0 (gain * -0.0 + 0 is +0.0)."""
    u = np.random.default_rng(seed).uniform(-0.078, 0.078, (B, V, K))
    assert not np.any(u == 0.0)
    return u


def _rows(B, V):
    """Rows away from nominal: lf, lr +-30 %, tau in {0.08, 0.2}, gain in {0.8, 1.25},
    bias +-0.01, in changing combinations."""
    t = np.zeros((B, V, 5))
    n = 0
    for b in range(B):
        for v in range(V):
            t[b, v] = [0.34 * (1.3 if n & 1 else 0.7), 0.34 * (0.7 if n & 2 else 1.3),
                       0.08 if (n // 2) & 1 == 0 else 0.2, 0.8 if n % 3 else 1.25,
                       0.01 if n % 4 in (0, 3) else -0.01]
            n += 1
    return t


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


# ---------------------------------------------------------------------------
# 1. the nominal truth is the existing plant step, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B, V, n_ticks", SHAPES)
def test_nominal_truth_is_bitwise_the_existing_plant_step(gpu, B, V, n_ticks):
    p = _params(V)
    xs, ut = _states(B, V), _commands(B, V, n_ticks + 1)
    truth = TR.nominal(p, B, device=gpu)
    assert tuple(truth.shape) == (B, V, 5)
    pair = np.random.default_rng(9).standard_normal((B, V, 2)) * 1e-3
    rng = PL.NoiseStream(41, SIGMA_TEST, 2, 100)
    for kw in (dict(), dict(noise=pair), dict(rng=rng)):
        want = PL.plant_step(p, xs, ut, TICK, device=gpu, **kw)
        got = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, **kw)
        assert not torch.isnan(got).any()
        assert _eq(got, want), sorted(kw)
    if n_ticks:
        free = PL.plant_step(p, xs, ut, TICK, device=gpu)
        assert not _eq(PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, noise=pair), free)
        assert not _eq(PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, rng=rng), free)


def test_u_eff_is_gain_times_command_plus_bias_in_two_roundings(gpu):
    """A row that differs from nominal in gain and bias only is the existing plant step at
    the command u_eff = gain * u_ref + bias, bitwise, when u_eff is formed in two roundings
    (numpy never fuses); a fused multiply-add differs in the last bit for about a third of
    the 352 commands."""
    B, V, n_ticks = SHAPES[1]
    p = _params(V)
    xs, ut = _states(B, V), _commands(B, V, n_ticks + 1)
    truth = np.broadcast_to(TR.nominal_rows(p)[None], (B, V, 5)).copy()
    rng = np.random.default_rng(21)
    truth[..., 3] = rng.uniform(0.8, 1.25, (B, V))
    truth[..., 4] = rng.uniform(-0.01, 0.01, (B, V))
    u_eff = truth[..., 3:4] * ut + truth[..., 4:5]
    got = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth)
    assert _eq(got, PL.plant_step(p, xs, u_eff, TICK, device=gpu))


# ---------------------------------------------------------------------------
# 2. parity with the exact flow
# ---------------------------------------------------------------------------
def test_truth_plant_step_matches_the_exact_flow(gpu):
    """Within 1e-9 of DOP853 at 1e-13 at every tick, the bound tests/test_gpu_plant.py holds
    the nominal plant to.  The fixed-step RK4 over these rows (tau >= 0.08, h_max 2.5 ms)
    was measured at <= 2.0e-10 from the exact flow on the CPU for horizons up to 0.43 s."""
    B, V, n_ticks = 2, 3, 8
    p = _params(V)
    xs, ut, truth = _states(B, V, seed=13), _commands(B, V, n_ticks + 1, seed=14), _rows(B, V)
    assert set(truth[..., 2].ravel()) == {0.08, 0.2} and set(truth[..., 3].ravel()) == {0.8, 1.25}
    assert set(truth[..., 4].ravel()) == {0.01, -0.01}
    got = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth).cpu().numpy()
    want = TM.plant_step_exact(xs, ut, truth, TICK)
    err = float(np.abs(got - want).max())
    nominal = PL.plant_step(p, xs, ut, TICK, device=gpu).cpu().numpy()
    print(f"truth rows: max |device - exact| = {err:.3e} (bound 1e-9); "
          f"the rows move the path by {np.abs(got - nominal).max():.3e}")
    assert np.abs(got - nominal).max() > 1e-4            # the truth is read
    assert err < 1e-9, err


def test_truth_plant_step_fast_lag_at_a_finer_step(gpu):
    """tau = 0.04 at h_max = 1 ms, under the same bound (measured 4.6e-11 on the CPU)."""
    B, V, n_ticks = 1, 1, 8
    p = _params(V)
    xs, ut = _states(B, V, seed=15), _commands(B, V, n_ticks + 1, seed=16)
    truth = np.array([[[0.25, 0.45, 0.04, 1.25, -0.01]]])
    got = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, h_max=1e-3).cpu().numpy()
    err = float(np.abs(got - TM.plant_step_exact(xs, ut, truth, TICK)).max())
    print(f"tau 0.04, h_max 1 ms: max |device - exact| = {err:.3e} (bound 1e-9)")
    assert err < 1e-9, err


# ---------------------------------------------------------------------------
# 3. seeded, with a truth
# ---------------------------------------------------------------------------
def test_seeded_truth_noise_enters_only_x_and_y_and_linearly(gpu):
    """The statement of tests/test_gpu_noise.py with a truth: states 2..5 equal the
    noise-free truth call's bitwise, and (x, y) differ from it by the mirror's
    sum h/6 sigma (z1 + 2 z2 + 2 z3 + z4) of the same counters (the step count, and so c0,
    is what it is without a truth), within 8 n ulp(|position|)."""
    B, V, n_ticks = 2, 3, 4
    seed, epoch, b_off = 4711, 5, 300
    p = _params(V)
    xs, ut, truth = _states(B, V), _commands(B, V, n_ticks + 1, seed=3), _rows(B, V)
    rng = PL.NoiseStream(seed, SIGMA_TEST, epoch, b_off)
    pf = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth)
    pn = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, rng=rng)
    assert _eq(pn[..., 2:], pf[..., 2:])
    assert _eq(pn[:, :, 0], pf[:, :, 0])
    d = (pn - pf).cpu().numpy()
    pos = np.abs(pn[..., 0:2].cpu().numpy()).max()
    worst = 0.0
    for b in range(B):
        for v in range(V):
            for k in range(1, n_ticks + 1):
                T = k * TICK
                n = TM.steps_for(T, H_MAX)
                assert n == 4 * k
                z = NM.draws(seed, epoch, NM.SITE_PLANT, k, v, b_off + b, 4 * n)
                want = TM.rk4_noise_shift(z, T / n, SIGMA_TEST)
                atol = 8 * n * np.spacing(pos)
                err = np.abs(d[b, v, k, 0:2] - want).max()
                worst = max(worst, err / atol)
                assert err <= atol, (b, v, k, err, atol)
                assert np.abs(d[b, v, k, 0:2]).max() > 1e-7
    print(f"seeded truth: worst error / tolerance = {worst:.3f}")


# ---------------------------------------------------------------------------
# 4. rows are per lane
# ---------------------------------------------------------------------------
def test_rows_are_per_lane(gpu):
    B, V, n_ticks = SHAPES[1]
    p = _params(V)
    xs, ut, truth = _states(B, V), _commands(B, V, n_ticks + 1), _rows(B, V)
    rng = PL.NoiseStream(7, 0.0, 0, 0)                   # sigma 0: the seeded kernel, no b in it
    perm = np.array([3, 0, 7, 1, 6, 2, 5, 4])
    for kw in (dict(), dict(rng=rng)):
        base = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, **kw)
        moved = PL.plant_step(p, xs[perm], ut[perm], TICK, device=gpu, truth=truth[perm], **kw)
        assert _eq(moved, base[torch.as_tensor(perm, device=gpu)])
        assert not _eq(moved, base)
        # another row for one (realisation, vehicle): only its outputs change
        t2 = truth.copy()
        t2[5, 2] = [0.40, 0.30, 0.12, 1.1, 0.005]
        other = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=t2, **kw)
        same = torch.ones((B, V), dtype=torch.bool)
        same[5, 2] = False
        assert _eq(other[same], base[same])
        assert not torch.equal(other[5, 2, 1:], base[5, 2, 1:])
        assert _eq(other[5, 2, 0], base[5, 2, 0])        # k = 0 is the start state


# ---------------------------------------------------------------------------
# 5. bad rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["tau=0", "tau=nan", "lf=-lr"])
def test_a_bad_row_makes_exactly_its_own_block_nan(gpu, what):
    B, V, n_ticks = SHAPES[1]
    p = _params(V)
    xs, ut, truth = _states(B, V), _commands(B, V, n_ticks + 1), _rows(B, V)
    bad = truth.copy()
    b, v = 6, 3                                          # lanes of the second workgroup's tail
    if what == "tau=0":
        bad[b, v, 2] = 0.0
    elif what == "tau=nan":
        bad[b, v, 2] = float("nan")
    else:
        bad[b, v, 0] = -bad[b, v, 1]
    for kw in (dict(), dict(rng=PL.NoiseStream(3, SIGMA_TEST, 1, 0))):
        base = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=truth, **kw)
        got = PL.plant_step(p, xs, ut, TICK, device=gpu, truth=bad, **kw)   # returns 0: no raise
        assert tuple(got[b, v].shape) == (n_ticks + 1, 6)
        assert bool(torch.isnan(got[b, v]).all())        # k = 0 included
        ok = torch.ones((B, V), dtype=torch.bool)
        ok[b, v] = False
        assert not torch.isnan(got[ok]).any()
        assert _eq(got[ok], base[ok])


# ---------------------------------------------------------------------------
# 6. the sampler against the mirror
# ---------------------------------------------------------------------------
def _dists(sc, seed, b_offset=0):
    d = TR.TruthDist(sc, seed, b_offset)
    d.uniform("lf", 0.1, 0.2, 0.5).uniform("lr", 0.1, 0.30, 0.36)
    d.normal("tau", 0.02, 0.07, 0.13).normal("gain", 0.1, 0.5, 2.0)
    m = TM.Dist(d.mean, seed, b_offset)
    m.set(TM.LF, TM.UNIFORM, 0.1, 0.2, 0.5).set(TM.LR, TM.UNIFORM, 0.1, 0.30, 0.36)
    m.set(TM.TAU, TM.NORMAL, 0.02, 0.07, 0.13).set(TM.GAIN, TM.NORMAL, 0.1, 0.5, 2.0)
    return d, m


def test_sampler_matches_the_mirror(gpu):
    """FIXED and UNIFORM fields bitwise (the uniform is exact and mean + spread * xi is two
    roundings on both sides); NORMAL fields within the tolerance of a normal draw of
    tests/test_gpu_noise.py::test_raw_draws_match_the_mirror (64 * 2^-52 * 10) times spread."""
    sc = R.circle_scenario(3, Hp=10)
    seed, b_off, B = 0x123456789ABCDEF, 1000, 64
    d, m = _dists(sc, seed, b_off)
    got = d.sample(B, device=gpu).cpu().numpy()
    want = TM.sample(m, B)
    assert got.shape == want.shape == (B, 3, 5)
    for f in (TM.LF, TM.LR, TM.BIAS):
        assert np.array_equal(got[..., f], want[..., f]), f
    assert np.all(got[..., TM.BIAS] == 0.0)
    atol = 64 * 2.0 ** -52 * 10
    for f, spread in ((TM.TAU, 0.02), (TM.GAIN, 0.1)):
        err = np.abs(got[..., f] - want[..., f]).max()
        print(f"field {f}: max |device - mirror| = {err:.3e} (atol {atol * spread:.3e})")
        assert err <= atol * spread
    # clamps are honoured, and reached
    assert got[..., TM.LR].min() == 0.30 and got[..., TM.LR].max() == 0.36
    assert got[..., TM.TAU].min() == 0.07 and got[..., TM.TAU].max() == 0.13
    assert np.all(got[..., TM.GAIN] >= 0.5) and np.all(got[..., TM.GAIN] <= 2.0)
    assert np.all(np.abs(got[..., TM.LF] - 0.34) <= 0.1) and np.ptp(got[..., TM.LF]) > 0.15
    TR.validate(got, H_MAX)


def test_sampler_does_not_depend_on_the_sharding(gpu):
    sc = R.circle_scenario(3, Hp=10)
    d, _ = _dists(sc, 99)
    whole = d.sample(6, device=gpu)
    parts = [d.with_offset(o).sample(3, device=gpu) for o in (0, 3)]
    assert _eq(whole, torch.cat(parts))
    assert not _eq(parts[0], parts[1])
    assert not _eq(whole, _dists(sc, 100)[0].sample(6, device=gpu))


def test_fill_nominal_equals_the_host_rows(gpu):
    for B, V, _ in SHAPES:
        p = _params(V)
        got = TR.nominal(p, B, device=gpu).cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(TR.nominal_rows(p)[None], (B, V, 5)))
    sc = R.circle_scenario(3, Hp=10)
    got = TR.nominal(sc, 2, device=gpu).cpu().numpy()
    assert np.array_equal(got[1, 2], TM.nominal_row(sc.Lf[2], sc.Lr[2]))


# ---------------------------------------------------------------------------
# 7. rollout: 2-vehicle circle, Hp 10, B = 4, 3 steps, noise seed 1
# ---------------------------------------------------------------------------
STEPS = 3
KEYS = ("x0", "u0", "umax", "U", "traj", "n_scp", "status", "path", "delay_traj", "u_tick",
        "x_start", "ec_noise")


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(hist):
    return [{k: h[k].clone() for k in KEYS} for h in hist]


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(2, Hp=10)
    B = 4
    x_init = _x_init(sc, B)
    nominal = np.broadcast_to(TR.nominal_rows(sc)[None], (B, 2, 5)).copy()
    mixed = nominal.copy()
    mixed[2:, :, 0:2] *= 0.8                              # a 20 % shorter wheelbase
    mixed[2:, :, 2] = 0.15
    mixed[2:, :, 3] = 0.9
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True)
    runs = {}
    for name, truth in (("none", None), ("nominal", nominal), ("mixed", mixed)):
        cl.reset(x_init, seed=1, truth=truth)
        assert (cl.truth is None) == (truth is None)
        runs[name] = _snapshot(cl.run(STEPS))
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o, truth=mixed[o:o + 2])
        runs[f"half{o}"] = _snapshot(half.run(STEPS))
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, runs=runs, mixed=mixed)
    half.close()
    cl.close()


def test_rollout_nominal_truth_is_the_rollout_without(rollouts):
    for a, b in zip(rollouts.runs["none"], rollouts.runs["nominal"]):
        for k in KEYS:
            assert _eq(a[k], b[k]), k


def test_rollout_nominal_realisations_do_not_see_their_neighbours_truth(rollouts):
    for i, (a, b) in enumerate(zip(rollouts.runs["none"], rollouts.runs["mixed"])):
        for k in KEYS:
            assert _eq(a[k][:2], b[k][:2]), (i, k)


def test_rollout_controller_does_not_know_the_truth(rollouts, gpu):
    ro = rollouts
    a, b = ro.runs["none"][0], ro.runs["mixed"][0]
    for k in ("x0", "U", "traj", "u_tick", "x_start"):
        assert _eq(a[k][2:], b[k][2:]), k                 # step 0: the same measurement
    moved = (a["path"][2:, :, :, 0:2] - b["path"][2:, :, :, 0:2]).abs().max().item()
    print(f"step 0: the truth moves the realised positions by up to {moved:.3e} m")
    assert moved > 1e-6
    for i, rec in enumerate(ro.runs["mixed"]):
        again = PL.plant_step(ro.cl.params, rec["x_start"], rec["u_tick"], ro.sc.tick_length,
                              truth=ro.mixed, rng=PL.NoiseStream(1, PL.SIGMA_NOISE, i, 0),
                              device=gpu)
        assert _eq(rec["path"], again), i
    # later steps: the controller reacts to another measurement
    assert not _eq(ro.runs["none"][2]["U"][2:], ro.runs["mixed"][2]["U"][2:])


def test_rollout_with_a_truth_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["mixed"]):
        for k in KEYS:
            parts = torch.cat([ro.runs["half0"][i][k], ro.runs["half2"][i][k]])
            assert _eq(whole[k], parts), (i, k)


def test_reset_refuses_a_bad_truth_before_anything_is_launched(rollouts):
    ro = rollouts
    cl = ro.cl
    n_hist, i = len(cl.history), cl.i
    bad_tau, bad_len, coarse = ro.mixed.copy(), ro.mixed.copy(), ro.mixed.copy()
    bad_tau[1, 0, 2] = 0.0
    bad_len[3, 1, 0] = -bad_len[3, 1, 1]
    coarse[0, 0, 2] = 0.01                                # < 8 h_max
    nan = ro.mixed.copy()
    nan[0, 1, 4] = float("nan")
    for truth in (ro.mixed[:2], ro.mixed[:, :1], ro.mixed[..., :4], bad_tau, bad_len, coarse, nan,
                  torch.as_tensor(bad_tau)):
        with pytest.raises(ValueError):
            cl.reset(ro.x_init, seed=1, truth=truth)
    assert len(cl.history) == n_hist and cl.i == i      # the refused resets changed nothing
