"""The reference's per-evaluation model noise on the device (include/scpqp_noise.h):
the generator against the CPU mirror (tests/noise_mirror.py), sharding, the way the
noise enters the integrators, and the noisy closed-loop rollout.

Shapes are the smallest that exercise every counter field: two realisations and two
vehicles at least, several RK4 steps per span, several output ticks."""
import types

import numpy as np
import pytest
import torch

import noise_mirror as NM
from oracle import scp_reference as R
from scpqp import plant as PL

pytestmark = pytest.mark.gpu

SIGMA_TEST = 1e-2      # the signal stands ~10 orders above the rounding tolerances
H_MAX = PL.H_MAX


def _params():
    sc = R.circle_scenario(2, Hp=10)
    return sc, PL.plant_params(sc.Lf, sc.Lr)


def _states(B, V, seed=3):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, V, 6))
    x[..., 0:2] = rng.uniform(-30, 30, (B, V, 2))
    x[..., 2] = rng.uniform(-np.pi, np.pi, (B, V))
    x[..., 3] = rng.uniform(2.0, 6.0, (B, V))
    x[..., 4] = rng.uniform(-0.5, 0.5, (B, V))
    x[..., 5] = rng.uniform(-0.05, 0.05, (B, V))
    return x


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def test_raw_draws_match_the_mirror(gpu):
    """out / sigma against the mirror's (z0, z1).  Both sides compute the same 53-bit
    uniforms exactly; they differ by the libm of log, sqrt, sin and cos and by the
    multiplication and division by sigma: a few ulp on values of magnitude <= 10
    (|z| <= sqrt(2 * 53 ln 2) = 8.6), so atol = 64 * 2^-52 * 10.  A wrong word order,
    round count, shift or counter field moves a draw by order 1."""
    B, V, n_eval, k, epoch, b_off, seed = 3, 2, 5, 3, 7, 1000, 0x123456789ABCDEF
    atol = 64 * 2.0 ** -52 * 10
    for site in (NM.SITE_DELAY, NM.SITE_PLANT, NM.SITE_LINEARIZE):
        rng = PL.NoiseStream(seed, SIGMA_TEST, epoch, b_off)
        out = PL.noise_fill(rng, B, V, site, k, n_eval, device=gpu).cpu().numpy()
        assert out.shape == (B, V, n_eval, 2)
        worst = 0.0
        for b in range(B):
            for v in range(V):
                want = NM.draws(seed, epoch, site, k, v, b_off + b, n_eval)
                worst = max(worst, np.abs(out[b, v] / SIGMA_TEST - want).max())
        print(f"site {site}: max |out / sigma - mirror| = {worst:.3e} (atol {atol:.3e})")
        assert worst <= atol
    # the ec_noise wrapper: site 2, k 0, one evaluation
    rng = PL.NoiseStream(seed, 3e-6, epoch, b_off)
    ec = PL.draw_ec_noise(rng, B, V, device=gpu)
    assert _eq(ec, PL.noise_fill(rng, B, V, NM.SITE_LINEARIZE, 0, 1, device=gpu).view(B, V, 2))
    want = np.array([[NM.draws(seed, epoch, 2, 0, v, b_off + b, 1)[0] for v in range(V)]
                     for b in range(B)])
    assert np.abs(ec.cpu().numpy() / 3e-6 - want).max() <= atol


def test_sharding_is_bitwise(gpu):
    """A realisation's draws depend on its global index only: B = 8 at offset 0 is the
    concatenation of B = 4 at offsets 0 and 4 (fill), and B = 4 of 2 + 2 (plant step,
    delay compensation)."""
    V, seed = 2, 99
    whole = PL.noise_fill(PL.NoiseStream(seed, 3e-6, 2, 0), 8, V, 1, 5, 6, device=gpu)
    parts = [PL.noise_fill(PL.NoiseStream(seed, 3e-6, 2, o), 4, V, 1, 5, 6, device=gpu)
             for o in (0, 4)]
    assert _eq(whole, torch.cat(parts))
    assert not _eq(parts[0], parts[1])
    sc, p = _params()
    xs = _states(4, V)
    ut = np.random.default_rng(1).uniform(-0.05, 0.05, (4, V, 5))
    whole = PL.plant_step(p, xs, ut, 0.01, rng=PL.NoiseStream(seed, SIGMA_TEST, 3, 0), device=gpu)
    parts = [PL.plant_step(p, xs[o:o + 2], ut[o:o + 2], 0.01,
                           rng=PL.NoiseStream(seed, SIGMA_TEST, 3, o), device=gpu) for o in (0, 2)]
    assert _eq(whole, torch.cat(parts))
    uh = ut[:, :, 0]
    whole = PL.delay_compensate(p, xs, uh, 0.43, rng=PL.NoiseStream(seed, SIGMA_TEST, 3, 0),
                                device=gpu)
    parts = [PL.delay_compensate(p, xs[o:o + 2], uh[o:o + 2], 0.43,
                                 rng=PL.NoiseStream(seed, SIGMA_TEST, 3, o), device=gpu)
             for o in (0, 2)]
    assert _eq(whole[0], torch.cat([q[0] for q in parts]))
    assert _eq(whole[1], torch.cat([q[1] for q in parts]))


def test_noise_enters_only_x_and_y_and_linearly(gpu):
    """The right-hand side never reads x[0], x[1], so with noise states 2..5 equal the
    noise-free entry points' bitwise, and (x, y) minus the noise-free (x, y) equals
    sum_steps h/6 sigma (z_k1 + 2 z_k2 + 2 z_k3 + z_k4) of the mirror's draws.
    atol = 8 * n_steps * ulp(max |position|) bounds the rounding of the two
    accumulations (nothing in it is measured).  Catches a wrong c0 order, a wrong
    per-tick stream and a draw reused across stages."""
    sc, p = _params()
    B, V, seed, epoch, b_off = 2, 2, 4711, 5, 300
    xs = _states(B, V)
    rng = PL.NoiseStream(seed, SIGMA_TEST, epoch, b_off)
    # delay compensation: horizon 0.43, 10 outputs, c0 counting on across the 9 spans
    horizon, n_out = 0.43, 10
    uh = np.random.default_rng(2).uniform(-0.05, 0.05, (B, V))
    x0_f, tr_f = PL.delay_compensate(p, xs, uh, horizon, n_out=n_out, device=gpu)
    x0_n, tr_n = PL.delay_compensate(p, xs, uh, horizon, n_out=n_out, rng=rng, device=gpu)
    assert _eq(x0_n[..., 2:], x0_f[..., 2:])
    assert _eq(tr_n[:, :, 2:, :], tr_f[:, :, 2:, :])
    assert _eq(tr_n[:, 0], tr_f[:, 0])                       # the start is not integrated
    assert _eq(tr_n[:, -1].transpose(1, 2), x0_n)
    span = horizon / (n_out - 1)
    n = NM.steps_for(span, H_MAX)
    assert n == 20
    d = (tr_n - tr_f).cpu().numpy()                          # [B, n_out, 6, V]
    pos = np.abs(tr_n[:, :, 0:2, :].cpu().numpy()).max()
    worst = 0.0
    for b in range(B):
        for v in range(V):
            z = NM.draws(seed, epoch, NM.SITE_DELAY, 0, v, b_off + b, 4 * n * (n_out - 1))
            for j in range(1, n_out):
                want = NM.rk4_noise_shift(z[:4 * n * j], span / n, SIGMA_TEST)
                atol = 8 * (n * j) * np.spacing(pos)
                err = np.abs(d[b, j, 0:2, v] - want).max()
                worst = max(worst, err / atol)
                assert err <= atol, (b, v, j, err, atol)
            assert np.abs(d[b, -1, 0:2, v]).max() > 1e-6     # the noise is there
    print(f"delay: worst error / tolerance = {worst:.3f}")
    # plant step: 4 ticks of 0.01; output k restarts at t0 with the stream of its own k
    n_ticks, tick = 4, 0.01
    ut = np.random.default_rng(3).uniform(-0.05, 0.05, (B, V, n_ticks + 1))
    pf = PL.plant_step(p, xs, ut, tick, device=gpu)
    pn = PL.plant_step(p, xs, ut, tick, rng=rng, device=gpu)
    assert _eq(pn[..., 2:], pf[..., 2:])
    assert _eq(pn[:, :, 0], pf[:, :, 0])
    d = (pn - pf).cpu().numpy()                              # [B, V, K, 6]
    pos = np.abs(pn[..., 0:2].cpu().numpy()).max()
    worst = 0.0
    for b in range(B):
        for v in range(V):
            for k in range(1, n_ticks + 1):
                T = k * tick
                n = NM.steps_for(T, H_MAX)
                assert n == 4 * k
                z = NM.draws(seed, epoch, NM.SITE_PLANT, k, v, b_off + b, 4 * n)
                want = NM.rk4_noise_shift(z, T / n, SIGMA_TEST)
                atol = 8 * n * np.spacing(pos)
                err = np.abs(d[b, v, k, 0:2] - want).max()
                worst = max(worst, err / atol)
                assert err <= atol, (b, v, k, err, atol)
                assert np.abs(d[b, v, k, 0:2]).max() > 1e-7
    print(f"plant: worst error / tolerance = {worst:.3f}")


def test_noisy_flow_matches_the_mirror_flow(gpu):
    """The whole noisy integration against the mirror's RK4 over bicycle_rhs with the
    same draws.  Same method, same steps, same draws: the two differ by the libm of the
    right-hand side (tan, atan, sin, cos, sqrt), fused multiply-adds and the draws' own
    libm, a few ulp of the largest state per evaluation, so atol = 64 ulp(30) per RK4
    step (4e-11 over the 180 steps; the noise itself moves x, y by ~1e-4)."""
    sc, p = _params()
    B, V, seed, epoch, b_off = 2, 2, 31, 1, 6
    xs = _states(B, V, seed=8)
    uh = np.random.default_rng(4).uniform(-0.05, 0.05, (B, V))
    horizon, n_out = 0.43, 10
    x0, _ = PL.delay_compensate(p, xs, uh, horizon, n_out=n_out,
                                rng=PL.NoiseStream(seed, SIGMA_TEST, epoch, b_off), device=gpu)
    x0 = x0.cpu().numpy()
    span = horizon / (n_out - 1)
    n = NM.steps_for(span, H_MAX)
    atol = 64 * n * (n_out - 1) * np.spacing(30.0)
    for b in range(B):
        for v in range(V):
            z = NM.draws(seed, epoch, NM.SITE_DELAY, 0, v, b_off + b, 4 * n * (n_out - 1))
            x = xs[b, v]
            for j in range(n_out - 1):
                x = NM.flow(x, uh[b, v], sc.Lf[v], sc.Lr[v], span, n, z[4 * n * j:], SIGMA_TEST)
            assert np.abs(x0[b, v] - x).max() <= atol, (b, v, np.abs(x0[b, v] - x).max(), atol)


def test_sigma_zero_equals_the_noise_free_entry_points(gpu):
    sc, p = _params()
    B, V = 2, 2
    xs = _states(B, V, seed=5)
    uh = np.random.default_rng(6).uniform(-0.05, 0.05, (B, V))
    ut = np.random.default_rng(7).uniform(-0.05, 0.05, (B, V, 5))
    rng = PL.NoiseStream(77, 0.0, 3, 11)
    a = PL.delay_compensate(p, xs, uh, 0.43, device=gpu)
    b = PL.delay_compensate(p, xs, uh, 0.43, rng=rng, device=gpu)
    assert _eq(a[0], b[0]) and _eq(a[1], b[1])
    assert _eq(PL.plant_step(p, xs, ut, 0.01, device=gpu),
               PL.plant_step(p, xs, ut, 0.01, rng=rng, device=gpu))
    assert not PL.noise_fill(rng, B, V, 1, 2, 4, device=gpu).any()


# ---------------------------------------------------------------------------
# rollout: 2-vehicle circle, Hp 10, B = 4, 3 steps
# ---------------------------------------------------------------------------
STEPS = 3
STATE_KEYS = ("x0", "u0", "umax", "U", "u", "traj", "n_scp", "status", "path", "delay_traj",
              "u_tick", "x_start")


def _x_init(sc, B):
    rng = np.random.default_rng(12)
    return np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])


def _snapshot(hist):
    """Records of a run, detached from the batch's reused output buffers."""
    out = []
    for h in hist:
        out.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in h.items()
                    if k in STATE_KEYS + ("ec_noise", "u_warm", "epoch")})
    return out


@pytest.fixture(scope="module")
def rollouts(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(2, Hp=10)
    B = 4
    x_init = _x_init(sc, B)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, trace=True)
    runs = {}
    for name, kw in (("seed1", dict(seed=1)), ("seed1_again", dict(seed=1)),
                     ("seed2", dict(seed=2)), ("seedless", dict()),
                     ("seed_none", dict(seed=None))):
        cl.reset(x_init, **kw)
        runs[name] = _snapshot(cl.run(STEPS))
    half = ClosedLoopBatch(sc, 2, device=gpu, keep_path=True, trace=True)
    for o in (0, 2):
        half.reset(x_init[o:o + 2], seed=1, b_offset=o)
        runs[f"half{o}"] = _snapshot(half.run(STEPS))
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, cl=cl, B=B, x_init=x_init, runs=runs)
    half.close()
    cl.close()


def test_rollout_ec_noise_is_the_fill_of_its_epoch(rollouts, gpu):
    ro = rollouts
    for i, rec in enumerate(ro.runs["seed1"]):
        assert rec["epoch"] == i
        want = PL.noise_fill(PL.NoiseStream(1, 3e-6, i, 0), ro.B, 2, 2, 0, 1, device=gpu)
        assert _eq(rec["ec_noise"], want.view(ro.B, 2, 2))
        assert rec["ec_noise"].abs().max() > 0
    for a, b in zip(ro.runs["seed1"][:-1], ro.runs["seed1"][1:]):
        assert not _eq(a["ec_noise"], b["ec_noise"])


def test_rollout_path_is_the_noisy_plant_step_of_its_epoch(rollouts, gpu):
    ro = rollouts
    for i, rec in enumerate(ro.runs["seed1"]):
        again = PL.plant_step(ro.cl.params, rec["x_start"], rec["u_tick"], ro.sc.tick_length,
                              rng=PL.NoiseStream(1, 3e-6, i, 0), device=gpu)
        assert _eq(rec["path"], again)
        free = PL.plant_step(ro.cl.params, rec["x_start"], rec["u_tick"], ro.sc.tick_length,
                             device=gpu)
        assert not _eq(rec["path"], free)


def test_rollout_solve_reads_the_recorded_ec_noise(rollouts, gpu):
    ro = rollouts
    for i, rec in enumerate(ro.runs["seed1"]):
        assert (rec["u_warm"] is None) == (i == 0)
        out = ro.cl.solver.solve(rec["x0"], rec["u0"], rec["ec_noise"], u_warm=rec["u_warm"],
                                 trace=True)
        assert _eq(out.u, rec["u"])
        assert _eq(out.n_scp, rec["n_scp"])


def test_rollout_is_reproducible_from_the_seed(rollouts):
    ro = rollouts
    for a, b, c in zip(ro.runs["seed1"], ro.runs["seed1_again"], ro.runs["seed2"]):
        for k in STATE_KEYS + ("ec_noise",):
            assert _eq(a[k], b[k]), k
        assert not _eq(a["path"], c["path"])
        assert not _eq(a["ec_noise"], c["ec_noise"])
        assert not _eq(a["u"], c["u"])


def test_rollout_does_not_depend_on_the_sharding(rollouts):
    ro = rollouts
    for i, whole in enumerate(ro.runs["seed1"]):
        for k in STATE_KEYS + ("ec_noise",):
            parts = torch.cat([ro.runs["half0"][i][k], ro.runs["half2"][i][k]])
            assert _eq(whole[k], parts), (i, k)


def test_rollout_without_a_seed_is_the_noise_free_rollout(rollouts, gpu):
    """No seed on an is_noise=False scenario: every step is the noise-free entry points
    on its own inputs, bitwise, and the records carry no noise; with scenario.model.is_noise
    set, a seedless reset raises instead of running noise-free."""
    from scpqp.rollout import ClosedLoopBatch
    ro = rollouts
    for name in ("seedless", "seed_none"):
        for i, rec in enumerate(ro.runs[name]):
            assert "ec_noise" not in rec and "epoch" not in rec
            assert _eq(rec["path"], PL.plant_step(ro.cl.params, rec["x_start"], rec["u_tick"],
                                                  ro.sc.tick_length, device=gpu))
            out = ro.cl.solver.solve(rec["x0"], rec["u0"], None, u_warm=rec["u_warm"], trace=True)
            assert _eq(out.u, rec["u"])
            # tdx = 0 here: the measurement is the step's start state
            x0, dtraj = PL.delay_compensate(ro.cl.params, rec["x_start"].contiguous(), rec["u0"],
                                            ro.sc.delay_x + ro.sc.dt + ro.sc.delay_u, device=gpu)
            assert _eq(x0, rec["x0"]) and _eq(dtraj, rec["delay_traj"])
    for a, b in zip(ro.runs["seedless"], ro.runs["seed_none"]):
        for k in STATE_KEYS:
            assert _eq(a[k], b[k]), k
    noisy = R.circle_scenario(2, Hp=10)
    noisy.model = types.SimpleNamespace(is_noise=True)     # as Scenario(is_noise=True).model
    cl = ClosedLoopBatch(noisy, 2, device=gpu)
    try:
        with pytest.raises(ValueError, match="seed"):
            cl.reset(ro.x_init[:2])
        with pytest.raises(ValueError, match="seed"):
            cl.reset(ro.x_init[:2], seed=None)
        cl.reset(ro.x_init[:2], seed=5)
        assert "ec_noise" in cl.step()
    finally:
        cl.close()
