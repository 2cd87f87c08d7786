"""The drive truth on the device (include/scpqp_drive.h).

Kernel: ideal rows against ``plant_step(..., truth=)`` with ``x_start[4] = a_eff`` bitwise in the
three noise forms; the case table of tests/drive_cases.py against the CPU mirror
(tests/drive_mirror.py) at the tolerance derived in tests/test_drive_host.py; held speeds exactly
zero; bad rows; split batches; the sampler against the mirror.

Rollout: ideal rows, and rows that do what the ideal ones do without being them (limits that
are never reached, which take the drive's kernel), against ``governor=`` / ``right_of_way=``
alone; a lagged drive with the hold rule on ``governor_cases.stop_scene``, replayed through the
mirror.

Equality of float64 tensors is equality of values with NaN equal to NaN: the ideal a_eff is
1 * a_cmd + 0, which turns a command of -0.0 into +0.0, as the header says."""
import types

import numpy as np
import pytest
import torch

import drive_cases as DC
import drive_mirror as DM
import governor_cases as GC
import yield_cases as YC
from oracle import scp_reference as R
from scpqp import drive as DRV
from scpqp import governor as GOV
from scpqp import obstacles as OB
from scpqp import plant as PL
from scpqp import truth as TR
from scpqp import yielding as YLD

pytestmark = pytest.mark.gpu


def _eq(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return bool(torch.equal(a, b))


def _np(t):
    return t.detach().cpu().numpy()


def _params():
    d = DC.inputs()
    return PL.plant_params(d["lf"], d["lr"])


def _form_kw(form, b0=0, b1=DC.B):
    if form == "pair":
        return dict(noise=DC.inputs()["pair"][b0:b1])
    if form == "seeded":
        seed, sigma, epoch, b_off = DC.SEEDED
        return dict(rng=PL.NoiseStream(seed, sigma, epoch, b_off + b0))
    return {}


def device_step(gpu, form, drive=None, a_cmd=None, b0=0, b1=DC.B):
    d = DC.inputs()
    drive = d["drive"] if drive is None else drive
    a_cmd = d["a_cmd"] if a_cmd is None else a_cmd
    return PL.plant_step(_params(), d["x_start"][b0:b1], d["u_tick"][b0:b1], DC.TICK, h_max=DC.H_MAX,
                         device=gpu, truth=d["truth"][b0:b1], drive=drive[b0:b1],
                         a_cmd=a_cmd[b0:b1], **_form_kw(form, b0, b1))


@pytest.fixture(scope="module")
def table(gpu):
    """The case table on the device, once per form."""
    out = {form: device_step(gpu, form) for form in DC.FORMS}
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", DC.FORMS)
def test_ideal_rows_are_the_truth_plant_step_at_a_eff_bitwise(gpu, form):
    d = DC.inputs()
    good = np.isfinite(d["a_cmd"])
    a_cmd = np.where(good, d["a_cmd"], -0.7)
    drive = DRV.ideal(DC.B, DC.V, device=gpu)
    xs = d["x_start"].copy()
    xs[..., 4] = 1.0 * a_cmd + 0.0                            # a_eff of the ideal row
    kw = _form_kw(form)
    want = PL.plant_step(_params(), xs, d["u_tick"], DC.TICK, h_max=DC.H_MAX, device=gpu,
                         truth=d["truth"], **kw)
    got = device_step(gpu, form, drive=drive, a_cmd=a_cmd)
    assert not torch.isnan(got).any()
    assert _eq(got, want)
    # x_start[4] is not read by a lane without a lag
    assert not _eq(got, PL.plant_step(_params(), d["x_start"], d["u_tick"], DC.TICK, h_max=DC.H_MAX,
                                      device=gpu, truth=d["truth"], **kw))
    # without a truth the nominal rows are filled in
    nominal = PL.plant_step(_params(), xs, d["u_tick"], DC.TICK, h_max=DC.H_MAX, device=gpu, **kw)
    bare = PL.plant_step(_params(), d["x_start"], d["u_tick"], DC.TICK, h_max=DC.H_MAX, device=gpu,
                         drive=drive, a_cmd=a_cmd, **kw)
    assert _eq(bare, nominal)


@pytest.mark.parametrize("form", DC.FORMS)
def test_every_case_matches_the_mirror(table, form):
    got, want = _np(table[form]), DC.mirror(form)
    r = DC.ratio(got, want)
    per = {}
    for i, kind in enumerate(DC.KINDS):
        b, v = i // DC.V, i % DC.V
        if i not in DC.BAD:
            per[kind] = max(per.get(kind, 0.0), DC.ratio(got[b, v], want[b, v]))
    print(f"drive table, {form}: worst |device - mirror| / (1 + |mirror|) = {r:.3g} "
          f"(tolerance {DC.TOL:.3g})")
    print("  per kind:", {k: f"{v:.2g}" for k, v in per.items()})
    assert r <= DC.TOL


@pytest.mark.parametrize("form", DC.FORMS)
def test_held_speeds_are_exactly_zero(table, form):
    got, want = _np(table[form]), DC.mirror(form)
    zero = want[..., 3] == 0.0
    # hold_early 8 ticks, hold_late 2, hold_lag_cross 5, hold_lag_released 3, hold_released's start
    assert zero.sum() == 19
    assert np.array_equal(got[..., 3] == 0.0, zero)
    assert not np.signbit(got[..., 3][zero]).any()
    for kind in DC.CROSSING:
        (b, v), = DC.rows_of(kind)
        assert got[b, v, -1, 3] == 0.0
    (b, v), = DC.rows_of("free_early")
    assert (got[b, v, 1:, 3] < 0.0).all()                     # HOLD = 0 on the same lane


@pytest.mark.parametrize("form", ["free", "seeded"])
def test_bad_rows_are_nan_and_their_neighbours_are_untouched(gpu, table, form):
    d = DC.inputs()
    got = table[form]
    mended_d, mended_a = d["drive"].copy(), d["a_cmd"].copy()
    for r in DC.BAD:
        b, v = r // DC.V, r % DC.V
        assert bool(torch.isnan(got[b, v]).all())            # k = 0 included
        mended_d[b, v], mended_a[b, v] = DM.IDEAL_ROW, -1.0
    base = device_step(gpu, form, drive=mended_d, a_cmd=mended_a)
    assert not torch.isnan(base).any()
    ok = torch.ones((DC.B, DC.V), dtype=torch.bool)
    for r in DC.BAD:
        ok[r // DC.V, r % DC.V] = False
    assert not torch.isnan(got[ok]).any()
    assert _eq(got[ok], base[ok])
    # the truth row's own bad rule stays
    truth = d["truth"].copy()
    truth[3, 1, 2] = 0.0
    t = PL.plant_step(_params(), d["x_start"], d["u_tick"], DC.TICK, h_max=DC.H_MAX, device=gpu,
                      truth=truth, drive=mended_d, a_cmd=mended_a, **_form_kw(form))
    ok = torch.ones((DC.B, DC.V), dtype=torch.bool)
    ok[3, 1] = False
    assert bool(torch.isnan(t[3, 1]).all()) and _eq(t[ok], base[ok])


@pytest.mark.parametrize("form", DC.FORMS)
def test_a_split_batch_gives_what_the_whole_gives(gpu, table, form):
    parts = [device_step(gpu, form, b0=b0, b1=b1) for b0, b1 in ((0, 5), (5, DC.B))]
    assert _eq(torch.cat(parts), table[form])


def test_python_side_refuses_what_does_not_fit(gpu):
    d = DC.inputs()
    p = _params()
    args = (p, d["x_start"], d["u_tick"], DC.TICK)
    with pytest.raises(ValueError, match="drive and a_cmd"):
        PL.plant_step(*args, device=gpu, drive=d["drive"])
    with pytest.raises(ValueError, match="drive and a_cmd"):
        PL.plant_step(*args, device=gpu, a_cmd=d["a_cmd"])
    with pytest.raises(ValueError, match=r"\[B, nVeh, 6\]"):
        PL.plant_step(*args, device=gpu, drive=d["drive"][..., :5], a_cmd=d["a_cmd"])
    with pytest.raises(ValueError, match=r"\[B, nVeh, 6\]"):
        PL.plant_step(*args, device=gpu, drive=d["drive"], a_cmd=d["a_cmd"][:, :1])
    with pytest.raises(ValueError, match=r"\[B, nVeh, 5\]"):
        PL.plant_step(*args, device=gpu, drive=d["drive"], a_cmd=d["a_cmd"], truth=d["truth"][:3])
    with pytest.raises(ValueError, match="not both"):
        PL.plant_step(*args, device=gpu, drive=d["drive"], a_cmd=d["a_cmd"], noise=d["pair"],
                      rng=PL.NoiseStream(1))


# ---------------------------------------------------------------------------
# 2. the sampler against the mirror
# ---------------------------------------------------------------------------
def _dists(seed, b_offset=0):
    d = DRV.DriveDist(3, seed, b_offset)
    d.fixed("tau_a", 0.2).uniform("tau_a", 0.15, 0.1, 0.3).uniform("gain_a", 0.2)
    d.normal("bias_a", 0.3, -0.5, 0.5).fixed("b_max", [3.0, 2.5, 2.0]).normal("b_max", 1.0, lo=1.5)
    d.fixed("hold", 1)
    m = DM.Dist(3, seed, b_offset)
    m.fixed(DM.TAU_A, 0.2).set(DM.TAU_A, DM.UNIFORM, 0.15, 0.1, 0.3).set(DM.GAIN_A, DM.UNIFORM, 0.2)
    m.set(DM.BIAS_A, DM.NORMAL, 0.3, -0.5, 0.5)
    m.mean[DM.B_MAX] = [3.0, 2.5, 2.0]
    m.set(DM.B_MAX, DM.NORMAL, 1.0, 1.5).fixed(DM.HOLD, 1.0)
    return d, m


def test_sampler_matches_the_mirror(gpu):
    """FIXED and UNIFORM fields bitwise (the uniform is exact and mean + spread * xi is two
    roundings on both sides); NORMAL fields within the tolerance of a normal draw of
    tests/test_gpu_noise.py::test_raw_draws_match_the_mirror (64 * 2^-52 * 10) times spread: what
    tests/test_gpu_truth.py holds the truth sampler to."""
    seed, b_off, B = 0x123456789ABCDEF, 1000, 64
    d, m = _dists(seed, b_off)
    got = _np(d.sample(B, device=gpu))
    want = DM.sample(m, B)
    assert got.shape == want.shape == (B, 3, 6)
    for f in (DM.TAU_A, DM.GAIN_A, DM.A_MAX, DM.HOLD):
        assert np.array_equal(got[..., f], want[..., f]), f
    assert np.all(got[..., DM.A_MAX] == np.inf) and np.all(got[..., DM.HOLD] == 1.0)
    atol = 64 * 2.0 ** -52 * 10
    for f, spread in ((DM.BIAS_A, 0.3), (DM.B_MAX, 1.0)):
        err = np.abs(got[..., f] - want[..., f]).max()
        print(f"field {f}: max |device - mirror| = {err:.3e} (atol {atol * spread:.3e})")
        assert err <= atol * spread
    # clamps are honoured, and reached
    assert got[..., DM.TAU_A].min() == 0.1 and got[..., DM.TAU_A].max() == 0.3
    assert got[..., DM.BIAS_A].min() == -0.5 and got[..., DM.BIAS_A].max() == 0.5
    assert got[..., DM.B_MAX].min() == 1.5
    assert np.all(np.abs(got[..., DM.GAIN_A] - 1.0) <= 0.2) and np.ptp(got[..., DM.GAIN_A]) > 0.3
    DRV.validate(got, DC.H_MAX)
    assert not any(DM.is_bad(r, 0.0) for r in got.reshape(-1, 6))


def test_sampler_does_not_depend_on_the_sharding(gpu):
    d, _ = _dists(99)
    whole = d.sample(6, device=gpu)
    parts = [d.with_offset(o).sample(3, device=gpu) for o in (0, 3)]
    assert _eq(whole, torch.cat(parts))
    assert not _eq(parts[0], parts[1])
    assert not _eq(whole, _dists(100)[0].sample(6, device=gpu))
    with pytest.raises(RuntimeError, match="hold"):
        bad = _dists(1)[0]
        bad.mean[DM.HOLD, 1] = 0.5
        bad.sample(2, device=gpu)


def test_fill_ideal_is_bitwise(gpu):
    for B, V in ((1, 1), (5, 3), (40, 16)):
        got = _np(DRV.ideal(B, V, device=gpu))
        assert np.array_equal(got, np.broadcast_to(DM.IDEAL_ROW, (B, V, 6)))
        assert DRV.is_ideal(got)


# ---------------------------------------------------------------------------
# 3. rollout, ideal rows
# ---------------------------------------------------------------------------
def _snapshot(cl):
    return types.SimpleNamespace(hist=[{k: v.clone() for k, v in h.items()
                                        if isinstance(v, torch.Tensor)} for h in cl.history],
                                 metrics=cl.metrics(), control=cl.control.clone(),
                                 state=cl.state.clone())


def _same_runs(a, b, drive_ran):
    """Paths, control, every shared record key and the metrics bit for bit.  ``drive_ran``: b ran
    the drive's kernel: it alone records accel_real, and its state differs in column 4, which
    holds the realised acceleration: the previous step's command."""
    assert len(a.hist) == len(b.hist)
    for i in range(len(a.hist)):
        assert set(b.hist[i]) - set(a.hist[i]) == ({"accel_real"} if drive_ran else set())
        assert set(a.hist[i]) <= set(b.hist[i]) and "path" in a.hist[i] and "accel_cmd" in a.hist[i]
        for k in a.hist[i]:
            assert _eq(a.hist[i][k], b.hist[i][k]), (i, k)
    assert _eq(a.control, b.control)
    for k, v in a.metrics.items():
        assert torch.equal(v, b.metrics[k]), k
    cols = [0, 1, 2, 3, 5]
    assert _eq(a.state[..., cols], b.state[..., cols])
    if drive_ran:
        prev = b.hist[-2]["accel_cmd"]
        assert _eq(b.state[..., 4], prev + 0.0) and _eq(b.hist[-1]["accel_real"], prev + 0.0)
        assert _eq(a.state[..., 4], a.hist[-1]["accel_cmd"])
    else:
        assert _eq(a.state, b.state)


def _ideal_against_alone(gpu, cl, x_init, steps, nV, **reset_kw):
    B = x_init.shape[0]
    runs = []
    for drive in (None, DRV.ideal(B, nV, device=gpu),
                  DRV.rows(B, nV, a_max=1e30, b_max=1e30, device=gpu)):
        cl.reset(x_init, drive=drive, **reset_kw)
        assert (cl.drive_rows is None) == (drive is None or DRV.is_ideal(drive))
        assert (cl.a_cmd is None) == (cl.drive_rows is None)
        cl.run(steps)
        runs.append(_snapshot(cl))
    _same_runs(runs[0], runs[1], drive_ran=False)     # nothing allocated, nothing launched
    _same_runs(runs[0], runs[2], drive_ran=True)      # the drive's kernel, to the same effect
    return runs


@pytest.mark.parametrize("how", ["plain", "delay_x", "sensor", "estimator"])
def test_rollout_ideal_drive_is_the_governed_rollout_on_the_stop_scene(gpu, how):
    from scpqp import estimator as EST
    from scpqp import sensing as SE
    from scpqp.rollout import ClosedLoopBatch
    sc, x_init, kw = GC.stop_scene(delay_x=0.1 if how != "plain" else 0.0)
    B = GC.STOP_B
    extra = dict(obstacles=OB.nominal(sc, B, device=gpu), governor=GOV.rows(B, 1, device=gpu, **kw))
    if how in ("sensor", "estimator"):
        srows = SE.nominal(B, 1, device=gpu)
        srows[..., SE.FIELDS.index("sig_pos")] = 0.02
        extra.update(sensing=srows, sense_seed=3)
        if how == "estimator":
            extra.update(estimator=EST.matched(srows))
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = _ideal_against_alone(gpu, cl, x_init, GC.STOP_STEPS, 1, **extra)
    if how == "plain":
        assert (runs[2].metrics["first_collision_tick"] < 0).all()
        assert (runs[2].hist[0]["accel_cmd"] == -kw["a_brake"]).all()
        # refused before anything is launched: no commander, a bad row, a shape that does not fit
        n = len(cl.history)
        with pytest.raises(ValueError, match="governor= or right_of_way="):
            cl.reset(x_init, obstacles=extra["obstacles"], drive=DRV.rows(B, 1, tau=0.3, device=gpu))
        with pytest.raises(ValueError, match="8 \\* h_max"):
            cl.reset(x_init, drive=DRV.rows(B, 1, tau=0.01, device=gpu), **extra)
        with pytest.raises(ValueError, match="hold"):
            cl.reset(x_init, drive=DRV.rows(B, 1, hold=2, device=gpu), **extra)
        with pytest.raises(ValueError, match=r"\[B, nVeh, 6\]"):
            cl.reset(x_init, drive=DRV.rows(B + 1, 1, device=gpu), **extra)
        assert len(cl.history) == n
    cl.close()


def test_rollout_ideal_drive_with_right_of_way_on_the_crossing_scene(gpu):
    from scpqp.rollout import ClosedLoopBatch
    scs, variant_of, x_init, ranks = YC.crossing_scene()
    B = YC.CROSS_B
    rows = YLD.from_governor(GOV.rows(B, 2, device=gpu, **YC.CROSS_KW), ranks)
    cl = ClosedLoopBatch(scs[0], B, device=gpu, keep_path=True, metrics=True, variants=scs,
                         variant_of=variant_of)
    runs = _ideal_against_alone(gpu, cl, x_init, YC.CROSS_STEPS, 2, right_of_way=rows)
    cl.close()
    acc = torch.stack([h["accel_cmd"] for h in runs[2].hist])
    assert (acc < 0).any() and "gov_who" in runs[2].hist[0]


def test_rollout_ideal_drive_on_four_steps_of_c2(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc = R.circle_scenario(4, Hp=20)
    B, steps = 4, 4
    rng = np.random.default_rng(12)
    x_init = np.array(sc.x0, float)[None] + rng.standard_normal((B, sc.nVeh, 6)) * np.array(
        [0.05, 0.05, 0.005, 0.02, 0.0, 0.002])
    gov = GOV.rows(B, 4, v_ref=4.0, a_acc=1.0, a_brake=3.0, k_v=0.5, look=20, band=2.0, device=gpu)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = _ideal_against_alone(gpu, cl, x_init, steps, 4, seed=1,
                                right_of_way=YLD.from_governor(gov, 5))
    cl.close()
    kc = torch.stack([h["gov_k_conf"] for h in runs[2].hist])
    assert (kc >= 0).any()                                    # the comparison is not an empty one


# ---------------------------------------------------------------------------
# 4. rollout, a lagged drive with the hold rule
# ---------------------------------------------------------------------------
LAG_TAU = 0.3
REPLAY_TICKS = (0, 1, 10, 25, 40)


@pytest.fixture(scope="module")
def lagged(gpu):
    from scpqp.rollout import ClosedLoopBatch
    sc, x_init, kw = GC.stop_scene()
    B = GC.STOP_B
    extra = dict(obstacles=OB.nominal(sc, B, device=gpu), governor=GOV.rows(B, 1, device=gpu, **kw))
    drive = DRV.rows(B, 1, tau=LAG_TAU, hold=1, device=gpu)
    cl = ClosedLoopBatch(sc, B, device=gpu, keep_path=True, metrics=True)
    runs = {}
    for name, dr in (("ideal", None), ("lagged", drive)):
        cl.reset(x_init, drive=dr, **extra)
        cl.run(GC.STOP_STEPS)
        runs[name] = _snapshot(cl)
    torch.cuda.synchronize()
    yield types.SimpleNamespace(sc=sc, B=B, x_init=x_init, drive=drive, runs=runs)
    cl.close()


def test_lagged_rollout_calls_the_plant_as_defined(lagged):
    """Every step's path from its recorded x_start and u_tick and the command in force (the
    previous step's accel_cmd; x_init's column 4 for step 0) through the mirror, at the ticks
    REPLAY_TICKS of every step (a lane restarts from x_start, so a tick stands alone)."""
    ro, sc = lagged, lagged.sc
    truth = np.broadcast_to(TR.nominal_rows(sc)[None], (ro.B, 1, 5))
    drive = _np(ro.drive)
    worst = 0.0
    for i, rec in enumerate(ro.runs["lagged"].hist):
        cmd = ro.x_init[:, :, 4] if i == 0 else _np(ro.runs["lagged"].hist[i - 1]["accel_cmd"])
        ks = list(REPLAY_TICKS)
        assert ks[-1] == rec["path"].shape[2] - 1
        want = np.stack([DM.plant_step(_np(rec["x_start"]), _np(rec["u_tick"])[:, :, [k, k]], truth, cmd,
                                       drive, k * sc.tick_length, PL.H_MAX)[:, :, 1]
                         if k else _np(rec["x_start"]) for k in ks], axis=2)
        r = DC.ratio(_np(rec["path"])[:, :, ks], want)
        worst = max(worst, r)
        assert r <= DC.TOL, (i, r)
        # the realised acceleration is continuous across steps and recorded at the step's end
        assert _eq(rec["accel_real"], rec["path"][:, :, -1, 4])
        if i:
            assert _eq(rec["x_start"][:, :, 4], ro.runs["lagged"].hist[i - 1]["accel_real"])
            # the controller planned from the command, not from the realised acceleration
            assert _eq(rec["x0"][:, :, 4], ro.runs["lagged"].hist[i - 1]["accel_cmd"])
    print(f"lagged rollout replayed through the mirror: worst figure {worst:.3g} (tolerance {DC.TOL:.3g})")


def test_lagged_rollout_never_reverses_and_stops_no_earlier(lagged):
    ro = lagged
    speed = {k: torch.stack([h["path"][:, :, :, 3] for h in ro.runs[k].hist]) for k in ro.runs}
    x_end = {k: ro.runs[k].hist[-1]["path"][:, 0, -1, 0] for k in ro.runs}
    first = ro.runs["lagged"].metrics["first_collision_tick"]
    print("stop scene, TAU_A = 0.3, HOLD = 1: stopping points", x_end["lagged"].tolist(),
          "against the ideal drive's", x_end["ideal"].tolist())
    print("  end speeds", speed["lagged"][-1, :, 0, -1].tolist(), "first collision ticks (reported, "
          "not asserted)", first.tolist(), "min gap", ro.runs["lagged"].metrics["min_gap_obs"].flatten().tolist())
    assert (speed["lagged"] >= 0.0).all()                     # no realised speed below zero
    assert (x_end["lagged"] >= x_end["ideal"]).all()          # it stops no earlier
    assert (x_end["lagged"] > x_end["ideal"] + 0.1).any()     # and the lag is felt
    real = torch.stack([h["accel_real"] for h in ro.runs["lagged"].hist])
    cmd = torch.stack([h["accel_cmd"] for h in ro.runs["lagged"].hist])
    assert not _eq(real[1:], cmd[:-1])                        # realised is not commanded
