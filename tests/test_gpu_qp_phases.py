"""The KKT assembly (``assemble``, ``assemble_tiles<2>`` and ``<4>``) and the IPM's vector phases
(``g_apply``, ``gt_apply_fin`` through ``ph_rhs_from_tv``, ``residuals``, ``ph_init_b``,
``newton_back_body`` / ``affine_body`` through ``ph_back_affine_rhs``, ``update_body`` through
``ph_back_update_residuals``) of csrc/scpqp_kernel.h, each run alone by
tests/qp_phases/qp_phases_harness.hip on a given state and held to the 80-bit dense mirror
(tests/qp_phase_mirror.py) at every case of tests/qp_phase_cases.py.

Bounds, in the convention of test_gpu_linalg: u = 2^-53, gamma(p) = p u / (1 - p u), and every
device value obeys |dev - ref| <= c gamma(p) abs, abs being the sum of the absolute values of
the value's terms (the mirror forms it beside the value), p the operations on the value's
longest chain, counted from the kernel's code as if no product were contracted into an FMA,
and c = 2 where the chain holds a quotient formed as ``recip(x) * y`` (each of its operations
then carries at most two roundings, as established there), else 1.  With L3 = ceil(Hb / 3):

  calB x (toeplitz_apply)      L3 + 3      a lane's chain of L3 terms (product, L3 adds), two
                                           combining adds
  calB' y (toeplitz_t_apply)   L3 + 5      the same with two products and an add per term
  (G x)_r (gx_row)             L3 + 7      calB x, then e . ya (2), the second vehicle (1), w x_w (1)
    - h                        + 1
  incident_sum                 V + O       a product and V - 1 + O adds (+ 1 where the
                                           coefficient is itself a product, d_r w_r)
  (G' t)_e, e < N              V + O + L3 + 7   incident_sum, calB', the two bound rows
  (G' t)_N                     ceil(m / 256) + 11   product, a thread's chain, 6 wave and 3
                                           workgroup steps, - t_{mc-1}
  rhs of ph_rhs_from_tv        + 3         - q, + rho dz
  W~ entries                   V + O + 1   2 u^2 Q (2) or d e e (2), V - 1 + O adds
  K_uu                         2 Hb + V + O + 8   a W~ entry, W~ g_b (3), two FMAs per step
                                           over up to Hb steps, the diagonal's terms (4)
  K_Nu (omega row)             V + O + L3 + 6     incident_sum of d w, then calB'
  K_NN                         ceil(m / 256) + 13
  rp = G z + s - h             L3 + 9
  d = lam / s                  2, c = 2
  tv = d rp - (s lam) / s      |d| bound(rp) + 2 gamma(5) (|d rp| + |lam|)
  rd_e                         max(L3 + 7, V + O + 1) + L3 + 9   yb = q_k ya + incident_sum(lam),
                                           calB', the four added terms
  rd_N                         ceil(m / 256) + 12
  gap, pobj                    ceil(mc / 256) + 10;  2 (L3 + 3) + ceil(N / 84) + 18
  ds = -rp - G dz              L3 + 8
  dl = -(rc + lam ds) / s      8, c = 2 (+ |lam / s| bound(ds) where ds is not the stored one)
  a ratio -s / ds              2 (4 with ds's own bound), c = 2
  sigma mu                     the affine step's bound through (s + a ds)(lam + a dl), summed
                               with ceil(mc / 256) + 14 operations, cubed (x 3) and 9 more
  corrector tv                 7, c = 2
  new z, s, lam                the step's bound times the direction, the direction's bound
                               times the step, 2 gamma(2) for the update itself
  ph_init_b                    omega: (G_u z - h) / -w, L3 + 9, its maximum, + 1; s: bound(G_u z)
                               + |w| bound(omega) + gamma(3) abs; the shift 1.5 max(-s), the
                               floor 0.1 max(1, max s + shift) and max(s + shift, floor) carry
                               the bounds of the entries they pick

A site that forms a value from one it has stored (the affine direction, then sigma mu, then
tv, then the right-hand side; the updated point, then its residuals) is checked link by link:
the later value's reference starts from the device's stored earlier one, so no bound has to
carry another's.  Values that hang on an extremum (the step lengths, omega and the shift of
the starting point, max |rp|, max |rd|) take the binding entry's bound; the case table holds
the separation condition that makes that valid (the binding entry leads the runner-up by more
than the two bounds together), asserted here on the device's values and in
tests/test_qp_phases_host.py on the float64 mirror's.

rho: ``assemble`` adds it to every diagonal entry, the omega one included (as the oracle's
polish does), so the mirror's K is P + rho I + G' D G with the full identity.

Every test prints ``qp_phases_gpu`` lines with its figures; profiles/qp_phases_gpu_tests.txt is
one run's output."""
import numpy as np
import pytest

import qp_phase_cases as QC
import qp_phase_mirror as QM
import qp_phases_harness as QH

pytestmark = pytest.mark.gpu

UNITS = tuple(QC.SHAPES)
UNIT_IDS = ["unit%d_k%s" % (u, "".join(str(v) for v in QH.KERNELS[u])) for u in UNITS]
_runs = {}


def device_run(unit):
    """One launch per unit with every case of the table: [(case, Result)]."""
    if unit not in _runs:
        cases = QC.unit_cases(unit)
        res = QH.run(unit, [c[1:] for c in cases])
        _runs[unit] = list(zip(cases, res))
    return _runs[unit]


def dev_outputs(r, site):
    """What a site left behind, in the names qp_phase_cases.check reads."""
    p = r.plan
    vec = lambda *ks: {k: r.get(k, p.mc) for k in ks}
    if site == QH.S_A:
        return {"K": r.packed(), "Wt": r.get("Wt", 4 * p.Hb * p.nb).reshape(p.Hb, p.nb, 4)}
    if site in (QH.S_G, QH.S_GH):
        return vec("rp")
    if site == QH.S_T:
        return {"rhs": r.get("rhs", p.n)}
    if site == QH.S_R:
        return dict(vec("rp", "dd", "tv"), rd=r.get("rd", p.n), ret=r.ret)
    if site == QH.S_I:
        return dict(vec("s", "lam"), om=r.get("z", p.n)[p.N])
    if site == QH.S_B:
        return dict(vec("sa", "la", "tv"), rhs=r.get("rhs", p.n), smu=r.ret[0])
    return dict(vec("s", "lam", "sa", "la", "rp", "dd", "tv"), z=r.get("z", p.n), rd=r.get("rd", p.n), ret=r.ret)


@pytest.mark.parametrize("unit", UNITS, ids=UNIT_IDS)
def test_every_site_within_its_bound(gpu, unit):
    """Every value of every site of every case within its bound of the 80-bit mirror, and
    every separation condition holds on the device's values."""
    worst, over, unsep = {}, [], []
    run = device_run(unit)
    for (key, V, O, HM, Hb, site, st, par, args), r in run:
        out, sep = QC.check(st, par, site, args, dev_outputs(r, site), direction_stored=r.plan.slots == 0)
        for k, v in out.items():
            w = worst.setdefault((site, key[0]), {})
            if not v <= w.get(k, (-1.0,))[0]:
                w[k] = (v, key[1:3])
            if not v <= 1.0:
                over.append((key, k, v))
        unsep += [(key, k) for k, ok in sep.items() if not ok]
    for (site, fam), w in sorted(worst.items()):
        figs = ", ".join(f"{k} {v[0]:.3f}" for k, v in w.items())
        top = max(w.values(), key=lambda v: v[0] if v[0] == v[0] else np.inf)
        print(f"qp_phases_gpu unit {unit} {QH.KERNELS[unit]} site {QH.SITES[site]} family {fam}: "
              f"largest |dev - ref| / bound per value: {figs}; largest at {top[1]}")
    print(f"qp_phases_gpu unit {unit}: {len(run)} cases in one launch")
    assert not over, over[:10]
    assert not unsep, unsep[:10]


@pytest.mark.parametrize("unit", UNITS, ids=UNIT_IDS)
def test_nothing_else_is_written(gpu, unit):
    """Outside what a site owns (Plan.owned) the LDS and the workspace slice are bitwise what
    they were: the other arrays, the padding and canaries past every array, the rest of the
    launch's LDS."""
    n = 0
    for (key, V, O, HM, Hb, site, st, par, args), r in device_run(unit):
        w = r.written_outside(site)
        assert w.size == 0, ("written outside the site's own", key, w[:8], r.lds_img)
        n += 1
    print(f"qp_phases_gpu unit {unit}: {n} cases wrote nothing outside what their site owns")


@pytest.mark.parametrize("unit", UNITS, ids=UNIT_IDS)
def test_g_and_its_transpose_agree(gpu, unit):
    """<G x, t> against <x, G' t> from the device's own g_apply and ph_rhs_from_tv on the same
    state (x = z, t = tv), within the two sites' bounds: a cross-check that does not go through
    the mirror's values."""
    by = {}
    for case, r in device_run(unit):
        key, site = case[0], case[5]
        if site in (QH.S_G, QH.S_T) and key[0] != "one-hot":
            by.setdefault(key[:3], {})[site] = (case, r)
    worst = 0.0
    for k3, d in by.items():
        (key, V, O, HM, Hb, site, st, par, args), rg = d[QH.S_G]
        rt = d[QH.S_T][1]
        D = QC.dense(st, par, QM.F80)
        T = QM.F80
        x, t, dz = (np.asarray(st[k], dtype=T).reshape(-1) for k in ("z", "tv", "dz"))
        gx = rg.get("rp", D.mc).astype(T)
        gtt = rt.get("rhs", D.n).astype(T) + D.q - T(args["rho"]) * dz
        bg = QM.site_gapply(D, st, False)["rp"][1]
        bt = QM.site_rhs_from_tv(D, st, args["rho"])["rhs"][1]
        bound = np.abs(t) @ bg + np.abs(x) @ bt
        ratio = float(abs(gx @ t - x @ gtt) / bound)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k3, ratio)
    assert by
    print(f"qp_phases_gpu unit {unit}: |<G x, t> - <x, G' t>| / (the two bounds) max {worst:.3f} "
          f"over {len(by)} states")
