"""The case table of the QP-phase tests (tests/test_qp_phases_host.py on the CPU,
tests/test_gpu_qp_phases.py on the GPU): shapes per harness unit, and the states each shape
is run on, all generated on the host from a fixed seed or taken from the oracle.

Families
  random   seeded; d = lam / s in [0.5, 2], so every row carries weight and a dropped or
           misplaced term shows at full size; rowW of both magnitudes (0.1 .. 1 and
           1e-3 .. 1e-2); obstacle rows where the unit is run-time shaped.
  oracle   the first QP of a dispatch_cases row: g from ``R.linearise``, the factored rows from
           the oracle's rows, and (z, s, lam) with its directions at the first, a middle and
           the last iteration of the restated IPM (linalg_cases.ipm_systems).  d spans many
           orders of magnitude: what the solver actually runs.  Two states per iterate: the
           predictor's (dz = the affine dx: every site but the update) and the corrector's
           (dz = the corrected dx, (sa, la) = the affine (ds, dl): the update).
  one-hot  (assembly only, small shapes) d = e_r for each collision row r in turn, with
           Q = Qf = R = 0 and rho = 0: K is one row's outer product, so every row's place in
           every W~ block and tile has a case of its own.

Shapes are (V, O, Hb) at slot horizon HM, the smallest that reach each edge (SHAPES says which);
every unit's plan accepts them within the LDS limit, so none stands in for another.  The
oracle family's cost gradient ``qs`` is the oracle's scaled q (the kernel forms it in
setup_problem, outside these phases)."""
import functools

import numpy as np

import dispatch_cases as DC
import qp_phase_mirror as QM
import qp_phases_harness as QH

SEED = 20250301

# unit -> [(V, O, HM, Hb, what the shape is there for)]
SHAPES = {
    1: [(1, 0, 3, 3, "m = 0"), (1, 1, 1, 1, "Hb = 1, n = 2"), (3, 1, 7, 7, "V Hb = 21: one wave's share"),
        (2, 0, 11, 11, "V Hb = 22"), (3, 0, 21, 21, "V Hb = 63"), (1, 3, 51, 51, "mc = 256"),
        (1, 6, 32, 32, "mc = 257"), (2, 1, 12, 5, "Hb < HM")],
    2: [(4, 0, 20, 20, "c2: compile-time shape, tv in pb's storage, two row slots")],
    3: [(4, 0, 30, 30, "class 6"), (4, 0, 30, 20, "class 5"), (4, 0, 30, 10, "class 4"),
        (4, 0, 30, 21, "V Hb = 84: one pass, run-time shape 2"), (4, 0, 30, 1, "Hb = 1")],
    4: [(7, 0, 18, 18, "4 x 4 tiles"), (7, 0, 18, 17, "4 x 4 tiles, partial"), (7, 0, 18, 9, "2 x 2 tiles, partial"),
        (7, 0, 18, 4, "2 x 2 tiles"), (5, 0, 17, 17, "V Hb = 85: a second pass of one output"),
        (3, 2, 6, 6, "obstacle rows on a workspace plan")],
    5: [(8, 0, 30, 30, "4 x 4 tiles"), (8, 0, 30, 15, "528 tiles: just over the switch"),
        (8, 0, 30, 12, "300 tiles: under it"), (8, 0, 30, 6, "2 x 2 tiles"), (8, 0, 30, 1, "Hb = 1")],
    6: [(8, 0, 30, 30, "c3: compile-time shape")],
}
# the tile size assemble takes at every shape of the workspace-factor units
TILES = {(4, 7, 18): 4, (4, 7, 17): 4, (4, 7, 9): 2, (4, 7, 4): 2, (4, 5, 17): 2, (4, 3, 6): 2,
         (5, 8, 30): 4, (5, 8, 15): 4, (5, 8, 12): 2, (5, 8, 6): 2, (5, 8, 1): 2, (6, 8, 30): 4}
# unit -> [(scenario, V, HM, start scale, horizons, problem, Hb)]: dispatch_cases inputs
ORACLE = {
    1: [("frog", 1, 10, 1.0, None, 0, 10)],
    2: [("circle", 4, 20, 1.0, None, 0, 20)],
    3: [("circle", 4, 30, 1.0, (10, 20, 30), b, h) for b, h in ((0, 10), (1, 20), (2, 30))],
    4: [("circle", 7, 18, 1.1, (18, 9, 4), b, h) for b, h in ((0, 18), (1, 9), (2, 4))],
    5: [("circle", 8, 30, 1.0, (30, 15, 6), b, h) for b, h in ((0, 30), (1, 15), (2, 6))],
    6: [("circle", 8, 30, 1.0, None, 0, 30)],
}
ORACLE_STAGES = {u: ("first", "middle", "last") for u in (1, 2, 3, 4, 5)}
ORACLE_STAGES[6] = ("middle",)     # its 80-bit dense products are the slow ones on the CPU
# one-hot: (unit, V, O, HM, Hb)
ONE_HOT = [(1, 3, 1, 7, 7), (3, 4, 0, 30, 10), (4, 3, 2, 6, 6), (4, 7, 0, 18, 4)]


def random_params(V):
    return {"uLim": 0.5, "slackW": 1e5, "polDelta": 1e-6, "polRho": 1e-6,
            "Q": 1.0 + 0.125 * np.arange(V), "Qf": 2.0 + 0.25 * np.arange(V), "R": 0.5 + 0.0625 * np.arange(V)}


def zero_cost_params(V):
    p = random_params(V)
    p["Q"], p["Qf"], p["R"] = np.zeros(V), np.zeros(V), np.zeros(V)
    return p


@functools.lru_cache(maxsize=None)
def _params(kind, V):
    return random_params(V) if kind == "random" else zero_cost_params(V)


@functools.lru_cache(maxsize=None)
def random_state(V, O, Hb, tag=0):
    rng = np.random.default_rng([SEED, V, O, Hb, tag])
    N, n, m, mc = QH.dims(V, O, Hb)
    ang = rng.uniform(0, 2 * np.pi, m)
    E = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rng.uniform(0.5, 2.0, m)[:, None]
    W = -np.where(rng.uniform(size=m) < 0.5, rng.uniform(0.1, 1.0, m), rng.uniform(1e-3, 1e-2, m))
    s = rng.uniform(0.5, 2.0, mc)
    d = rng.uniform(0.5, 2.0, mc)
    z = 0.5 * rng.standard_normal(n)
    z[N] = rng.uniform(0.5, 2.0)
    st = dict(V=V, O=O, Hb=Hb, g=0.3 * rng.standard_normal((V, Hb, 2)), rowE=E, rowW=W,
              rowH=rng.standard_normal(m), z=z, dz=0.3 * rng.standard_normal(n), s=s, lam=d * s,
              rp=rng.standard_normal(mc), dd=d, sa=0.5 * rng.standard_normal(mc),
              la=0.5 * rng.standard_normal(mc), tv=rng.standard_normal(mc), rd=rng.standard_normal(n),
              qs=rng.standard_normal(N))
    mu = float(st["s"] @ st["lam"]) / mc
    st["args"] = dict(rho=_params("random", V)["polRho"], mu=mu, smu=0.1 * mu, eta=max(0.99, 1.0 - mu))
    return st


def one_hot_states(V, O, Hb):
    """d = e_r for every collision row r of the shape's random state."""
    base = random_state(V, O, Hb)
    m = QH.dims(V, O, Hb)[2]
    out = []
    for r in range(m):
        st = dict(base)
        st["dd"] = np.zeros_like(base["dd"])
        st["dd"][r] = 1.0
        out.append(st)
    return out


# ---------------------------------------------------------------------------------------
# the oracle family
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_problem(src):
    """Structured state of the first QP of problem b of a dispatch_cases input: (base state
    without an iterate, parameters, the oracle's scaled dense (P, q, G, h), the trace-style
    rows [m, 4])."""
    DC._paths()
    from oracle import scp_reference as R
    kind, V, HM, scale, hps, b, Hb = src
    sc, bt = DC.make_inputs(kind, V, HM, scale, hps)
    job = DC.oracle_jobs(kind, V, sc, bt)[b]
    assert job[3] == Hb, (src, job[3])
    qp = DC.first_qp_job(job)
    _, _, _, hp, x0, u0, ec, obst = job
    p = R.make_problem(sc, x0, u0, ec, Hp=hp, obst=obst if sc.nObst else None)
    lin = R.linearise(p, "structured")
    r = R.scp_solve(p, mode="structured", keep_history=True, max_scp=1)
    hh = r.history[0]
    O = sc.nObst
    N = V * Hb
    pos = R.positions(lin, hh["u_lin"], V, Hb)
    A, bb = hh["A"], hh["b"]
    rows = np.zeros((A.shape[0], 4))
    for ri, (i, j, o, k) in enumerate(R.row_list(V, Hb, O)):
        d = pos[i, k] - (pos[j, k] if j >= 0 else p.obst[o, :, k])
        nrm = np.sqrt(np.sum((A[ri, :N] * p.u_lim) ** 2) + 1.0)
        rows[ri] = 2 * d[0] * p.u_lim / nrm, 2 * d[1] * p.u_lim / nrm, -1.0 / nrm, bb[ri] / nrm
    par = {"uLim": p.u_lim, "slackW": R.SLACK_WEIGHT, "polDelta": R.POLISH_DELTA, "polRho": R.POLISH_RHO,
           "Q": np.array(p.Q), "Qf": np.array(p.Q_final), "R": np.array(p.R)}
    base = dict(V=V, O=O, Hb=Hb, g=np.array(lin.g), rowE=rows[:, 0:2].copy(), rowW=rows[:, 2].copy(),
                rowH=rows[:, 3].copy(), qs=qp[1][:N].copy())
    return base, par, qp, rows


@functools.lru_cache(maxsize=None)
def oracle_iterates(src):
    import linalg_cases as LC
    P, q, G, h = oracle_problem(src)[2]
    its = []
    LC.ipm_systems(P, q, G, h, iterates=its)
    assert len(its) >= 3, (src, len(its))
    return its


def stage_index(n, stage):
    return {"first": 0, "middle": n // 2, "last": n - 1}[stage]


def _states_of(base, par, it):
    d = it["lam"] / it["s"]
    common = dict(base, z=it["x"], s=it["s"], lam=it["lam"], rp=it["rp"], dd=d, rd=it["rd"],
                  tv=d * it["rp"] - it["lam"])
    args = dict(rho=par["polRho"], mu=it["mu"], smu=it["smu"], eta=it["eta"])
    pred = dict(common, dz=it["dx_aff"], sa=np.zeros_like(d), la=np.zeros_like(d), args=args)
    corr = dict(common, dz=it["dx"], sa=it["ds_aff"], la=it["dl_aff"], args=args)
    return pred, corr


def separated(pred, corr, par):
    """Every separation condition of an iterate's states holds (float64 stand-in for the device)."""
    for site in (QH.S_R, QH.S_I, QH.S_B, QH.S_U):
        st = corr if site == QH.S_U else pred
        sep = check(st, par, site, st["args"], outputs_f64(st, par, site, st["args"]))[1]
        if not all(sep.values()):
            return False
    return True


@functools.lru_cache(maxsize=None)
def last_separated(src):
    """The last iterate of the restated IPM at which every separation condition holds.  At the
    converged iterates rp and rd are rounding noise (no entry of them leads another by more
    than its bound) and steps bind on several rows at once, so the very last few do not
    qualify; the one taken is past the middle, with d over many decades."""
    base, par, _, _ = oracle_problem(src)
    its = oracle_iterates(src)
    for i in range(len(its) - 1, len(its) // 2, -1):
        if separated(*_states_of(base, par, its[i]), par):
            return i
    raise AssertionError(("no separated iterate past the middle", src))


@functools.lru_cache(maxsize=None)
def oracle_states(src, stage):
    """(predictor state, corrector state, parameters) of an iterate of the source's first QP."""
    base, par, _, _ = oracle_problem(src)
    its = oracle_iterates(src)
    i = last_separated(src) if stage == "last" else stage_index(len(its), stage)
    pred, corr = _states_of(base, par, its[i])
    return pred, corr, par


# ---------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------
ALL_SITES = (QH.S_A, QH.S_G, QH.S_GH, QH.S_T, QH.S_R, QH.S_I, QH.S_B, QH.S_U)


def unit_cases(unit):
    """[(key, V, O, HM, Hb, site, state, params, args)] of a unit: key = (family, shape or
    source, stage or row, site, variant)."""
    out = []
    for V, O, HM, Hb, _ in SHAPES[unit]:
        st, par = random_state(V, O, Hb), _params("random", V)
        for site in ALL_SITES:
            out.append((("random", (V, O, HM, Hb), 0, site, 0), V, O, HM, Hb, site, st, par, st["args"]))
        out.append((("random", (V, O, HM, Hb), 0, QH.S_A, 1), V, O, HM, Hb, QH.S_A, st, par, dict(rho=0.0)))
    for src in ORACLE[unit]:
        kind, V, HM, scale, hps, b, Hb = src
        for stage in ORACLE_STAGES[unit]:
            pred, corr, par = oracle_states(src, stage)
            O = pred["O"]
            for site in ALL_SITES:
                st = corr if site == QH.S_U else pred
                out.append((("oracle", src, stage, site, 0), V, O, HM, Hb, site, st, par, st["args"]))
            out.append((("oracle", src, stage, QH.S_A, 1), V, O, HM, Hb, QH.S_A, pred, par, dict(rho=0.0)))
    for u, V, O, HM, Hb in ONE_HOT:
        if u != unit:
            continue
        par = _params("zero", V)
        for r, st in enumerate(one_hot_states(V, O, Hb)):
            out.append((("one-hot", (V, O, HM, Hb), r, QH.S_A, 1), V, O, HM, Hb, QH.S_A, st, par, dict(rho=0.0)))
    return out


_dense = {}


def dense(st, par, T=QM.F80, mutate=None):
    """The dense problem of a state, cached by the structured arrays it is built from."""
    key = (id(st["g"]), id(st["rowE"]), id(st["qs"]), id(par), T, mutate)
    if key not in _dense:
        _dense[key] = (QM.Dense(st, par, T, mutate), st["g"], st["rowE"], st["qs"], par)
    return _dense[key][0]


# ---------------------------------------------------------------------------------------
# one case against the 80-bit mirror
# ---------------------------------------------------------------------------------------
def outputs_f64(st, par, site, args):
    """What a float64 evaluation of a site leaves behind, in the names ``check`` reads: the
    stand-in for the device in the CPU test."""
    T = QM.F64
    D = dense(st, par, T)
    if site == QH.S_A:
        return {"K": QM.site_assemble(D, st, args["rho"])["K"][0], "Wt": QM.wt_blocks(D, st, par)[0]}
    if site in (QH.S_G, QH.S_GH):
        return {"rp": QM.site_gapply(D, st, site == QH.S_GH)["rp"][0]}
    if site == QH.S_T:
        return {"rhs": QM.site_rhs_from_tv(D, st, args["rho"])["rhs"][0]}
    if site == QH.S_R:
        r = QM.site_residuals(D, st)
        return {k: r[k][0] for k in ("rp", "dd", "tv", "rd", "ret")}
    if site == QH.S_I:
        r = QM.site_init_b(D, st)
        return {"s": r["s"][0], "lam": r["lam"][0], "om": r["om"][0]}
    if site == QH.S_B:
        d = QM.direction(D, st, 0, 0.0)
        ds, dl = d["ds"][0], d["dl"][0]
        smu = QM.centring(D, st, args["mu"], ds, dl)["smu"][0]
        tv = QM.corrector_tv(D, st, smu, ds, dl)["tv"][0]
        return {"sa": ds, "la": dl, "smu": smu, "tv": tv, "rhs": QM.newton_rhs(D, st, tv)["rhs"][0]}
    r = QM.site_update(D, st, args["smu"], args["eta"])
    out = {k: r[k][0] for k in ("z", "s", "lam")}
    out["sa"], out["la"] = r["ds"][0], r["dl"][0]
    rr = QM.site_residuals(D, st, z=out["z"], s=out["s"], lam=out["lam"])
    out.update({k: rr[k][0] for k in ("rp", "dd", "tv", "rd", "ret")})
    return out


def check(st, par, site, args, dev, direction_stored=True):
    """({value name: largest |dev - ref| / bound}, {condition: separated}) of one case's outputs
    ``dev`` against the 80-bit mirror.  Where a site forms a value from one it has stored
    (the affine direction, sigma mu, tv, the updated point), the reference of the later value
    starts from the device's stored one, so no bound carries another's."""
    D = dense(st, par, QM.F80)
    out, sep = {}, {}

    def cmp(ref, names, dev_names=None):
        for k, dk in zip(names, dev_names or names):
            out[k] = QM.ratio(dev[dk], ref[k][0], ref[k][1])
        sep.update(ref.get("sep", {}))
    if site == QH.S_A:
        ref = QM.site_assemble(D, st, args["rho"])
        out["K"] = QM.ratio(np.tril(dev["K"]), ref["K"][0], ref["K"][1])
        W, Wb = QM.wt_blocks(D, st, par)
        out["Wt"] = QM.ratio(dev["Wt"], W, Wb)
    elif site in (QH.S_G, QH.S_GH):
        cmp(QM.site_gapply(D, st, site == QH.S_GH), ("rp",))
    elif site == QH.S_T:
        cmp(QM.site_rhs_from_tv(D, st, args["rho"]), ("rhs",))
    elif site == QH.S_R:
        cmp(QM.site_residuals(D, st), ("rp", "dd", "tv", "rd", "ret"))
    elif site == QH.S_I:
        cmp(QM.site_init_b(D, st), ("s", "lam", "om"))
    elif site == QH.S_B:
        cmp(QM.direction(D, st, 0, 0.0), ("ds",), ("sa",))
        cmp(QM.direction(D, st, 0, 0.0, ds=dev["sa"]), ("dl",), ("la",))
        cmp(QM.centring(D, st, args["mu"], dev["sa"], dev["la"]), ("smu",))
        cmp(QM.corrector_tv(D, st, dev["smu"], dev["sa"], dev["la"]), ("tv",))
        cmp(QM.newton_rhs(D, st, dev["tv"]), ("rhs",))
    else:
        ref = QM.site_update(D, st, args["smu"], args["eta"])
        cmp(ref, ("z", "s", "lam"))
        if direction_stored:
            cmp(ref, ("ds", "dl"), ("sa", "la"))
        rr = QM.site_residuals(D, st, z=dev["z"], s=dev["s"], lam=dev["lam"])
        sep.update({"new point " + k: v for k, v in rr.pop("sep").items()})
        cmp(rr, ("rp", "dd", "tv", "rd", "ret"))
    return out, sep
