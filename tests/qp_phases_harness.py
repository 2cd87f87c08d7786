"""Build and bind tests/qp_phases/qp_phases_harness.hip: the KKT assembly and the IPM's vector
phases of csrc/scpqp_kernel.h, each run alone on a given state (tests/test_gpu_qp_phases.py).

``ensure_built()`` compiles the harness with the flags of ``scpqp/build.py`` into
``tests/qp_phases/libqp_phases_harness.so``; whether the library is current is decided by a
hash of the kernel header and the harness source kept beside it, as tests/linalg_harness.py
does.  A stale or missing library is rebuilt when ``hipcc`` is there and is an error when it is
not: never a skip.

The module also holds the plan of a unit at a shape (``Plan``: where every array lies in the
image of a workgroup's LDS and workspace slice) and what each site may write (``Plan.owned``),
both read off csrc/scpqp_kernel.h."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from scpqp import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "qp_phases", "qp_phases_harness.hip")
LIB = os.path.join(HERE, "qp_phases", "libqp_phases_harness.so")
STAMP = LIB + ".hash"
UNITS = 6
# (HG, VG, RM, OCC, SH) of every unit
KERNELS = {1: (0, 0, 1, 3, 0), 2: (0, 1, 2, 3, 1), 3: (0, 1, 2, 2, 2), 4: (1, 1, 2, 3, 0),
           5: (1, 1, 4, 2, 0), 6: (1, 1, 4, 2, 3)}
HDR = 8            # kQpHdr
NT = 256
MAX_VEH = 16
NPARAM = 4 + 3 * MAX_VEH
KVECS = 7
VEC = {"s": 0, "lam": 1, "rp": 2, "dd": 3, "sa": 4, "la": 5, "tv": 6}
SITES = ("assemble", "g_apply", "g_apply_minus_h", "rhs_from_tv", "residuals", "init_b", "back_affine_rhs",
         "back_update_residuals")
S_A, S_G, S_GH, S_T, S_R, S_I, S_B, S_U = range(8)
FLAGS = ["--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
         f"-I{B.INCLUDE}"]


def source_hash():
    h = hashlib.sha256()
    for p in (B.HEADER, SRC):
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS[:5]).encode())
    return h.hexdigest()


def is_current():
    if not (os.path.exists(LIB) and os.path.exists(STAMP)):
        return False
    with open(STAMP) as f:
        return f.read().strip() == source_hash()


def ensure_built(verbose=False):
    if is_current():
        return LIB
    if shutil.which("hipcc") is None:
        raise RuntimeError("tests/qp_phases/libqp_phases_harness.so is missing or stale and "
                           "there is no hipcc to build it")
    want = source_hash()
    tmp = tempfile.mkdtemp(prefix="qp_phases_harness_")
    try:
        def unit(k):
            obj = os.path.join(tmp, f"unit{k}.o")
            cmd = ["hipcc", "-c"] + FLAGS + [f"-DQP_UNIT={k}", SRC, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            return obj
        with ThreadPoolExecutor(min(UNITS + 1, B._jobs())) as ex:
            objs = list(ex.map(unit, (3, 6, 5, 4, 2, 1, 0)))
        out = os.path.join(tmp, "lib.so")
        subprocess.run(["hipcc", "-shared", "-fPIC", "--offload-arch=" + B.ARCH] + objs + ["-o", out],
                       check=True)
        shutil.move(out, LIB + ".tmp")
        os.replace(LIB + ".tmp", LIB)
        with open(STAMP, "w") as f:
            f.write(want + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return LIB


class QpCase(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("Hb", "site", "pidx", "lead", "inoff", "ooff", "pad0", "pad1")] + \
               [(k, C.c_double) for k in ("rho", "mu", "smu", "eta")]


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(ensure_built())
        lib.qp_plan.argtypes = [C.c_int] * 5 + [C.c_void_p]
        lib.qp_in_size.argtypes = [C.c_int] * 3
        lib.qp_rinfo_host.argtypes = [C.c_int] * 4
        lib.qp_roff.argtypes = [C.c_int]
        lib.qp_tile_size.argtypes = [C.c_int] * 3
        lib.qp_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(QpCase), C.c_void_p,
                               C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        _lib = lib
    return _lib


def roff(i):
    return i * (i + 1) // 2 + ((i + 1) >> 1)


def dims(V, O, Hb):
    """(N, n, m, mc) of a problem."""
    N = V * Hb
    m = V * (V - 1) // 2 * Hb + V * O * Hb
    return N, N + 1, m, m + 2 * N + 1


def tile_size(hg, V, Hb):
    """assemble's switch between assemble_tiles<4> and assemble_tiles<2>, restated."""
    if not hg:
        return 4
    T4, PV = (Hb + 3) // 4, V * (V - 1) // 2
    return 4 if V * (T4 * (T4 + 1) // 2) + PV * T4 * T4 >= 2 * NT else 2


def rinfo(r, V, O, Hb, rows):
    """Entry r of the row table from the oracle's row list: i | (j + 1) << 8 | (o + 1) << 16 | k << 24."""
    i, j, o, k = rows[r]
    return i | ((j + 1) << 8) | ((o + 1) << 16) | (k << 24)


class Plan:
    """The layout of a unit at (V, O, HM) for a problem of horizon Hb: offsets in doubles into
    the image [LDS (lds_img doubles) | workspace slice], lds_img being the launch's LDS size."""
    def __init__(self, unit, V, O, HM, Hb=None):
        Hb = HM if Hb is None else Hb
        v = (C.c_int * 28)()
        if load().qp_plan(unit, V, O, HM, Hb, v) != 0:
            raise ValueError((unit, V, O, HM, Hb))
        (self.lds, self.ws, self.g, self.ya, self.yb, self.qs, self.rowE, self.rowW, self.rowH, self.rinfo,
         self.z, self.dz, self.rhs, self.rd, self.dinv, self.red, self.H, self.Wt, self.vec, self.pb,
         self.mcAlloc, self.hg, self.vg, self.wg, self.lean, self.tvlds, self.slots, self.red_size) = list(v)
        self.unit, self.V, self.O, self.HM, self.Hb = unit, V, O, HM, Hb
        self.N, self.n, self.m, self.mc = dims(V, O, Hb)
        self.nb = V * (V + 1) // 2
        self.tile = tile_size(self.hg, V, Hb)

    # image offsets, given the launch's LDS size
    def at(self, name, lds_img):
        """Image offset of an LDS array, the factor ("H"), W~ ("Wt") or a constraint-space vector."""
        if name in VEC:
            k = VEC[name]
            if k == 6 and self.tvlds:
                return self.pb
            return (lds_img if self.vg else 0) + self.vec + k * self.mcAlloc
        if name == "H":
            return (lds_img if self.hg else 0) + self.H
        if name == "Wt":
            return (lds_img if self.wg else 0) + self.Wt
        if name in ("rowE", "rowW", "rowH", "rinfo"):
            return (lds_img if self.lean else 0) + getattr(self, name)
        return getattr(self, name)

    def packed_index(self, lds_img):
        """Image offsets of the entries (i, j <= i) of the packed factor's rows 0..N, as (rows, cols, offsets)."""
        i, j = np.tril_indices(self.n)
        ro = i * (i + 1) // 2 + ((i + 1) >> 1)
        return i, j, self.at("H", lds_img) + ro + j

    def owned(self, site, lds_img, size):
        """Boolean mask over the image of what a site may write (read off each phase's code):
        block_reduce4's three partial-sum buffers red[0, 48) wherever a reduction runs, and
          assemble        the packed entries (i, j <= i) of rows 0..N, W~ (4 Hb nb), yb (2 N)
          g_apply         ya (2 N), rp (mc)
          rhs_from_tv     yb, rhs (n)
          residuals       ya, yb, rp, dd, tv, rd (n)
          init_b          ya, s, lam, z[N]
          back_affine_rhs ya, yb, sa, la, tv, rhs
          back_update_residuals  ya, yb, z, s, lam, sa, la (the direction: RowsMem only writes
                          it), rp, dd, tv, rd"""
        N, n, mc = self.N, self.n, self.mc
        w = np.zeros(size, dtype=bool)

        def own(name, cnt):
            a = self.at(name, lds_img)
            w[a:a + cnt] = True
        if site != S_G and site != S_GH:
            w[self.red:self.red + 48] = True
        if site == S_A:
            w[self.packed_index(lds_img)[2]] = True
            own("Wt", 4 * self.Hb * self.nb)
            own("yb", 2 * N)
        elif site in (S_G, S_GH):
            own("ya", 2 * N)
            own("rp", mc)
        elif site == S_T:
            own("yb", 2 * N)
            own("rhs", n)
        elif site == S_R:
            for k in ("ya", "yb"):
                own(k, 2 * N)
            for k in ("rp", "dd", "tv"):
                own(k, mc)
            own("rd", n)
        elif site == S_I:
            own("ya", 2 * N)
            own("s", mc)
            own("lam", mc)
            w[self.z + N] = True
        elif site == S_B:
            for k in ("ya", "yb"):
                own(k, 2 * N)
            for k in ("sa", "la", "tv"):
                own(k, mc)
            own("rhs", n)
        elif site == S_U:
            for k in ("ya", "yb"):
                own(k, 2 * N)
            for k in ("s", "lam", "sa", "la", "rp", "dd", "tv"):
                own(k, mc)
            own("z", n)
            own("rd", n)
        else:
            raise ValueError(site)
        return w


STATE_FIELDS = ("g", "rowE", "rowW", "rowH", "z", "dz", "s", "lam", "rp", "dd", "sa", "la", "tv", "rd", "qs")


def pack_state(st):
    """The input block of a state (a dict of STATE_FIELDS) in qp_in_doubles' order."""
    out = np.concatenate([np.ascontiguousarray(st[k], dtype=np.float64).reshape(-1) for k in STATE_FIELDS])
    assert out.size == load().qp_in_size(st["V"], st["O"], st["Hb"]), (out.size, st["V"], st["O"], st["Hb"])
    return out


def pack_params(par):
    """uLim slackW polDelta polRho Q[] Qf[] R[] of a parameter dict."""
    q = np.zeros(NPARAM)
    q[0:4] = par["uLim"], par["slackW"], par["polDelta"], par["polRho"]
    V = len(par["Q"])
    q[4:4 + V] = par["Q"]
    q[4 + MAX_VEH:4 + MAX_VEH + V] = par["Qf"]
    q[4 + 2 * MAX_VEH:4 + 2 * MAX_VEH + V] = par["R"]
    return q


class Result:
    def __init__(self, plan, lds_img, size, o):
        self.plan, self.lds_img = plan, lds_img
        self.ret = o[0:4].copy()
        self.before = o[HDR:HDR + size].copy()
        self.after = o[HDR + size:HDR + 2 * size].copy()

    def get(self, name, cnt, when="after"):
        a = self.plan.at(name, self.lds_img)
        return getattr(self, when)[a:a + cnt]

    def packed(self):
        """Rows 0..N of the packed factor as a dense lower triangle."""
        i, j, at = self.plan.packed_index(self.lds_img)
        K = np.zeros((self.plan.n, self.plan.n))
        K[i, j] = self.after[at]
        return K

    def written_outside(self, site):
        own = self.plan.owned(site, self.lds_img, self.before.size)
        return np.flatnonzero((self.before.view(np.uint64) != self.after.view(np.uint64)) & ~own)


def run(unit, cases):
    """cases: [(V, O, HM, Hb, site, state, params dict, {rho, mu, smu, eta})]; one launch, one
    workgroup per case.  Returns [Result]."""
    lib = load()
    shapes, pars, plans = [], [], []
    shape_of = {}
    ins, nin, seen = [], 0, {}
    desc = (QpCase * len(cases))()
    for c, (V, O, HM, Hb, site, st, par, arg) in zip(desc, cases):
        key = (V, O, HM, id(par))
        if key not in shape_of:
            shape_of[key] = len(shapes)
            shapes.append((V, O, HM))
            pars.append(pack_params(par))
        plans.append(Plan(unit, V, O, HM, Hb))
        if id(st) not in seen:
            seen[id(st)] = nin
            ins.append(pack_state(st))
            nin += ins[-1].size
        c.Hb, c.site, c.pidx, c.lead, c.inoff = Hb, site, shape_of[key], 0, seen[id(st)]
        c.rho, c.mu, c.smu, c.eta = (float(arg.get(k, 0.0)) for k in ("rho", "mu", "smu", "eta"))
    ldsN = max(p.lds for p in plans)
    wsN = max(p.ws for p in plans)
    size = ldsN + wsN
    per = HDR + 2 * size
    for i, c in enumerate(desc):
        c.ooff = i * per
    buf = np.concatenate(ins)
    out = np.zeros(per * len(cases))
    sh = np.ascontiguousarray(np.array(shapes, dtype=np.int32))
    pr = np.ascontiguousarray(np.array(pars, dtype=np.float64))
    rc = lib.qp_run(unit, len(shapes), sh.ctypes.data, pr.ctypes.data, len(cases), desc, buf.ctypes.data,
                    buf.size, out.ctypes.data, out.size, ldsN, wsN)
    if rc != 0:
        raise RuntimeError(f"qp_run(unit {unit}, {len(cases)} cases) returned {rc}")
    return [Result(p, ldsN, size, out[i * per:(i + 1) * per]) for i, p in enumerate(plans)]


if __name__ == "__main__":
    print(ensure_built(verbose=True))
