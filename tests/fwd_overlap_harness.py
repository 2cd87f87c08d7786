"""Build and bind tests/fwd_overlap/fwd_overlap_harness.hip: a factor phase of
csrc/scpqp_kernel.h and the solve that follows it, with the solve's forward sweep hidden under
the factorisation or run by the lead after it (tests/test_gpu_fwd_overlap.py).

``ensure_built()`` compiles the harness with the flags of ``scpqp/build.py`` into
``tests/fwd_overlap/libfwd_overlap_harness.so``; whether the library is current is decided by
a hash of the kernel header and the harness source kept beside it, as tests/rhs_overlap_harness.py
does.  A stale or missing library is rebuilt when ``hipcc`` is there and is an error when it is
not: never a skip.

The module also restates the sweep's schedule (fwd_sched, fwd_sched_fits) and the plan's write
sets, for the host test and the GPU test's masks."""
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
SRC = os.path.join(HERE, "fwd_overlap", "fwd_overlap_harness.hip")
LIB = os.path.join(HERE, "fwd_overlap", "libfwd_overlap_harness.so")
STAMP = LIB + ".hash"
UNITS = 4
HDR = 8            # kFoHdr
NT, NWAVE, CB = 256, 4, 8
FLAGS = ["--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
         f"-I{B.INCLUDE}"]
SITES = ("ipm", "polish", "init", "given K")


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
        raise RuntimeError("tests/fwd_overlap/libfwd_overlap_harness.so is missing or stale and "
                           "there is no hipcc to build it")
    want = source_hash()
    tmp = tempfile.mkdtemp(prefix="fwd_overlap_harness_")
    try:
        def unit(k):
            obj = os.path.join(tmp, f"unit{k}.o")
            cmd = ["hipcc", "-c"] + FLAGS + [f"-DFO_UNIT={k}", SRC, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            return obj
        with ThreadPoolExecutor(min(UNITS + 1, B._jobs())) as ex:
            objs = list(ex.map(unit, (3, 4, 2, 1, 0)))
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


class FoCase(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("Hb", "lead", "site", "order", "inoff", "ooff", "koff", "pad")]


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(ensure_built())
        lib.fo_plan.argtypes = [C.c_int] * 4 + [C.c_void_p]
        lib.fo_in_size.argtypes = [C.c_int] * 3
        lib.fo_fwd_sched.argtypes = [C.c_int] * 4
        lib.fo_fwd_sched_fits.argtypes = [C.c_int] * 3
        lib.fo_side_step.argtypes = [C.c_int] * 2
        lib.fo_fits.argtypes = [C.c_int] * 2
        lib.fo_run.argtypes = [C.c_int] * 5 + [C.POINTER(FoCase), C.c_void_p, C.c_longlong, C.c_void_p,
                                               C.c_longlong]
        _lib = lib
    return _lib


# ---------------------------------------------------------------------------------------
# the sweep's schedule, restated (fwd_sched, fwd_sched_fits of the header)
# ---------------------------------------------------------------------------------------
def fwd_sched(s, nsteps, n, s1, chunk=4):
    """Columns done after panel step s: step s covers [fwd_sched(s - 1), fwd_sched(s))."""
    j = 0
    for t in range(s1 + 1, min(s, nsteps - 1) + 1):
        left, steps = n - 1 - j, nsteps - t
        share = ((left + steps - 1) // steps + chunk - 1) // chunk * chunk
        j = min(j + share, CB * t, n - 1)
    return j


def fwd_sched_fits(nsteps, n, s1, chunk=4, min_steps=2):
    return (n > 1 and (n - 1) % chunk == 0 and nsteps == -(-n // CB) and s1 >= 0
            and nsteps - 1 - s1 >= min_steps and fwd_sched(nsteps - 1, nsteps, n, s1, chunk) == n - 1)


# ---------------------------------------------------------------------------------------
# plans and masks
# ---------------------------------------------------------------------------------------
def pad2(x):
    return (x + 1) & ~1


def roff(i):
    return i * (i + 1) // 2 + ((i + 1) >> 1)


class Plan:
    """The layout of a unit at (V, O, HM): offsets in doubles, LDS then workspace in one image."""
    def __init__(self, unit, V, O, HM):
        v = (C.c_int * 21)()
        if load().fo_plan(unit, V, O, HM, v) != 0:
            raise ValueError((unit, V, O, HM))
        (self.lds, self.ws, self.yb, self.rhs, self.dinv, self.red, self.H, self.Wt, self.vec, self.mcAlloc,
         self.pb, self.dz, self.rd, self.qs, self.z, self.vg, self.lean, self.tvlds, self.hg, self.wg,
         self.red_size) = list(v)
        self.unit, self.V, self.O, self.HM = unit, V, O, HM
        self.size = self.lds + self.ws
        self.side = load().fo_side_slot()
        nb = V * (V + 1) // 2
        self.Hlen = pad2(roff(V * HM + 2) + 16)
        self.Wtlen = pad2(4 * HM * nb)

    def vec_at(self, k):
        """Image offset of constraint-space vector k (s lam rp dd sa la tv)."""
        if k == 6 and self.tvlds:
            return self.pb
        return (self.lds if self.vg else 0) + self.vec + k * self.mcAlloc

    def dims(self, Hb):
        N = self.V * Hb
        m = self.V * (self.V - 1) // 2 * Hb + self.V * self.O * Hb
        return N, N + 1, m, m + 2 * N + 1

    def x_at(self, site):
        """Image offset of the solve's destination: z after the cold start, else dz."""
        return self.z if site == 2 else self.dz

    def owned(self, site, Hb):
        """Boolean mask over the image of what the site may write: the factor's storage, W~,
        yb, the first n of rhs, dinv and of the solve's destination, the reduction buffers, the
        failure flag, the side job's partials and the pivots; tv where the site forms it; d and
        dz where ph_init_a does."""
        N, n, m, mc = self.dims(Hb)
        w = np.zeros(self.size, dtype=bool)
        h = (self.lds if self.hg else 0) + self.H
        w[h:h + self.Hlen] = True
        wt = (self.lds if self.wg else 0) + self.Wt
        w[wt:wt + self.Wtlen] = True
        w[self.yb:self.yb + 2 * N] = True
        w[self.rhs:self.rhs + n] = True
        w[self.dinv:self.dinv + n] = True
        w[self.x_at(site):self.x_at(site) + n] = True
        r = self.red
        w[r:r + 65] = True                          # block_reduce4 / ldbuf, the failure flag
        w[r + self.side:r + self.side + NWAVE] = True
        w[r + 72:r + self.red_size] = True          # pivots
        if site in (1, 2):
            w[self.vec_at(6):self.vec_at(6) + mc] = True
        if site == 2:
            w[self.vec_at(3):self.vec_at(3) + mc] = True
            w[self.dz:self.dz + n] = True
        return w


def make_state(rng, V, O, Hb):
    """A problem state in fo_in_doubles' order: g rowE rowW rowH dd tv sa la rd qs dz."""
    N, n = V * Hb, V * Hb + 1
    m = V * (V - 1) // 2 * Hb + V * O * Hb
    mc = m + 2 * N + 1
    ang = rng.uniform(0, 2 * np.pi, m)
    rowE = np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(-1) * rng.uniform(0.5, 2.0, m).repeat(2)
    parts = [rng.standard_normal(2 * N) * 0.3, rowE, -rng.uniform(0.1, 1.0, m), rng.standard_normal(m),
             rng.uniform(0.5, 2.0, mc), rng.standard_normal(mc),
             (rng.uniform(size=mc) < 0.4).astype(np.float64), rng.uniform(0.0, 3.0, mc),
             rng.standard_normal(n), rng.standard_normal(N), rng.standard_normal(n)]
    out = np.concatenate(parts)
    assert out.size == load().fo_in_size(V, O, Hb)
    return out


class Result:
    def __init__(self, plan, o):
        self.ret = int(o[0])
        self.before = o[HDR:HDR + plan.size].view(np.uint64).copy()
        self.after = o[HDR + plan.size:HDR + 2 * plan.size].view(np.uint64).copy()


def run(plan, cases):
    """cases: [(Hb, lead, site, order, state, K or None)]; one launch, one workgroup per case.
    Returns [Result] (images as uint64: the comparison is of bits)."""
    lib = load()
    desc = (FoCase * len(cases))()
    ins, nin, nout, seen = [], 0, 0, {}

    def place(arr):
        nonlocal nin
        if id(arr) not in seen:
            seen[id(arr)] = nin
            ins.append(np.ascontiguousarray(arr, dtype=np.float64).reshape(-1))
            nin += ins[-1].size
        return seen[id(arr)]
    per = HDR + 2 * plan.size
    for c, (Hb, lead, site, order, state, K) in zip(desc, cases):
        c.Hb, c.lead, c.site, c.order = Hb, lead, site, order
        c.inoff = place(state)
        c.koff = place(K) if K is not None else 0
        c.ooff = nout
        nout += per
    buf = np.concatenate(ins)
    out = np.zeros(nout)
    rc = lib.fo_run(plan.unit, plan.V, plan.O, plan.HM, len(cases), desc, buf.ctypes.data, buf.size,
                    out.ctypes.data, out.size)
    if rc != 0:
        raise RuntimeError(f"fo_run(unit {plan.unit}, {len(cases)} cases) returned {rc}")
    return [Result(plan, out[c.ooff:c.ooff + per]) for c in desc]


if __name__ == "__main__":
    print(ensure_built(verbose=True))
