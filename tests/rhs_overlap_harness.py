"""Build and bind tests/rhs_overlap/rhs_overlap_harness.hip: the three assemble-and-factor
phases of csrc/scpqp_kernel.h with their right-hand side in front of the factorisation or
beside it (tests/test_gpu_rhs_overlap.py).

``ensure_built()`` compiles the harness with the flags of ``scpqp/build.py`` into
``tests/rhs_overlap/librhs_overlap_harness.so``; whether the library is current is decided by
a hash of the kernel header and the harness source kept beside it, as tests/linalg_harness.py
does.  A stale or missing library is rebuilt when ``hipcc`` is there and is an error when it is
not: never a skip.

The module also restates the virtual-thread mapping of the side job (GtSide) and the plan's
write sets, for the host test and the GPU test's masks."""
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
SRC = os.path.join(HERE, "rhs_overlap", "rhs_overlap_harness.hip")
LIB = os.path.join(HERE, "rhs_overlap", "librhs_overlap_harness.so")
STAMP = LIB + ".hash"
UNITS = 4
HDR = 8            # kRoHdr
NT, NWAVE, CB = 256, 4, 8
K_SPLIT, PER_WAVE = 3, 21          # split3_outputs: lanes per output, outputs per wave and pass
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
        raise RuntimeError("tests/rhs_overlap/librhs_overlap_harness.so is missing or stale and "
                           "there is no hipcc to build it")
    want = source_hash()
    tmp = tempfile.mkdtemp(prefix="rhs_overlap_harness_")
    try:
        def unit(k):
            obj = os.path.join(tmp, f"unit{k}.o")
            cmd = ["hipcc", "-c"] + FLAGS + [f"-DRO_UNIT={k}", SRC, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            return obj
        with ThreadPoolExecutor(min(UNITS + 1, B._jobs())) as ex:
            objs = list(ex.map(unit, (4, 3, 2, 1, 0)))
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


class RoCase(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("Hb", "lead", "site", "order", "inoff", "ooff", "koff", "pad")]


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(ensure_built())
        lib.ro_plan.argtypes = [C.c_int] * 4 + [C.c_void_p]
        lib.ro_in_size.argtypes = [C.c_int] * 3
        lib.ro_side_step.argtypes = [C.c_int] * 2
        lib.ro_run.argtypes = [C.c_int] * 5 + [C.POINTER(RoCase), C.c_void_p, C.c_longlong, C.c_void_p,
                                               C.c_longlong]
        _lib = lib
    return _lib


# ---------------------------------------------------------------------------------------
# the side job's mapping, restated (GtSide, gt_incident_part, split3_outputs, side_step)
# ---------------------------------------------------------------------------------------
def tw_of(wave, lead):
    """Helper index of a non-lead wave: (wave - lead + NWAVE - 1) % NWAVE."""
    return (wave - lead + NWAVE - 1) % NWAVE


def virtual_waves(h, nh):
    """The waves whose shares helper h of nh takes."""
    return list(range(h, NWAVE, nh))


def stage0_items(vw, lane, nout, m):
    """(outputs e of the incident sums, rows r of the omega sum) of virtual thread 64 vw + lane."""
    vt = 64 * vw + lane
    return list(range(vt, nout, NT)), list(range(vt, m, NT))


def stage1_outputs(vw, lane, nout):
    """The outputs e whose owner lane (term index 0 of the split) is this lane of virtual wave vw."""
    j, sidx = divmod(lane, K_SPLIT)
    if lane >= K_SPLIT * PER_WAVE or sidx != 0:
        return []
    return [e for e in range(vw * PER_WAVE + j, nout, PER_WAVE * NWAVE)]


def side_step(k, nsteps, late=8, stages=2):
    """side_step<stages>(k, nsteps) of the header at kSideLate = late."""
    if k == 0:
        return 0
    return min(late + k - 1, nsteps - stages + k - (1 if nsteps > stages else 0))


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
        v = (C.c_int * 17)()
        if load().ro_plan(unit, V, O, HM, v) != 0:
            raise ValueError((unit, V, O, HM))
        (self.lds, self.ws, self.yb, self.rhs, self.dinv, self.red, self.H, self.Wt, self.vec, self.mcAlloc,
         self.pb, self.dz, self.rd, self.qs, self.vg, self.lean, self.tvlds) = list(v)
        self.unit, self.V, self.O, self.HM = unit, V, O, HM
        self.size = self.lds + self.ws
        self.red_size = load().ro_red_size()
        self.side = load().ro_side_slot()
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

    def owned(self, site, Hb):
        """Boolean mask over the image of what the site may write: the factor's storage, W~,
        yb, the first n of rhs and dinv, the reduction buffers, the failure flag, the side job's
        partials and the pivots; tv where the site forms it; d and dz where ph_init_a does."""
        N, n, m, mc = self.dims(Hb)
        w = np.zeros(self.size, dtype=bool)
        w[self.H:self.H + self.Hlen] = True
        wt = (self.lds if self.lean else 0) + self.Wt
        w[wt:wt + self.Wtlen] = True
        w[self.yb:self.yb + 2 * N] = True
        w[self.rhs:self.rhs + n] = True
        w[self.dinv:self.dinv + n] = True
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

    def scratch(self):
        """What the two orders may leave different: block_reduce4's partial sums (the order in
        front reduces through them, after the factorisation on the cold start) and the side
        job's partials."""
        w = np.zeros(self.size, dtype=bool)
        w[self.red:self.red + 48] = True
        w[self.red + self.side:self.red + self.side + NWAVE] = True
        return w


def make_state(rng, V, O, Hb, negative_d=False):
    """A problem state in ro_in_doubles' order: g rowE rowW rowH dd tv sa la rd qs dz."""
    N, n = V * Hb, V * Hb + 1
    m = V * (V - 1) // 2 * Hb + V * O * Hb
    mc = m + 2 * N + 1
    ang = rng.uniform(0, 2 * np.pi, m)
    rowE = np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(-1) * rng.uniform(0.5, 2.0, m).repeat(2)
    parts = [rng.standard_normal(2 * N) * 0.3, rowE, -rng.uniform(0.1, 1.0, m), rng.standard_normal(m),
             rng.uniform(0.5, 2.0, mc) * (-1.0 if negative_d else 1.0), rng.standard_normal(mc),
             (rng.uniform(size=mc) < 0.4).astype(np.float64), rng.uniform(0.0, 3.0, mc),
             rng.standard_normal(n), rng.standard_normal(N), rng.standard_normal(n)]
    out = np.concatenate(parts)
    assert out.size == load().ro_in_size(V, O, Hb)
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
    desc = (RoCase * len(cases))()
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
    rc = lib.ro_run(plan.unit, plan.V, plan.O, plan.HM, len(cases), desc, buf.ctypes.data, buf.size,
                    out.ctypes.data, out.size)
    if rc != 0:
        raise RuntimeError(f"ro_run(unit {plan.unit}, {len(cases)} cases) returned {rc}")
    return [Result(plan, out[c.ooff:c.ooff + per]) for c in desc]


if __name__ == "__main__":
    print(ensure_built(verbose=True))
