"""Build and bind tests/asm_overlap/asm_overlap_harness.hip: the KKT assembly of
csrc/scpqp_kernel.h alone, in the order of -DSCPQP_DIAG_ASM_FRONT (order 0) and in the shipped
one (order 1) (tests/test_gpu_asm_overlap.py).

``ensure_built()`` compiles the harness with the flags of ``scpqp/build.py`` into
``tests/asm_overlap/libasm_overlap_harness.so``; whether the library is current is decided by a
hash of the kernel header and the harness source kept beside it, as tests/linalg_harness.py
does.  A stale or missing library is rebuilt when ``hipcc`` is there and is an error when it is
not: never a skip.

The units are those of tests/qp_phases_harness.py (1, 2, 3 and 6 of them), whose ``Plan`` gives
the layout of the images.

The module also restates the work assignment of ``assemble`` in the shipped order (who writes
which W~ block, yb entry, tile entry and omega-row entry), for tests/test_asm_overlap_host.py."""
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
SRC = os.path.join(HERE, "asm_overlap", "asm_overlap_harness.hip")
LIB = os.path.join(HERE, "asm_overlap", "libasm_overlap_harness.so")
STAMP = LIB + ".hash"
UNITS = (1, 2, 3, 6)
HDR = 8            # kAoHdr
NT, NWAVE = 256, 4
K_SPLIT, PER_WAVE = 3, 21          # split3_outputs: lanes per output, outputs per wave and pass
OMEGA_WAVES = 2                    # kAsmOmegaWaves
MAX_VEH = 16
NPARAM = 4 + 3 * MAX_VEH
SITES = ("ipm", "polish", "cold")
S_IPM, S_POL, S_COLD = range(3)
FRONT, SHIPPED = 0, 1
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
        raise RuntimeError("tests/asm_overlap/libasm_overlap_harness.so is missing or stale and "
                           "there is no hipcc to build it")
    want = source_hash()
    tmp = tempfile.mkdtemp(prefix="asm_overlap_harness_")
    try:
        def unit(ko):
            k, order = ko
            obj = os.path.join(tmp, f"unit{k}_{order}.o")
            front = ["-DSCPQP_DIAG_ASM_FRONT"] if order == FRONT else []
            cmd = ["hipcc", "-c"] + FLAGS + [f"-DAO_UNIT={k}"] + front + [SRC, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            return obj
        todo = [(k, o) for k in (3, 6, 2, 1) for o in (FRONT, SHIPPED)] + [(0, SHIPPED)]
        with ThreadPoolExecutor(min(len(todo), B._jobs())) as ex:
            objs = list(ex.map(unit, todo))
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


class AoCase(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("Hb", "site", "pidx", "lead", "inoff", "ooff", "pad0", "pad1")] + \
               [("rho", C.c_double)]


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(ensure_built())
        lib.ao_in_size.argtypes = [C.c_int] * 3
        lib.ao_plan_size.argtypes = [C.c_int] * 4 + [C.c_void_p]
        lib.ao_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(AoCase),
                               C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        _lib = lib
    return _lib


# ---------------------------------------------------------------------------------------
# the work assignment of assemble() in the shipped order, restated
# ---------------------------------------------------------------------------------------
def roff(i):
    return i * (i + 1) // 2 + ((i + 1) >> 1)


def tri_decode(t):
    i = 0
    while (i + 1) * (i + 2) // 2 <= t:
        i += 1
    return i, t - i * (i + 1) // 2


def tile_decode(t, V, PV):
    """tile_decode of the header: tile t -> (a, b, lt, mt)."""
    d, base = 0, 0
    while True:
        cnt = V * (d + 1) + PV * (2 * d + 1)
        if t < base + cnt:
            break
        base += cnt
        d += 1
    r = t - base
    if r < V * (d + 1):
        a = r // (d + 1)
        return a, a, d, r - a * (d + 1)
    r -= V * (d + 1)
    pr, q = divmod(r, 2 * d + 1)
    i_, k_ = tri_decode(pr)
    return (i_ + 1, k_, d, q) if q <= d else (i_ + 1, k_, q - (d + 1), d)


def tile_size(hg, V, Hb):
    """assemble's switch between assemble_tiles<4> and assemble_tiles<2>."""
    if not hg:
        return 4
    T4, PV = (Hb + 3) // 4, V * (V - 1) // 2
    return 4 if V * (T4 * (T4 + 1) // 2) + PV * T4 * T4 >= 2 * NT else 2


def ntiles(V, Hb, TS):
    TH = (Hb + TS - 1) // TS
    return V * (TH * (TH + 1) // 2) + V * (V - 1) // 2 * TH * TH


def omega_beside(hg, V, Hb):
    """Whether the omega row is formed beside the tiles: an LDS factor whose 4 x 4 tile pass
    is a single round."""
    return (not hg) and ntiles(V, Hb, 4) <= NT


def phase1_writes(V, O, Hb):
    """[(thread, 'Wt' | 'yb', index)]: the W~ blocks (index e = k nb + ab) and the yb entries
    (index 2 q, 2 q + 1) every thread stores in phase 1."""
    nb = V * (V + 1) // 2
    out = []
    for e in range(Hb * nb):
        tid = e % NT
        k, ab = divmod(e, nb)
        a = 0
        while (a + 1) * (a + 2) // 2 <= ab:
            a += 1
        b = ab - a * (a + 1) // 2
        out.append((tid, "Wt", e))
        if a == b:
            q = a * Hb + k
            out += [(tid, "yb", 2 * q), (tid, "yb", 2 * q + 1)]
    return out


def tile_writes(hg, V, Hb):
    """[(thread, row, col)]: the K_uu entries every thread stores in the tile pass."""
    TS = tile_size(hg, V, Hb)
    PV = V * (V - 1) // 2
    nt = ntiles(V, Hb, TS)
    out = []
    for r0 in range(0, nt, NT):
        for tid in range(NT):
            t = r0 + (NT - 1 - tid if (r0 // NT) & 1 else tid)
            if t >= nt:
                continue
            a, b, lt, mt = tile_decode(t, V, PV)
            for di in range(TS):
                for dj in range(TS):
                    l, lp = TS * lt + di, TS * mt + dj
                    if l >= Hb or lp >= Hb or (a == b and lp > l):
                        continue
                    out.append((tid, a * Hb + l, b * Hb + lp))
    return out


def virtual_wave_outputs(vw, nout):
    """[(lane, e)]: the outputs whose owner lane (term 0 of the three-lane split) lies in
    virtual wave vw (split3_outputs)."""
    out = []
    for base in range(0, nout, PER_WAVE * NWAVE):
        for j in range(PER_WAVE):
            e = base + vw * PER_WAVE + j
            if e < nout:
                out.append((K_SPLIT * j, e))
    return out


def row_n_writes(hg, V, Hb):
    """[(thread, col)]: who stores the entries of row N of H (the omega row, H[N][N] included)."""
    N = V * Hb
    out = []
    if omega_beside(hg, V, Hb):
        for w in range(NWAVE - OMEGA_WAVES, NWAVE):
            for vw in range(w - (NWAVE - OMEGA_WAVES), NWAVE, OMEGA_WAVES):
                out += [(64 * w + lane, e) for lane, e in virtual_wave_outputs(vw, N)]
    else:
        for w in range(NWAVE):
            out += [(64 * w + lane, e) for lane, e in virtual_wave_outputs(w, N)]
    return out + [(0, N)]


# ---------------------------------------------------------------------------------------
# running cases
# ---------------------------------------------------------------------------------------
def run(unit, order, cases):
    """cases: [(V, O, HM, Hb, site, lead, state, params dict, rho)]; one launch of the order's
    kernel, one workgroup per case.  Returns (launch's LDS doubles, [(before, after)]), the
    images as uint64 (the comparison is of bits)."""
    import qp_phases_harness as QH
    lib = load()
    shapes, pars, shape_of = [], [], {}
    ins, nin, seen = [], 0, {}
    desc = (AoCase * len(cases))()
    ldsN = wsN = 0
    for c, (V, O, HM, Hb, site, lead, st, par, rho) in zip(desc, cases):
        key = (V, O, HM, id(par))
        if key not in shape_of:
            shape_of[key] = len(shapes)
            shapes.append((V, O, HM))
            pars.append(QH.pack_params(par))
            sz = (C.c_int * 2)()
            if lib.ao_plan_size(unit, V, O, HM, sz) != 0:
                raise ValueError((unit, V, O, HM))
            ldsN, wsN = max(ldsN, sz[0]), max(wsN, sz[1])
        if id(st) not in seen:
            seen[id(st)] = nin
            blk = np.concatenate([np.ascontiguousarray(st[k], dtype=np.float64).reshape(-1)
                                  for k in QH.STATE_FIELDS])
            assert blk.size == lib.ao_in_size(V, O, Hb)
            ins.append(blk)
            nin += blk.size
        c.Hb, c.site, c.pidx, c.lead, c.inoff, c.rho = Hb, site, shape_of[key], lead, seen[id(st)], float(rho)
    size = ldsN + wsN
    per = HDR + 2 * size
    for i, c in enumerate(desc):
        c.ooff = i * per
    buf = np.concatenate(ins)
    out = np.zeros(per * len(cases))
    sh = np.ascontiguousarray(np.array(shapes, dtype=np.int32))
    pr = np.ascontiguousarray(np.array(pars, dtype=np.float64))
    rc = lib.ao_run(unit, order, len(shapes), sh.ctypes.data, pr.ctypes.data, len(cases), desc, buf.ctypes.data,
                    buf.size, out.ctypes.data, out.size, ldsN, wsN)
    if rc != 0:
        raise RuntimeError(f"ao_run(unit {unit}, order {order}, {len(cases)} cases) returned {rc}")
    res = []
    for i in range(len(cases)):
        o = out[i * per:(i + 1) * per]
        assert int(o[0]) == order, "the launch ran the other order's kernel"
        res.append((o[HDR:HDR + size].view(np.uint64).copy(), o[HDR + size:HDR + 2 * size].view(np.uint64).copy()))
    return ldsN, res


if __name__ == "__main__":
    print(ensure_built(verbose=True))
