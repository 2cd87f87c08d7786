"""Build and bind tests/linalg/linalg_harness.hip: the factorisation and the triangular
solves of csrc/scpqp_kernel.h, callable per case (tests/test_gpu_linalg.py).

``ensure_built()`` compiles the harness with the flags of ``scpqp/build.py`` into
``tests/linalg/liblinalg_harness.so``.  Whether the library is current is decided by a hash
of the kernel header and the harness source, kept in a text file beside the library (file
times do not survive a copy of the tree).  A stale or missing library is rebuilt when
``hipcc`` is there and is an error when it is not: never a skip.

The module also restates the header's ``roff`` and ``pad2`` (tests/test_linalg_host.py holds
them to the header's own) and packs cases for ``lh_run``."""
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
SRC = os.path.join(HERE, "linalg", "linalg_harness.hip")
LIB = os.path.join(HERE, "linalg", "liblinalg_harness.so")
STAMP = LIB + ".hash"
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (1, 4))    # (HG, RM) the product instantiates
CT_ORDERS = (41, 81, 121, 241)      # n of the compile-time shapes (shape_c: V H + 1)
HDR = 8                             # kLhHdr
FLAGS = ["--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
         f"-I{B.INCLUDE}"]


def pad2(x):
    return (x + 1) & ~1


def roff(i):
    """Offset of row i of the packed lower triangle: i + 1 entries, padded to an even count."""
    return i * (i + 1) // 2 + ((i + 1) >> 1)


def factor_doubles(n):
    """What the plan allocates for the factor: the packed K, a spare row, 16 more."""
    return pad2(roff(n + 1) + 16)


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
        raise RuntimeError("tests/linalg/liblinalg_harness.so is missing or stale and there is "
                           "no hipcc to build it")
    want = source_hash()
    tmp = tempfile.mkdtemp(prefix="linalg_harness_")
    try:
        def unit(k):
            obj = os.path.join(tmp, f"pair{k}.o")
            cmd = ["hipcc", "-c"] + FLAGS + [f"-DLH_PAIR={k}", SRC, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            return obj
        # the pairs with the most unrolled solves first
        with ThreadPoolExecutor(min(7, B._jobs())) as ex:
            objs = list(ex.map(unit, (6, 5, 4, 3, 2, 1, 0)))
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


class LhCase(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n", "lead", "koff", "form", "nrhs", "boff", "ooff", "pad")]


_lib = None


def load(path=None):
    """The bound library.  ``path``: another build of the harness (a variant of the header under
    study) instead of the tree's own, for the rest of the process."""
    global _lib
    if _lib is None or path is not None:
        lib = C.CDLL(path or ensure_built())
        for name in ("lh_roff", "lh_pad2", "lh_red_size", "lh_factor_doubles"):
            getattr(lib, name).argtypes = [C.c_int]
        lib.lh_ld_alloc.argtypes = [C.c_int, C.c_int]
        lib.lh_out_doubles.argtypes = [C.c_int, C.c_int]
        lib.lh_run.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(LhCase), C.c_void_p, C.c_longlong,
                               C.c_void_p, C.c_longlong, C.c_void_p]
        _lib = lib
    return _lib


def pack_lower(K):
    """The lower triangle of K row by row: entry (i, j) at i (i + 1) / 2 + j."""
    return np.ascontiguousarray(K[np.tril_indices(K.shape[0])], dtype=np.float64)


def unpack_lower(v, n):
    L = np.zeros((n, n))
    L[np.tril_indices(n)] = v
    return L


class Result:
    """One case's output: ok (cholesky's return value), L (unit lower: the strictly lower
    entries of the device's H, the diagonal set to one), dinv, x [nrhs, n], bad (the four
    counts of disturbed canaries)."""
    def __init__(self, n, nrhs, o, bad):
        F = n * (n + 1) // 2
        self.ok = o[0] == 1.0
        self.L = np.tril(unpack_lower(o[HDR:HDR + F], n), -1) + np.eye(n)
        self.dinv = o[HDR + F:HDR + F + n].copy()
        self.x = o[HDR + F + n:HDR + F + n + nrhs * n].reshape(nrhs, n).copy()
        self.bad = tuple(int(v) for v in bad)


def run(hg, rm, cases):
    """cases: [(K, lead, form, rhs)] with K [n, n] symmetric (its lower triangle is used),
    form 0 (run-time n) or n itself (a compile-time shape), rhs [nrhs, n].  One launch, one
    workgroup per case, in the order given.  Returns [Result]."""
    lib = load()
    desc = (LhCase * len(cases))()
    ins, nin, nout = [], 0, 0
    seen = {}      # an array object passed for several cases is uploaded once

    def place(key, make):
        nonlocal nin
        if key not in seen:
            seen[key] = nin
            ins.append(make())
            nin += ins[-1].size
        return seen[key]
    for c, (K, lead, form, rhs) in zip(desc, cases):
        n = K.shape[0]
        rhs2 = np.asarray(rhs, dtype=np.float64).reshape(-1, n)
        c.n, c.lead, c.form, c.nrhs = n, lead, form, rhs2.shape[0]
        c.koff = place(("K", id(K)), lambda: pack_lower(K))
        c.boff = place(("b", id(rhs)), lambda: rhs2.reshape(-1).copy())
        c.ooff = nout
        nout += lib.lh_out_doubles(n, rhs2.shape[0])
    buf = np.concatenate(ins)
    out = np.zeros(nout)
    bad = np.zeros((len(cases), 4), dtype=np.int32)
    rc = lib.lh_run(hg, rm, len(cases), desc, buf.ctypes.data, buf.size, out.ctypes.data, out.size,
                    bad.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"lh_run({hg}, {rm}, {len(cases)} cases) returned {rc}")
    return [Result(c.n, c.nrhs, out[c.ooff:], bad[i]) for i, c in enumerate(desc)]


if __name__ == "__main__":
    print(ensure_built(verbose=True))
