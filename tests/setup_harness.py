"""Build and bind tests/setup/setup_harness.hip: the squaring count of the 8x8 matrix
exponential (``expm_squarings`` of csrc/scpqp_kernel.h, a host and device function) and
``expm8`` on its own (tests/test_setup_host.py, tests/test_gpu_setup.py).

``ensure_built()`` compiles the harness with the flags of ``scpqp/build.py`` into
``tests/setup/libsetup_harness.so``.  Whether the library is current is decided by a hash of
the kernel header and the harness source, kept in a text file beside the library (file times
do not survive a copy of the tree).  A stale or missing library is rebuilt when ``hipcc`` is
there and is an error when it is not: never a skip."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import tempfile

import numpy as np

from scpqp import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "setup", "setup_harness.hip")
LIB = os.path.join(HERE, "setup", "libsetup_harness.so")
STAMP = LIB + ".hash"
NWAVE = 4
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
        raise RuntimeError("tests/setup/libsetup_harness.so is missing or stale and there is "
                           "no hipcc to build it")
    want = source_hash()
    tmp = tempfile.mkdtemp(prefix="setup_harness_")
    try:
        out = os.path.join(tmp, "lib.so")
        cmd = ["hipcc", "-shared"] + FLAGS + [SRC, "-o", out]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        shutil.move(out, LIB + ".tmp")
        os.replace(LIB + ".tmp", LIB)
        with open(STAMP, "w") as f:
            f.write(want + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return LIB


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(ensure_built())
        lib.sh_squarings.argtypes = [C.c_double]
        lib.sh_squarings.restype = C.c_int
        lib.sh_expm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib = lib
    return _lib


def squarings(nrm):
    """``expm_squarings(nrm)`` as the header computes it on the host."""
    return int(load().sh_squarings(float(nrm)))


def expm(mats, actmask=15):
    """``expm8`` of four 8x8 matrices in one workgroup, wave w taking part iff bit w of
    ``actmask`` is set.  Returns (the exponentials [4, 8, 8], zeros for the other waves;
    disturbed guard doubles; disturbed scratch doubles of the waves outside the mask)."""
    a = np.ascontiguousarray(np.asarray(mats, dtype=np.float64).reshape(NWAVE, 8, 8))
    out = np.full((NWAVE, 8, 8), np.nan)
    bad = np.full(2, -1, dtype=np.int32)
    rc = load().sh_expm(a.ctypes.data, int(actmask), out.ctypes.data, bad.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"sh_expm returned {rc}")
    return out, int(bad[0]), int(bad[1])


if __name__ == "__main__":
    print(ensure_built(verbose=True))
