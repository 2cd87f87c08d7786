"""Model-noise generator, the parts that need no GPU: the CPU mirror
(tests/noise_mirror.py) against the Philox4x32-10 known answers and the moments of its
normals; the new C-ABI (include/scpqp_noise.h): exports, ctypes layout (gcc probe of
the header) and argument validation without touching a device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import noise_mirror as NM
from scpqp import _lib as LB
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_noise.h")


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr, key, want", KNOWN_ANSWERS)
def test_mirror_philox_known_answers(ctr, key, want):
    w = NM.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(x) for x in w) == want


def test_mirror_uniform_ranges():
    """u1 in (0, 1] (the logarithm stays finite), u2 in [0, 1), at the extreme words."""
    lo = [np.uint64(0)] * 4
    hi = [np.uint64(0xFFFFFFFF)] * 4
    u1, u2 = NM.uniforms(lo)
    assert u1 == 2.0 ** -53 and u2 == 0.0
    u1, u2 = NM.uniforms(hi)
    assert u1 == 1.0 and u2 == 1.0 - 2.0 ** -53


def test_mirror_normal_moments():
    """Seed 12345, counters (e, 7, (1<<24)|(3<<8)|1, b), b < 64, e < 512 (32768 calls,
    65536 normals): mean 0 and variance 1 of the n = 65536 values and correlation 0 of
    the 32768 (z0, z1) pairs, each within 4 standard errors (1/sqrt(n), sqrt(2/n),
    1/sqrt(pairs)).  The z-scores are -0.72, 0.41 and 1.01."""
    e, b = np.meshgrid(np.arange(512), np.arange(64), indexing="ij")
    z0, z1 = NM.normals(12345, e, 7, NM.counter2(1, 3, 1), b)
    z0, z1 = z0.ravel(), z1.ravel()
    z = np.concatenate([z0, z1])
    n = z.size
    assert n == 65536 and np.all(np.isfinite(z))
    scores = (z.mean() * math.sqrt(n), (z.var() - 1.0) / math.sqrt(2.0 / n),
              np.corrcoef(z0, z1)[0, 1] * math.sqrt(z0.size))
    print("z-scores (mean, variance, correlation):", scores)
    assert all(abs(s) < 4.0 for s in scores), scores


def test_mirror_streams_are_distinct():
    """Every counter field and the seed select another stream."""
    base = NM.draws(1, 0, 0, 0, 0, 0, 4)
    others = [NM.draws(2, 0, 0, 0, 0, 0, 4), NM.draws(1 << 32 | 1, 0, 0, 0, 0, 0, 4),
              NM.draws(1, 1, 0, 0, 0, 0, 4), NM.draws(1, 0, 1, 0, 0, 0, 4),
              NM.draws(1, 0, 0, 1, 0, 0, 4), NM.draws(1, 0, 0, 0, 1, 0, 4),
              NM.draws(1, 0, 0, 0, 0, 1, 4)]
    for o in others:
        assert not np.any(o == base)
    assert not np.any(base[1:] == base[:-1])


def test_noise_header_declares_the_boundary():
    assert header_functions() == sorted(LB.NOISE_EXPORTS)
    assert not set(LB.NOISE_EXPORTS) & set(LB.EXPORTS)


def test_library_exports_every_noise_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.NOISE_EXPORTS:
        assert hasattr(lib, name)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "scpqp_noise.h"
int main(void) {
  printf("size %zu\n", sizeof(scpqp_noise));
  printf("seed %zu\n", offsetof(scpqp_noise, seed));
  printf("sigma %zu\n", offsetof(scpqp_noise, sigma));
  printf("epoch %zu\n", offsetof(scpqp_noise, epoch));
  printf("b_offset %zu\n", offsetof(scpqp_noise, b_offset));
  return 0;
}
"""


def test_noise_ctypes_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(LB.Noise)
    assert [f for f, _ in LB.Noise._fields_] == ["seed", "sigma", "epoch", "b_offset"]
    for f, _ in LB.Noise._fields_:
        assert int(got[f]) == getattr(LB.Noise, f).offset, f


def test_noise_argument_validation_without_gpu(lib):
    E_ARG, E_SIZE = -1, -4
    pp = LB.PlantParams(n_veh=2)
    pp.lf[0] = pp.lr[0] = pp.lf[1] = pp.lr[1] = 0.34
    nz = LB.Noise(seed=1, sigma=3e-6, epoch=0, b_offset=0)
    P, N = C.byref(pp), C.byref(nz)

    def delay(p=P, B=1, horizon=0.43, n_out=10, n=N):
        return lib.scpqp_delay_compensate_noisy(p, B, horizon, n_out, None, None, n, None, None,
                                                2.5e-3, None)

    def plant(p=P, B=1, n_ticks=40, tick=0.01, n=N):
        return lib.scpqp_plant_step_noisy(p, B, n_ticks, tick, None, None, n, None, 2.5e-3, None)

    def fill(n=N, B=1, V=2, site=2, k=0, n_eval=1):
        return lib.scpqp_noise_fill(n, B, V, site, k, n_eval, None, None)

    bad_pp = LB.PlantParams(n_veh=0)
    assert delay(p=C.byref(bad_pp)) == E_ARG
    assert plant(p=C.byref(bad_pp)) == E_ARG
    # null noise parameters
    assert delay(n=None) == E_ARG and b"null" in lib.scpqp_last_error()
    assert plant(n=None) == E_ARG
    assert fill(n=None) == E_ARG
    # sigma negative or not finite
    for s in (-1e-6, float("inf"), float("nan")):
        bad = C.byref(LB.Noise(seed=1, sigma=s))
        assert delay(n=bad) == E_ARG and b"sigma" in lib.scpqp_last_error()
        assert plant(n=bad) == E_ARG
        assert fill(n=bad) == E_ARG
    # sizes
    assert delay(n_out=1) == E_ARG
    assert delay(B=-1) == E_ARG
    assert delay(horizon=-0.1) == E_ARG
    assert plant(tick=0.0) == E_ARG
    assert plant(n_ticks=-1) == E_ARG
    assert plant(n_ticks=65536) == E_SIZE and b"65536" in lib.scpqp_last_error()
    assert plant(B=0, n_ticks=65536) == E_SIZE
    assert fill(V=0) == E_ARG and fill(V=17) == E_ARG
    assert fill(site=3) == E_ARG and fill(site=-1) == E_ARG
    assert fill(k=-1) == E_ARG
    assert fill(k=65536) == E_SIZE
    assert fill(n_eval=-1) == E_ARG
    assert fill(B=1 << 20, V=16, n_eval=1 << 10) == E_SIZE
    # null arrays, only reached when there is work
    assert delay(B=3) == E_ARG and b"null array" in lib.scpqp_last_error()
    assert plant(B=3) == E_ARG
    assert fill(B=3) == E_ARG
    # B = 0 (and no evaluations) is a no-op
    assert delay(B=0) == 0
    assert plant(B=0) == 0
    assert fill(B=0) == 0
    assert fill(B=3, n_eval=0) == 0
    # sigma = 0 is valid
    assert delay(B=0, n=C.byref(LB.Noise(seed=1, sigma=0.0))) == 0


def test_noise_stream_object_and_exclusive_arguments():
    from scpqp import plant as PL
    s = PL.NoiseStream(7)
    assert (s.seed, s.sigma, s.epoch, s.b_offset) == (7, 3e-6, 0, 0)
    t = s.at(5)
    assert (t.seed, t.sigma, t.epoch, t.b_offset) == (7, 3e-6, 5, 0) and s.epoch == 0
    c = PL.NoiseStream(2 ** 64 - 1, 1e-2, 3, 9).c_struct()
    assert (c.seed, c.sigma, c.epoch, c.b_offset) == (2 ** 64 - 1, 1e-2, 3, 9)
    for bad in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=1, sigma=-1.0),
                dict(seed=1, sigma=float("nan")), dict(seed=1, epoch=2 ** 32),
                dict(seed=1, b_offset=-1)):
        with pytest.raises(ValueError):
            PL.NoiseStream(**bad)
    p = PL.plant_params([0.34], [0.34])
    # both noise sources: refused before anything touches a device
    with pytest.raises(ValueError, match="not both"):
        PL.delay_compensate(p, np.zeros((1, 1, 6)), np.zeros((1, 1)), 0.43,
                            noise=np.zeros((1, 1, 2)), rng=s)
    with pytest.raises(ValueError, match="not both"):
        PL.plant_step(p, np.zeros((1, 1, 6)), np.zeros((1, 1, 5)), 0.01,
                      noise=np.zeros((1, 1, 2)), rng=s)
