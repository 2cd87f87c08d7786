"""The c2 triangular solve's sweeps hold no capture bookkeeping (scpqp_kernel.h Solver, DESIGN
§3).  Read from the ISA of kernel group 1, compiled with the compile line of
tools/isa_chain_mix.py; no GPU needed.

Per substitution step the algorithm needs one 64-bit broadcast (two ``v_readlane_b32``) and
the capture of the broadcast value into its owner lane.  With the step index a compile-time
constant the capture is two ``v_writelane_b32`` with an immediate lane; the select form
(``lane == (j & 63) ? xj : old``) costs two ``v_cndmask_b32`` per step and, for its hoisted
lane masks spilled into VGPR lanes, further readlanes (parent: 426 readlanes against the 324
of the 2 n = 162 steps, 325 selects).
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 81                  # c2: 4 vehicles x Hp 20 + 1
OUTSIDE_SWEEPS = 8      # readlanes of the phase outside the sweeps (uniform context), at most


@pytest.fixture(scope="module")
def c2_solve(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not found")
    import isa_chain_mix as CM
    fns = CM.functions(CM.listing(ROOT, 1, str(tmp_path_factory.mktemp("isa") / "k.s")))
    names = CM.demangled([n for n, _ in fns])
    hits = [body for (_, body), d in zip(fns, names)
            if re.search(r"ph_solve<false, true, 2, 3, 1>", d)]
    assert len(hits) == 1, names
    return [CM.opcode(t) for t, _ in hits[0] if not re.match(r"^\.LBB", t)]


def test_two_readlanes_per_step(c2_solve):
    n = c2_solve.count("v_readlane_b32")
    assert 2 * 2 * N <= n <= 2 * 2 * N + OUTSIDE_SWEEPS, n


def test_no_selects_in_the_sweeps(c2_solve):
    n = c2_solve.count("v_cndmask_b32")
    assert n < N / 2, n


def test_capture_is_a_writelane_per_half(c2_solve):
    # one capture per step, two halves; nothing else in the phase writes a lane
    assert c2_solve.count("v_writelane_b32") >= 2 * 2 * N
