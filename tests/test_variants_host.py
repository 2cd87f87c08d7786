"""Scenario variants, the parts that need no GPU: the C-ABI of include/scpqp_variants.h
(exports, the ctypes layouts against a gcc probe of the headers, argument validation
without touching a device) and ``summarize_by_variant``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from scpqp import _lib as LB
from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scpqp_variants.h")
E_ARG = -1


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^int\s+(scpqp_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LB.load()


def test_variants_header_declares_the_boundary():
    assert header_functions() == sorted(["scpqp_set_variants", "scpqp_metrics_set_variants",
                                         "scpqp_metrics_accumulate_variants"])
    assert header_functions() == sorted(LB.VARIANT_EXPORTS)
    others = set(LB.EXPORTS) | set(LB.NOISE_EXPORTS) | set(LB.METRICS_EXPORTS)
    assert not set(LB.VARIANT_EXPORTS) & others


def test_library_exports_every_variant_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s(scpqp_\w+)", out))
    assert set(header_functions()) <= exported
    for name in LB.VARIANT_EXPORTS:
        assert hasattr(lib, name)


STRUCTS = {"scpqp_batch_in": LB.BatchIn, "scpqp_params": LB.Params,
           "scpqp_metrics_params": LB.MetricsParams, "scpqp_metrics_acc": LB.MetricsAcc,
           "scpqp_metrics_dense": LB.MetricsDense}


def test_ctypes_layouts_match_the_headers(tmp_path):
    """Every structure the new entry points take, through scpqp_variants.h alone (it must
    include what it needs); scpqp_batch_in ends with the variant pointer."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "scpqp_variants.h"',
             'int main(void) {']
    for cname, cls in STRUCTS.items():
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.dirname(HEADER)}", str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in STRUCTS.items():
        assert int(got[f"{cname}.size"]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert LB.BatchIn._fields_[-1][0] == "variant"
    assert LB.BatchIn.variant.offset + C.sizeof(C.c_void_p) == C.sizeof(LB.BatchIn)
    # the member is declared last in the header, too
    txt = open(os.path.join(ROOT, "include", "scpqp.h")).read()
    body = re.search(r"typedef struct scpqp_batch_in \{(.*?)\} scpqp_batch_in;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", decl)[-1] for decl in body.split(";") if decl.strip()]
    assert names == [f for f, _ in LB.BatchIn._fields_]


def test_set_variants_argument_validation_without_gpu(lib):
    """Null pointers and n are rejected before the handle is looked at, and a call without
    a handle returns before any HIP call (this process never opens a device)."""
    P = (LB.Params * 2)()
    assert lib.scpqp_set_variants(None, 2, P) == E_ARG and b"handle" in lib.scpqp_last_error()
    assert lib.scpqp_set_variants(None, 2, None) == E_ARG and b"params" in lib.scpqp_last_error()
    assert lib.scpqp_set_variants(None, 0, P) == E_ARG and b"n < 1" in lib.scpqp_last_error()
    assert lib.scpqp_set_variants(None, -3, P) == E_ARG and b"n < 1" in lib.scpqp_last_error()
    M = (LB.MetricsParams * 2)()
    assert lib.scpqp_metrics_set_variants(None, 2, M) == E_ARG \
        and b"handle" in lib.scpqp_last_error()
    assert lib.scpqp_metrics_set_variants(None, 2, None) == E_ARG \
        and b"params" in lib.scpqp_last_error()
    assert lib.scpqp_metrics_set_variants(None, 0, M) == E_ARG \
        and b"n < 1" in lib.scpqp_last_error()
    acc = LB.MetricsAcc()
    var = (C.c_int32 * 4)()

    def accumulate(B=1, n_ticks=4, tick0=0, k_first=0):
        return lib.scpqp_metrics_accumulate_variants(None, B, n_ticks, tick0, k_first, None,
                                                     C.byref(acc), None, var, None)

    assert accumulate(k_first=2) == E_ARG and b"k_first" in lib.scpqp_last_error()
    assert accumulate(B=-1) == E_ARG and b"batch" in lib.scpqp_last_error()
    assert accumulate(tick0=-1) == E_ARG and b"tick0" in lib.scpqp_last_error()
    assert accumulate() == E_ARG and b"handle" in lib.scpqp_last_error()
    # the solve entry points still reject a null handle with the longer input structure
    bi = LB.BatchIn(variant=C.cast(var, C.c_void_p))
    bo = LB.BatchOut()
    assert lib.scpqp_solve(None, 1, C.byref(bi), C.byref(bo), None) == E_ARG


def test_summarize_by_variant():
    from scpqp import metrics as M

    def res(gaps, first, seen, ssq, xmax, margin):
        n = len(gaps)
        return dict(min_gap_veh=np.array(gaps, float), min_gap_obs=np.full(n, np.inf),
                    min_margin_veh=np.array(margin, float), min_margin_obs=np.full(n, np.inf),
                    first_collision_tick=np.array(first, np.int32),
                    n_ticks_seen=np.full(n, seen, np.int32), sum_sq_xtrack=np.array(ssq, float),
                    max_xtrack=np.array(xmax, float))

    a = res([1.0, 0.0, 2.0], [-1, 7, -1], 10, [[0.1, 0.3], [0.2, 0.2], [0.4, 0.4]],
            [[0.1, 0.2], [0.3, 0.1], [0.5, 0.6]], [0.5, -1.0, 1.0])
    b = res([3.0, 0.0], [-1, 2], 10, [[0.0, 0.0], [0.1, 0.1]], [[0.0, 0.0], [0.2, 0.1]], [2.0, -1.0])
    variant_of = [0, 1, 0, 2, 1]
    s = M.summarize_by_variant([a, b], variant_of)
    assert sorted(s) == [0, 1, 2] and all(isinstance(k, int) for k in s)
    # each entry is summarize() of that variant's realisations alone
    rows = {k: np.array(v) for k, v in a.items()}
    rows = {k: np.concatenate([rows[k], np.array(b[k])]) for k in rows}
    for k in (0, 1, 2):
        pick = np.array(variant_of) == k
        assert s[k] == M.summarize({f: v[pick] for f, v in rows.items()})
    assert s[0]["n_realisations"] == 2 and s[0]["n_collisions"] == 0
    assert s[1]["n_realisations"] == 2 and s[1]["collision_rate"] == 1.0
    assert s[1]["min_gap_veh"]["min"] == 0.0 and s[1]["frac_margin_veh_below_0"] == 1.0
    assert s[2]["n_realisations"] == 1 and s[2]["min_gap_veh"]["min"] == 3.0
    assert s[0]["xtrack_max"] == 0.6 and s[2]["xtrack_max"] == 0.0
    # one dict, a variant that occurs nowhere is absent, a wrong length is an error
    one = M.summarize_by_variant(a, np.array([5, 5, 7]))
    assert sorted(one) == [5, 7] and one[5]["n_realisations"] == 2
    with pytest.raises(ValueError):
        M.summarize_by_variant(a, [0, 1])
    with pytest.raises(ValueError):
        M.summarize_by_variant([], [])
