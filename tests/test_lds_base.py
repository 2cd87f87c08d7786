"""The solver kernels address their dynamic LDS from a base that the kernel forms once and
hands to every out-of-line function (scpqp_kernel.h lds_base_opaque).  Read from
the built library's gfx950 code objects; no GPU needed.

A device function other than the kernel that names the dynamic LDS array makes the compiler
emit ``llvm.amdgcn.dynlds.offset.table`` (one entry per kernel, in global memory) and fetch
the array's address from it at every such reference: a memory round trip on the lead wave's
chain in every phase and inside the panel-step loop.  And the memory plans put the dynamic
LDS at offset 0, so no solver kernel may own static LDS.
"""
import os
import re
import subprocess
import sys

import pytest

from scpqp.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

TABLE = "llvm.amdgcn.dynlds.offset.table"


def table_symbols(lib, tmp):
    """(code object index, llvm-readelf -s line) of every offset-table symbol in the library."""
    hits = []
    objs = KR.code_objects(lib)
    assert objs, f"{lib}: no gfx950 code object"
    for i, co in enumerate(objs):
        path = os.path.join(str(tmp), f"co{i}.elf")
        with open(path, "wb") as fh:
            fh.write(co)
        out = subprocess.run([os.path.join(KR.LLVM, "llvm-readelf"), "-s", "-W", path], check=True,
                             capture_output=True, text=True).stdout
        hits += [(i, ln.strip()) for ln in out.splitlines() if TABLE in ln]
    return hits


@pytest.fixture(scope="module")
def library():
    if not os.path.exists(LIB_PATH):
        pytest.fail("libscpqp.so not built: run __graft_entry__.build()")
    return LIB_PATH


def test_no_dynamic_lds_offset_table(library, tmp_path):
    hits = table_symbols(library, tmp_path)
    assert not hits, "a non-kernel device function references the dynamic LDS array: %r" % hits


def test_no_solver_kernel_has_static_lds(library):
    ks = KR.kernels(library)
    names = KR.demangle([k["name"] for k in ks])
    scp = [(d, k) for k, d in zip(ks, names) if "scp_kernel<" in d]
    # every instantiation of the shipped library (kernels.hip outside its SCPQP_DIAG blocks)
    kern = open(os.path.join(ROOT, "senquential-convex-programming-for-trajectory-planning_amd",
                             "csrc", "kernels.hip")).read().split("#define SCPQP_INST")[1]
    pat = r"SCPQP_INST\((\w+), (\w+), (\d), (\d), (\d)\)"
    diag = set(re.findall(r"#ifdef SCPQP_DIAG[^\n]*\n" + pat, kern))
    want = {"scp_kernel<%s, %s, %s, %s, %s>" % t for t in re.findall(pat, kern) if t not in diag}
    got = {re.search(r"scp_kernel<[^>]*>", d).group(0) for d, _ in scp}
    assert got == want
    bad = {d: k["group_segment_fixed_size"] for d, k in scp if k["group_segment_fixed_size"] != 0}
    assert not bad, f"static LDS beside the plan's dynamic LDS: {bad}"
