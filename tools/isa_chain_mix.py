"""Instruction mix of the lead wave's serial chains, from the ISA of one kernel group (no GPU).

    python tools/isa_chain_mix.py GROUP [REV]

Compiles csrc/kernels.hip for kernel group GROUP exactly as tools/isa_loop_loads.py does (the
library's flags, ``-S --cuda-device-only -gline-tables-only``) from the working tree, or from
git revision REV (with REV's headers), and prints

* per out-of-line phase (``ph_*``) its instruction count and an opcode histogram: the opcodes
  of the bookkeeping (selects, exec regions, lane moves, hazard padding) each on its own, the
  rest summed by class;
* for the solve phase (``ph_solve``) of a compile-time shape, the instructions whose source
  position, or the position of any frame they were inlined into, lies in the forward
  (``fwd*``, with the column loads) or the backward (``bwd*``, with the row loads) sweep of
  ``Solver``, per substitution step (n steps a sweep), with their own histograms.
"""
import collections
import os
import re
import sys
import tempfile
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools")]

from isa_loop_loads import PKG, functions, listing  # noqa: E402

# vehicles x horizon + 1 of the compile-time shapes (shape_c of scpqp_kernel.h)
SHAPE_N = {1: 81, 3: 241, 4: 41, 5: 81, 6: 121}
# printed on their own, in this order; everything else goes by class
NAMED = ["v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32", "v_cndmask_b32", "v_mov_b32",
         "v_cmp_eq_u32", "v_fma_f64", "v_mul_f64", "v_add_f64", "s_nop", "s_waitcnt",
         "s_and_saveexec_b64", "s_or_b64", "s_cbranch_execz", "s_cbranch_execnz", "s_barrier"]
CLASSES = [("ds_read*", r"ds_read"), ("ds_write*", r"ds_write"), ("global_load*", r"global_load"),
           ("global_store*", r"global_store"), ("scratch_*", r"scratch_"), ("s_load*", r"s_(buffer_)?load"),
           ("v_cmp*", r"v_cmpx?_"), ("s_branch*", r"s_c?branch"), ("other v_*", r"v_"), ("other s_*", r"s_")]


def opcode(text):
    op = text.split()[0]
    return re.sub(r"_e(32|64)$", "", op)


def histogram(ops):
    """[(name, count)] in the order NAMED, then CLASSES; zero counts left out."""
    cnt = collections.Counter(ops)
    rows = [(k, cnt.pop(k)) for k in NAMED if k in cnt]
    for name, pat in CLASSES:
        ks = [k for k in cnt if re.match(pat, k)]
        n = sum(cnt.pop(k) for k in ks)
        if n:
            rows.append((name, n))
    if cnt:
        rows.append(("other", sum(cnt.values())))
    return rows


def fmt(rows):
    return "  ".join(f"{k} {n}" for k, n in rows)


def sweep_ranges(header):
    """{"fwd": [(first, last)], "bwd": [...]}: the member functions fwd* / bwd* of Solver."""
    lines = open(header).read().splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r"^struct Solver", ln))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("};"))
    res = {"fwd": [], "bwd": []}
    i = start
    while i < end:
        m = re.search(r"void (fwd|bwd)\w*\(", lines[i])
        if m and lines[i].startswith("    __device__"):
            j = next(k for k in range(i, end) if lines[k].startswith("    }"))
            first = i
            while first > start and re.match(r"^\s*(template|//)", lines[first - 1]):
                first -= 1
            res[m.group(1)].append((first + 1, j + 1))
            i = j
        i += 1
    return res


def demangled(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                          text=True).stdout.splitlines()


def main():
    group = int(sys.argv[1])
    rev = sys.argv[2] if len(sys.argv) > 2 else None
    with tempfile.TemporaryDirectory() as tmp:
        tree = ROOT
        if rev:
            tree = os.path.join(tmp, "rev")
            os.makedirs(tree)
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "include", PKG + "/csrc"],
                                 check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
        rng = sweep_ranges(os.path.join(tree, PKG, "csrc", "scpqp_kernel.h"))
        fns = functions(listing(tree, group, os.path.join(tmp, "k.s")))
    print(f"# kernel group {group}, {rev or 'working tree'}; sweep source ranges {rng}")
    for (name, body), full in zip(fns, demangled([n for n, _ in fns])):
        m = re.search(r"\b(ph_\w+)<([^>]*)>", full)
        if not m:
            continue
        insts = [(t, chain) for t, chain in body if not re.match(r"^\.LBB", t)]
        print(f"{m.group(1)}<{m.group(2).replace(' ', '')}>: {len(insts)} instructions")
        print("    " + fmt(histogram([opcode(t) for t, _ in insts])))
        if m.group(1) != "ph_solve":
            continue
        sh = int(m.group(2).split(",")[-1])
        n = SHAPE_N.get(sh)
        for what in ("fwd", "bwd"):
            ops = [opcode(t) for t, chain in insts
                   if any(a <= ln <= b for ln in chain for a, b in rng[what])]
            per = f", {len(ops) / n:.2f} per step (n = {n})" if n else " (run-time shape, rolled)"
            print(f"  solve:{what}: {len(ops)} instructions{per}")
            print("    " + fmt(histogram(ops)))


if __name__ == "__main__":
    main()
