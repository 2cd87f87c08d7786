"""The work assignment of ``assemble`` (csrc/scpqp_kernel.h) in its shipped order, from the host
restatement of its index arithmetic in tests/asm_overlap_harness.py, over every shape
V 1-8, O 0-3, Hp 1-30 and both kinds of plan (LDS factor, workspace factor):

  * every W~ block, yb entry, K_uu tile entry and omega-row entry is written exactly once;
  * a yb entry is written by the thread that writes the diagonal W~ block of its (v, k);
  * the omega row's writers hold no tile entry at or beyond row N, and where the row is formed
    beside the tiles they are lanes of the last two waves (H[N][N]: thread 0).

The assignment does not depend on O (the obstacle rows only lengthen a thread's sums), so O is
enumerated for the phase-1 check alone, where the shape's sizes are asserted."""
from collections import Counter

import pytest

import asm_overlap_harness as AH

VS, OS, HPS = range(1, 9), range(0, 4), range(1, 31)


@pytest.mark.parametrize("V", VS)
def test_phase1_writes_every_block_and_yb_entry_once(V):
    nb = V * (V + 1) // 2
    for O in OS:
        for Hb in HPS:
            w = AH.phase1_writes(V, O, Hb)
            wt = Counter(i for _, k, i in w if k == "Wt")
            yb = Counter(i for _, k, i in w if k == "yb")
            assert sorted(wt) == list(range(Hb * nb)) and set(wt.values()) == {1}, (V, O, Hb)
            assert sorted(yb) == list(range(2 * V * Hb)) and set(yb.values()) == {1}, (V, O, Hb)
            # the writer of yb[(v, k)] is the writer of the diagonal block (v, v) at k
            owner = {i: t for t, k, i in w if k == "Wt"}
            for t, k, i in w:
                if k == "yb":
                    v, kk = divmod(i // 2, Hb)
                    assert owner[kk * nb + v * (v + 1) // 2 + v] == t, (V, O, Hb, i)


@pytest.mark.parametrize("hg", (False, True), ids=("lds", "workspace"))
@pytest.mark.parametrize("V", VS)
def test_tiles_and_omega_row_are_written_once_and_apart(V, hg):
    for Hb in HPS:
        N = V * Hb
        tiles = AH.tile_writes(hg, V, Hb)
        ent = Counter((r, c) for _, r, c in tiles)
        assert set(ent.values()) == {1}, (V, Hb)
        assert sorted(ent) == [(r, c) for r in range(N) for c in range(r + 1)], (V, Hb)
        row = AH.row_n_writes(hg, V, Hb)
        cols = Counter(c for _, c in row)
        assert sorted(cols) == list(range(N + 1)) and set(cols.values()) == {1}, (V, Hb)
        writers = {t for t, _ in row}
        assert all(r < N and c < N for t, r, c in tiles if t in writers), (V, Hb)
        if AH.omega_beside(hg, V, Hb):
            assert AH.ntiles(V, Hb, 4) <= AH.NT and not hg
            assert all(t >= 64 * (AH.NWAVE - AH.OMEGA_WAVES) for t, c in row if c < N), (V, Hb)
            assert [t for t, c in row if c == N] == [0]


def test_which_shapes_take_the_omega_row_beside_the_tiles():
    """The shipped shapes: c2 / c4 (210 tiles) and c5's Hp-10 class (78) beside; c5's Hp-30
    class (528 tiles) and the workspace plans behind the tiles."""
    assert AH.ntiles(4, 20, 4) == 210 and AH.omega_beside(False, 4, 20)
    assert AH.ntiles(4, 10, 4) == 78 and AH.omega_beside(False, 4, 10)
    assert AH.ntiles(4, 30, 4) == 528 and not AH.omega_beside(False, 4, 30)
    assert not AH.omega_beside(True, 8, 30) and AH.tile_size(True, 8, 30) == 4
    assert AH.omega_beside(False, 2, 7) and AH.omega_beside(False, 1, 5)
