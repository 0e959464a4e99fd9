"""tests/cons_oracle.py -- CloseGap2's read stacks and their column consensus restated in plain Python, every stack materialised -- on the
four fixtures that have pairs: the table the two restatements (this one and superplus_amd/csrc/dfk_cons.h, held to each other by
tests/test_cons_cpu.py) must reproduce, what the fixtures hold and what they lack, and the file's layout.  CPU only."""
import struct

import numpy as np
import pytest

from tests import cons_oracle

# fixture, K, reads: pairs, stacks, rows, rows_kept, trimmed, columns, partner rows, side-0 stacks reversed
TABLE = [("graph_pathy2_k48", 48, "pathy2", (725, 1450, 98552, 92988, 555, 456411, 265, 2)), ("graph_frag_k48", 48, "frag", (937, 1874, 39363, 39363, 0, 318533, 2168, 0)),
         ("graph_pathy_k48", 48, "pathy", (63, 126, 11048, 10627, 43, 37530, 45, 0)), ("graph_k40_nobc", 40, "reads", (138, 276, 24631, 16658, 171, 101084, 7, 1))]


@pytest.mark.parametrize("case,K,which,row", TABLE, ids=[t[0] for t in TABLE])
def test_the_table_on_the_fixtures(golden_dir, case, K, which, row):
    r = cons_oracle.fixture_cons(golden_dir, case, K, which)
    assert (r["pairs"], r["n_stacks"], r["rows"], r["rows_kept"], r["trimmed"], r["columns"], r["partner_rows"], r["side0_reversed"]) == row
    assert r["reversed"] == r["pairs"] + r["side0_reversed"]                       # side 1 always, side 0 where e1 == inv[e2]
    for s, d, a, b in zip(r["stacks"], r["dims"], r["starts"], r["starts"][1:]):
        assert d == (s["rows"], s["rows_kept"], s["M"], s["cols"]) and b - a == s["cols"] == min(s["M"], cons_oracle.MAX_WIDTH)
        assert s["rows_kept"] == s["rows"] or s["trimmed"]
    assert len(r["bases"]) == r["columns"] and (int(r["bases"].max()) <= 3 if r["columns"] else True)
    # the file: magic, n, starts, dims, bases, zero bytes to a multiple of 8
    f, n = r["file"], r["n_stacks"]
    assert f[:8] == b"DFKCCON1" and struct.unpack_from("<Q", f, 8)[0] == n and len(f) == 16 + 8 * (n + 1) + 16 * n + (r["columns"] + 7) // 8 * 8
    assert list(np.frombuffer(f, "<u8", n + 1, 16)) == r["starts"] and struct.unpack_from("<IIiI", f, 16 + 8 * (n + 1)) == r["dims"][0]
    at = 16 + 8 * (n + 1) + 16 * n
    assert f[at:at + r["columns"]] == r["bases"].tobytes() and not any(f[at + r["columns"]:])


def test_what_the_fixtures_hold(golden_dir):
    r = cons_oracle.fixture_cons(golden_dir, "graph_pathy2_k48", 48, "pathy2")
    assert (r["tied"], r["empty"], r["lost_rows"]) == (928, 1596, 394)            # tied columns, columns no read covers, stacks that lose rows to the trim
    assert r["live"] < r["rows"] and r["added"] > 0
    f = cons_oracle.fixture_cons(golden_dir, "graph_frag_k48", 48, "frag")
    assert f["trimmed"] == 0 and f["rows_kept"] == f["rows"]                       # no stack of frag is wider than 400: nothing is erased, however empty


def test_chars_sums_and_the_first_maximum():
    assert list(cons_oracle.as_char([0, 127, 128, 255])) == [0, 127, -128, -1]
    B = np.array([[0], [0], [0], [1], [1], [1]]); Q = np.array([[2], [10], [10], [20], [0], [0]])
    con, added, sums = cons_oracle.consensus(B, Q)
    assert list(con) == [1] and added == 6 and (sums[0][0], sums[1][0]) == (20.2, 20.200000000000003)
    con, _, _ = cons_oracle.consensus(np.array([[3], [0]]), np.array([[10], [10]]))
    assert list(con) == [0]                                                        # a tie: the first
    con, added, _ = cons_oracle.consensus(np.full((2, 3), cons_oracle.UNDEF), np.full((2, 3), -1))
    assert list(con) == [0, 0, 0] and added == 0                                   # nothing added: base 0
    Br, Qr = cons_oracle.reverse(np.array([[0, cons_oracle.UNDEF, 1]]), np.array([[5, -1, 7]]))
    assert Br.tolist() == [[2, cons_oracle.UNDEF, 3]] and Qr.tolist() == [[7, -1, 5]]
    Bt, Qt = cons_oracle.trim(np.array([[0, 1, 2], [3, 3, 3]]), np.array([[5, -1, -1], [-1, 4, -1]]), 1, 3)
    assert Bt.tolist() == [[3, 3]] and Qt.tolist() == [[4, -1]]
