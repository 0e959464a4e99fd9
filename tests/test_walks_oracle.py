"""tests/walks_oracle.py -- Stackster's two stack walks per pair restated in plain Python, the reads oriented and the sorted triple table
materialised -- on the six fixtures that have pairs: the table the two restatements (this one and superplus_amd/csrc/dfk_walks.h, held to
each other by tests/test_walks_cpu.py) must reproduce, which branch each seeded case of tests/walks_cases.py fires, the lowering, and the
file's layout.  CPU only."""
import struct

import numpy as np
import pytest

from tests import walks_cases, walks_oracle
from tests.walks_oracle import NOT_WALKED, SHORT, WALKED

# fixture, K, reads: pairs, walks, entries, placed, sum |EE|, longest EE, duplicate steps, walks past the edge's end, side 0 empty, side 1 empty, short edges
TABLE = [("graph_frag_k48", 48, "frag", (937, 1868, 86008, 34457, 265707, 478, 0, 1024, 6, 1, 0)), ("graph_pathy_k48", 48, "pathy", (63, 126, 32356, 10419, 32404, 507, 124, 63, 0, 0, 0)),
         ("graph_k48", 48, "reads", (48, 96, 15724, 1984, 13718, 569, 0, 12, 0, 0, 0)), ("graph_k40_nobc", 40, "reads", (138, 275, 69273, 4569, 33795, 718, 0, 0, 1, 1, 0)),
         ("graph_special_k48", 48, "special", (6, 12, 1512, 887, 1970, 196, 0, 0, 0, 0, 0)), ("graph_pathy2_k48", 48, "pathy2", (725, 1447, 289399, 90670, 400020, 610, 376, 721, 3, 1, 0))]


@pytest.mark.parametrize("case,K,which,row", TABLE, ids=[t[0] for t in TABLE])
def test_the_table_on_the_fixtures(golden_dir, case, K, which, row):
    r = walks_oracle.fixture_walks(golden_dir, case, K, which)
    got = (r["pairs"], r["walks"], r["entries"], r["placed"], r["sum_ee"], r["longest"], r["dup_steps"], r["past_edge"], r["side0_empty"], r["side1_empty"], r["short"])
    assert got == row
    recs = r["recs"]
    assert len(recs) == 2 * r["pairs"] and r["walks"] == 2 * r["pairs"] - r["side0_empty"] and r["short"] == 0        # no fixture has an edge under 48 bases
    for a, b in zip(recs[0::2], recs[1::2]):
        assert a["status"] == WALKED and b["status"] == (WALKED if a["placed"] else NOT_WALKED) and a["entries"] == b["entries"]
    for x in recs:
        if x["status"] != WALKED:
            assert (x["placed"], x["nEE"], x["M"], x["trim"], x["dup_steps"]) == (0, 0, 0, 0, 0)
            continue
        assert x["nEE"] >= 48 and x["placed"] == len(x["locs"]) <= x["entries"] and x["trim"] == max(0, x["M"] - 400)
        assert max(x["sums"]) < 60 or max(x["sums"]) < 2 * sorted(x["sums"])[2]                  # why the walk ended
        ids = [l[0] for l in x["locs"]]
        assert ids == sorted(ids)                                                                # entry order
    # the file: magic, n, two starts tables, 32-byte records, 16-byte placed records, the bases four a byte, zero bytes to a multiple of 8
    f, n = r["file"], len(recs)
    assert f[:8] == b"DFKSWLK1" and struct.unpack_from("<Q", f, 8)[0] == n
    assert len(f) == 16 + 16 * (n + 1) + 32 * n + 16 * r["placed"] + ((r["sum_ee"] + 3) // 4 + 7) // 8 * 8
    assert int(np.frombuffer(f, "<u8", n + 1, 16)[-1]) == r["placed"] and int(np.frombuffer(f, "<u8", n + 1, 16 + 8 * (n + 1))[-1]) == r["sum_ee"]
    assert struct.unpack_from("<IIIIiIii", f, 16 + 16 * (n + 1)) == (recs[0]["status"], recs[0]["entries"], recs[0]["placed"], recs[0]["dup_steps"], recs[0]["nE"], recs[0]["nEE"], recs[0]["M"], recs[0]["trim"])
    at = 16 + 16 * (n + 1) + 32 * n
    assert struct.unpack_from("<qiI", f, at) == (recs[0]["locs"][0][0], recs[0]["locs"][0][1], int(recs[0]["locs"][0][2]))
    bases = np.frombuffer(f, np.uint8, offset=at + 16 * r["placed"])
    assert [int(bases[i >> 2] >> (2 * (i & 3))) & 3 for i in range(48)] == recs[0]["EE"][:48]


def test_what_the_fixtures_hold_and_lack(golden_dir):
    f = walks_oracle.fixture_walks(golden_dir, "graph_frag_k48", 48, "frag")
    p = walks_oracle.fixture_walks(golden_dir, "graph_pathy_k48", 48, "pathy")
    assert f["live_max"] == 23 and p["live_max"] == 38 and f["trimmed"] == 23 and p["trimmed"] == 43 and f["yields"] == 930
    starts = [l[1] for r in f["recs"] for l in r["locs"]]
    assert min(starts) < 0 and 0 in starts and max(starts) > 0
    both = sum(1 for r in p["recs"] if len({l[0] for l in r["locs"]}) < len(r["locs"]))
    assert both == 0                                                               # no fixture places one read twice in a walk: the seeded SAME case has the set that could


def test_lowering():
    lower = walks_oracle.lower
    b = [1] * 19 + [2] + [1] * 40
    assert list(lower(b, [40] * 60)) == [40] * 20 + [5] * 40                       # a run of 19 stays, one of 40 goes
    b = [3] * 20 + [0] + [3] * 18 + [0] + [3] * 20                                 # a run at each end, 18 between
    q = [255] * 60; q[0:4] = [0, 4, 5, 6]; q[30] = 128; q[59] = 127
    assert list(lower(b, q)) == [0, 4, 5, 5] + [5] * 16 + [255] * 10 + [128] + [255] * 9 + [5] * 20
    assert list(lower([2] * 20, [41] * 20)) == [5] * 20 and list(lower([2] * 19, [41] * 19)) == [41] * 19 and list(lower([], [])) == []
    assert list(lower([0] * 20, [0, 1, 127, 128, 255] * 4)) == [0, 1, 5, 5, 5] * 4


def test_seeded_cases_fire_what_the_fixtures_lack():
    cases = {name: c for name, c, _ in walks_cases.seeded()}
    got = {name: walks_cases.oracle(name, c) for name, c in cases.items()}
    c, r = cases["planted"], got["planted"]
    side = {}
    for (e1, e2), a, b in zip(c["pairs"], r["recs"][0::2], r["recs"][1::2]): side[e1] = (a, b)
    s = lambda name: side[c["name"][name]]
    f = lambda x: (x["status"], x["placed"], x["nE"], x["nEE"])
    # an edge of exactly 48 bases, walked well past its end; a walk that stops inside its edge
    assert f(s("EXACT48")[0]) == (WALKED, 4, 48, 250) and [l[1] for l in s("EXACT48")[0]["locs"]] == [0, 20, 60, 100] and [l[2] for l in s("EXACT48")[0]["locs"]] == [True, False, True, True]
    assert f(s("INSIDE")[0]) == (WALKED, 3, 200, 90)
    # nobody holds the first 48-mer: on side 0 (side 1 not walked), on side 1 only
    assert f(s("NOBODY0")[0]) == (WALKED, 0, 100, 48) and f(s("NOBODY0")[1]) == (NOT_WALKED, 0, 100, 0)
    assert f(s("NOBODY1")[0]) == (WALKED, 2, 100, 153) and f(s("NOBODY1")[1]) == (WALKED, 0, 90, 48)
    # a read holding the current 48-mer twice: the step places nobody; the same read placed at a later step
    t = s("TANDEM")[0]
    assert t["dup_steps"] == 25 and t["placed"] == 4 and (c["name"]["TANDEM_R"], 85, True) in t["locs"] and t["nEE"] == 259
    assert f(s("TANDEM0")[0]) == (WALKED, 0, 60, 48) and s("TANDEM0")[0]["dup_steps"] == 1
    # start negative, zero and positive; the pair listed twice
    assert [l[1] for l in s("STARTS")[0]["locs"]] == [-7, 0, 0, 30] and c["pairs"].count((c["name"]["STARTS"], c["name"]["F"] + 1)) == 2
    # a read of exactly 48 bases is placed; reads of 47 and 10 bases never
    l48 = s("LEN48")[0]
    assert (c["name"]["LEN48_R"], 20, True) in l48["locs"] and l48["placed"] == 4 and l48["entries"] == 7 and l48["live_max"] == 3
    assert sorted(len(c["reads"][id]) for id, fw in c["reads_per"][c["ce"].index(c["name"]["LEN48"])]) == [10, 47, 48, 150, 150, 150]
    # one read with both flags in one set
    entries = walks_oracle.closer_oracle.compose(c["reads_per"][c["ce"].index(c["name"]["BOTH"])], c["reads_per"][c["ce"].index(c["name"]["F"])])
    assert len({id for id, fw in entries}) == len(entries) - 1
    # the thresholds
    assert (s("TH59")[0]["nEE"], max(s("TH59")[0]["sums"])) == (48, 59) and s("TH60")[0]["nEE"] == 49
    assert s("TWICE")[0]["nEE"] == 49 and (s("TWICE1")[0]["nEE"], sorted(s("TWICE1")[0]["sums"])[2:]) == (48, [40, 79])
    assert s("THREE")[0]["nEE"] == 49 and s("THREE")[0]["placed"] == 4
    assert (s("ZERO")[0]["nEE"], s("ZERO")[0]["sums"]) == (70, [0, 0, 0, 0])
    # lowering: a run of 19 is crossed, a run of 20 ends the walk where it begins (three reads of quality 63 lowered to 5 each)
    assert s("LOW19")[0]["nEE"] == 208 and (s("LOW20")[0]["nEE"], max(s("LOW20")[0]["sums"])) == (70, 15)
    assert (s("LOWENDS")[0]["nEE"], s("LOWENDS")[0]["placed"], max(s("LOWENDS")[0]["sums"])) == (130, 3, 15)
    assert {0, 1, 4, 5, 6, 127, 128, 190} <= {int(q) for q in c["quals"][c["reads_per"][c["ce"].index(c["name"]["LOWENDS"])][0][0]]}
    # M > 400 and trim; M <= 400 elsewhere
    assert (s("M401")[0]["M"], s("M401")[0]["trim"], s("M401")[0]["nEE"]) == (460, 60, 460) and r["trimmed"] == 1
    # the self-inverse edge as e1; e1 == inv[e2]: every read with both flags, both sides the same walk
    S = c["name"]["SELF"]
    assert c["inv"][S] == S and f(s("SELF")[0]) == (WALKED, 2, 80, 152)
    a, b = s("SAME")
    assert a["entries"] == 6 and f(a) == f(b) == (WALKED, 3, 80, 157) and a["EE"] == b["EE"] and a["locs"] == b["locs"]          # (side 1 places the same reads through their other entries: fw ^ (s == 1) is the same)
    # the live list of 1, 64, 65 and 300
    assert [s("LIVE%d" % n)[0]["live_max"] for n in (1, 64, 65, 300)] == [1, 64, 65, 300]
    # sets that are empty
    assert f(s("EMPTY")[0]) == (WALKED, 0, 70, 48) and s("EMPTY")[0]["entries"] == 0 and s("EMPTY")[1]["status"] == NOT_WALKED
    assert (r["side0_empty"], r["side1_empty"], r["short"]) == (3, 1, 0)
    # K = 40: an edge of 47 bases on side 0 and on side 1
    k = got["k40-short"]["recs"]
    assert [x["status"] for x in k] == [SHORT, NOT_WALKED, WALKED, SHORT, WALKED, WALKED] and k[0]["nE"] == k[3]["nE"] == 47 and k[2]["placed"] == 2 and got["k40-short"]["yields"] == 1
    assert got["no-pairs"]["file"] == b"DFKSWLK1" + bytes(24) and got["no-pairs"]["digest"] == (0, 0)
    assert got["tiny-3000"]["pairs"] == 1500 and len(got["tiny-3000"]["recs"]) == 3000
    for name in ("random", "random-k60"):
        assert got[name]["placed"] > 0 and got[name]["side0_empty"] > 0 and got[name]["yields"] > 0, name
    # reads at odd byte offsets, the last read ending where the buffer ends
    a = walks_cases.arrays(c)
    assert any(int(o) % 2 for o in a["read_off"]) and int(a["read_off"][-1]) == len(a["read_packed"]) and int(a["pq_off"][-1]) == len(a["pq"])
    # the bound holds on every walk (one_pair asserts it), and is not idle: EXACT48's is 48 + 4 * 102
    assert walks_oracle.ee_bound([150] * 4 + [120]) == 48 + 4 * 102 + 72
