"""The hot-layout traces (tests/hotlayout.py) are what they claim to be -- on the CPU oracle and the restated rules alone, no GPU:
every case is one pass, its hot sub or bin holds exactly the c records of the hot key, every piece or group holds the count the
layout promises, and the case's expectation (stays in closed form / refused, and by which counter) follows from those counts.
Every generated case goes through here; none is skipped."""
import numpy as np
import pytest

import hotlayout as hl
import kvkeys
import opwords as ow
from dint_amd import wire

W = wire.Workload
NAMES = list(hl.CASES)


def test_the_rules_on_their_own():
    """piece_of is monotone, covers [0, np) and clamps at the top index; ranges are its level sets; the thresholds sit where the
    issue says"""
    for n, n_p in ((4096, 4), (5000, 64), ((1 << 19) + 1, 3), (1 << 20, 64), (65536, 128), (777, 5)):
        p = hl.piece_of(np.arange(n), n_p, n)
        assert p[0] == 0 and p[-1] == n_p - 1 and (np.diff(p) >= 0).all() and (np.diff(p) <= 1).all()
        for j, (lo, hi) in enumerate(hl.ranges(n, n_p)):
            assert p[lo] == j == p[hi] and (lo == 0 or p[lo - 1] == j - 1)
    r = hl.kv_rule(W.TATP)
    assert r == (65, 384, 64) and hl.kv_rule(W.SMALLBANK) == (65, 384, 128) and hl.kv_rule(W.STORE, "nosplit") is None
    assert hl.kv_rule(W.TATP, "t16") == (65, 16, 64) and hl.kv_rule(W.SMALLBANK, "sb-t64") == (200, 64, 128) and hl.kv_rule(W.SMALLBANK, "sb-off") is None
    assert [hl.listing(h, r) for h in (64, 65, 384, 385, 24_576, 24_577)] == [("small", 0), ("solo", 1), ("solo", 1), ("pieces", 2), ("pieces", 64), ("sub", 0)]
    assert hl.listing(49_152, hl.kv_rule(W.SMALLBANK)) == ("pieces", 128) and hl.listing(49_153, hl.kv_rule(W.SMALLBANK)) == ("sub", 0)
    assert [hl.stretches(c, 16384) for c in (4096, 4097, 8176, 8177)] == [1, 2, 2, 3]


def test_the_knob_sets_are_the_hot_key_tests_own():
    from test_gpu_kv import SB_KNOBS, SPLIT_KNOBS

    for name, (env, flags) in hl.KNOBS.items():
        if not name.startswith("lk-") and name != "rounds":
            assert env in SPLIT_KNOBS + SB_KNOBS, name


def test_every_case_is_run():
    assert len(NAMES) == len(set(NAMES)) and all(knobs and knobs[0] in hl.KNOBS for _, knobs in hl.CASES.values())
    large = [n for n in NAMES if n.endswith(("2^19+1-alone", "2^20-alone"))]
    assert sorted(large) == sorted(f"{w}-extremes-{s}-alone" for w in ("store", "tatp", "smallbank") for s in ("2^19+1", "2^20"))  # two per workload


def _kv_case_holds(c):
    wl, p0 = c.wl, c.passes[0]
    hs, fs = hl.hot_sel(c), hl.foreign_sel(c)
    assert len(p0) == c.n <= min(hl.PASS_MAX, c.log_cap or hl.PASS_MAX)  # one pass: within the engine's largest, and within its log ring
    assert int(hs.sum()) == c.c
    types = p0["type"]
    if c.variant != "traffic":
        # the hot sub holds exactly the hot pair's records: every other request is a filler (finished by the partition) or,
        # "neighbour", one of six requests on two other keys of the hot bucket
        other = ~(hs | fs)
        nb = other & (types != hl.FILLER[wl])
        assert int(nb.sum()) == (6 if c.variant == "neighbour" else 0)
        if c.variant == "neighbour":
            size = hl._hash_size(wl, c.table)
            b, q, kh = kvkeys.key_sig(p0["key"][nb], size)
            b0, q0, kh0 = kvkeys.key_sig([c.key], size)
            assert (b == b0).all() and (kh != kh0).all() and (wl == W.STORE or len(set((q == q0).tolist())) == 2)
            assert wl == W.STORE or (p0["table"][nb] == c.table).all()
        assert c.bad == (int((types == 99).sum()) if wl == W.STORE else 0)
        if wl == W.STORE:
            assert c.errors == c.bad  # (the oracle counts them too; the ordinary pass adds none)
    if c.foreign is not None:
        size = hl._hash_size(wl, c.table)
        assert [int(x[0]) for x in kvkeys.key_sig([c.foreign], size)][:2] == [int(x[0]) for x in kvkeys.key_sig([c.key], size)][:2]  # one counter pair
    # the hot row is there before the pass, or is not, as the case says (tatp's CALL_FORWARDING row: as lay_cf found it)
    if "exists" in c.promise:
        assert hl.row_exists(c) == c.promise["exists"], (c.name, c.promise["exists"])
    else:
        assert c.name.startswith("tatp-cf-even")  # (no struct op: the layout does not depend on it)
    # every writer's value and version payload is its own
    wr = hs & np.isin(types, hl.WRITERS[wl])
    if wr.any():
        assert len(np.unique(p0["val"][wr], axis=0)) == int(wr.sum()) == len(np.unique(p0["ver"][wr]))
    # the counts the layout promises, under the knob set it is cut for
    kind, n_p, per, fper = hl.piece_counts(c, c.built)
    pr = c.promise
    if "np" in pr:
        assert (kind, n_p) == ("pieces" if pr["np"] > 1 else "solo", pr["np"]), (kind, n_p, pr["np"])
    if "per" in pr:
        assert per == pr["per"], (per, pr["per"])
    if "fper" in pr:
        assert fper == pr["fper"] and sum(per) == c.c + sum(fper)
    idx = np.nonzero(hs)[0]
    if "edges" in pr:
        R = hl.ranges(c.n, n_p)
        assert pr["edges"] == [(R[j][1], R[j + 1][0]) for j in range(n_p - 1)] and all(b == a + 1 for a, b in pr["edges"])
        for a, b in pr["edges"]:
            assert hs[a] and hs[b]
    if "first" in pr:
        assert idx[0] == 0 and idx[-1] == c.n - 1 and types[c.n - 1] in hl.WRITERS[wl] and types[0] in hl.WRITERS[wl]
    if "struct_piece" in pr:
        st = np.nonzero(hs & ~np.isin(types, hl.SIMPLE[wl]))[0]
        assert len(st) == 2 and set(hl.piece_of(st, n_p, c.n).tolist()) == {pr["struct_piece"]}
        assert types[st].tolist() == ([22, 18] if pr["exists"] else [18, 22])  # DELETE then INSERT of a row that exists, else the other way round
    if "m" in pr:
        assert int((hs & np.isin(types, hl.WRITERS[wl] + hl.LOCK_OPS[wl])).sum()) == pr["m"]
    return kind, n_p, per, fper


def _kv_expectation_follows(c, kind, n_p, per, fper):
    """the counters `kv_counters` predicts are the ones the counts imply, spelt out once more for the cut the layout is built for"""
    if c.variant != "alone":
        return
    types = c.passes[0]["type"][hl.hot_sel(c) | hl.foreign_sel(c)]
    simple = bool(np.isin(types, hl.SIMPLE[c.wl]).all())
    for knobs in hl.CASES[c.name][1]:
        want = hl.kv_counters(c, knobs)
        k2, np2, per2, fper2 = hl.piece_counts(c, knobs)
        refused = k2 == "pieces" and (max(per2) > hl.KVB_T or not simple or max(fper2 + [0]) > hl.KSB_FMAX)
        solo_refused = k2 == "solo" and c.wl == W.SMALLBANK and max(fper2 + [0]) > hl.KSB_FMAX
        listed_late = k2 == "sub" and c.wl != W.SMALLBANK and hl.kv_rule(c.wl, knobs) is not None
        assert want is not None, (c.name, knobs)  # (no case leaves its counters to a path the rules do not decide)
        if refused or solo_refused or listed_late:
            assert want[0] == int(len(types)) and sum(want[1]) >= 1, (knobs, want)
            if c.wl == W.SMALLBANK:  # which counter: [0] a piece over 512, [1] a piece over 8 foreign requests
                assert want[1] == [sum(x > hl.KVB_T for x in per2), sum(x > hl.KSB_FMAX for x in fper2), 0]
        else:
            assert want == (0, [0, 0, 0]), (knobs, want)
    # and what each layout is FOR, under its own cut
    want = hl.kv_counters(c, c.built)
    name = c.name
    if "-full-513" in name:
        assert max(per) == hl.KVB_T + 1 and want[0] == c.c and want[1][0 if c.wl == W.SMALLBANK else 2] == 1
    if "-full-512" in name or "all-full" in name or "seven-full" in name:
        assert max(per) == hl.KVB_T and want == (0, [0, 0, 0])
    if "foreign-8" in name or "foreign-1-" in name:
        assert max(fper) in (1, hl.KSB_FMAX) and want == (0, [0, 0, 0])
    if "foreign-9" in name:
        assert max(fper) == hl.KSB_FMAX + 1 and want == (c.c + 9, [0, 1, 0])
    if c.foreign is not None:  # cut around the foreign key, every populated piece holds more than 8 of the hot row's: refused
        alt = hl.kv_counters(c, c.built, around="foreign")
        assert alt == (len(types), [0, sum(a - b > hl.KSB_FMAX for a, b in zip(per, fper)), 0]) and alt[1][1] == n_p
    if "own-insert" in name:
        assert want == (c.c, [0, 0, 1])
    if any(s in name for s in ("-front", "-back", "-gap", "-straddle", "-extremes", "-even-")) and "cf" not in name:
        assert want == (0, [0, 0, 0]), (name, want)
    if "gap" in name:
        assert sum(x == 0 for x in per) == n_p - 2 and per[0] and per[-1]
    if "np64" in name:
        assert n_p == 64


def _lock_case_holds(c):
    p0 = c.passes[0]
    hs = hl.hot_sel(c)
    n_bins_min = 32
    assert len(p0) == c.n and (c.n <= hl.TPL_HOT_NMAX or c.engine.get("max_pass", 0) >= c.n)  # one pass
    assert int(hs.sum()) == c.c and c.n > 16 * n_bins_min
    slot = ow.lid_slot(p0["lid"], c.n_slots)
    hot_slot = int(ow.lid_slot([c.key], c.n_slots)[0])
    line = (slot >> 4) == (hot_slot >> 4)
    if c.variant == "alone":
        # the hot bin = the low pbits >= 5 bits of the line number: exactly the hot slot's records and the promised others of its line
        assert int((((slot >> 4) & (n_bins_min - 1)) == ((hot_slot >> 4) & (n_bins_min - 1))).sum()) == c.c + c.promise["rest"]
        assert int((line & ~hs).sum()) == c.promise["rest"]
    idx = np.nonzero(hs)[0]
    pr = c.promise
    if "groups" in pr:
        g, cnt = np.unique(idx // hl.LK_GROUP, return_counts=True)
        assert g.tolist() == sorted(pr["groups"]) and (cnt == pr["per_group"]).all()
    if "edge" in pr:
        e = pr["edge"]
        assert e % hl.LK_GROUP == 0 and hs[e - 3:e + 3].all()
        rep = c.want[0]
        G, R = wire.Tpl.GRANT_LOCK, wire.Tpl.REJECT_LOCK
        acts = rep["action"][[e - 3, e - 2, e, e + 2]].tolist() if pr["order"] == "sx" else rep["action"][[e - 3, e - 1, e, e + 2]].tolist()
        assert acts == ([G, R, G, G] if pr["order"] == "sx" else [G, G, R, G]), acts
    if "commits" in c.name:
        assert c.c == hl.TPL_HOT_NMAX == c.n and (p0["type"] == wire.Fasst.COMMIT).all()
    if "acquire-abort" in c.name:
        assert c.c == hl.TPL_HOT_NMAX and set(p0["type"].tolist()) == {int(wire.Fasst.ACQUIRE_LOCK), int(wire.Fasst.ABORT)}
    if "-rest-" in c.name:
        assert pr["rest"] in (hl.LK_REST, hl.LK_REST + 1) and c.c >= hl.KVB_HOT_MIN_LOCKS and 2 * c.c >= c.c + pr["rest"]
    if "group" in c.name and c.built.startswith("lk-min32"):
        assert 32 <= c.c < hl.KVB_HOT_MIN_LOCKS and c.c + pr["rest"] > hl.LK_BINCAP and 2 * c.c >= c.c + pr["rest"]


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_what_it_promises(name):
    c = hl.case(name)
    assert c.name == name and len(c.passes) == 2 and len(c.want) == 2 and c.built == hl.CASES[name][1][0]
    if c.wl in hl.KV:
        _kv_expectation_follows(c, *_kv_case_holds(c))
    else:
        _lock_case_holds(c)
