"""A server's tables and overflow pool verified on the GPU and leaked entries reclaimed (include/dint_abi.h dint_state_verify,
dint_amd/csrc/k_verify.hip, dint_amd/recovery.py verify_tables): every hand-built view of tests/test_state_verify_host.py run
through the kernels (include/dint_driver.h dint_state_verify_view) against the host form and the numpy form, and live engines
against numbers that other calls report -- state_stats, state_digest, the exported image, a twin engine's replies.  The damaged
views are inputs the rule must bound, as the bent images of test_gpu_state_image.py are.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from test_gpu_state_rehash import _delete_rows, _store_insert, _store_read, _tatp_trace, _vals, chained  # noqa: F401
from test_state_verify_host import (ESTATE, RECLAIM, all_cases, assert_identities, expected, host_verify, is_clean)

W, T = wire.Workload, wire.Tatp
EINVAL = -1
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
pytestmark = pytest.mark.gpu
CASES = all_cases()


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def _up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


def dev_verify(view, flags=0):
    """the view uploaded and run through dint_state_verify_view: (rc, reports, the bytes downloaded afterwards)"""
    import torch

    dev = [[_up(x) for x in (t.entries, t.pool_next, t.ctl)] for t in view.tabs]
    cv = view.c_view()
    for i, (e, n, c) in enumerate(dev):
        cv.table[i].entries, cv.table[i].pool_next, cv.table[i].ctl = e.data_ptr(), n.data_ptr() if n.numel() else 0, c.data_ptr()
    out = (_lib.TableVerify * 5)()
    torch.cuda.synchronize()
    rc = _lib.load().dint_state_verify_view(torch.cuda.current_device(), C.byref(cv), out, 5, flags, None)
    torch.cuda.synchronize()
    return rc, [out[t].as_dict() for t in range(len(view.tabs))], [tuple(x.cpu().numpy().tobytes() for x in d) for d in dev]


def _clean(e, **kw):
    rep = e.state_verify(**kw)
    for r in rep:
        assert is_clean(r), r
        assert_identities(r)
    return rep


# ---------------------------------------------------------------------------------------------- 1. views on the device
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_view_on_the_device_equals_the_host_form_equals_the_numpy_form(name):
    _, view, flags = next(c for c in CASES if c[0] == name)
    want_rc, want, after = expected(view, flags)
    rc, got, raw = dev_verify(view, flags)
    host = view.copy()
    hrc, hgot = host_verify(host, flags)
    assert rc == hrc == want_rc, _lib.load().dint_last_error()
    for t, (g, h, w) in enumerate(zip(got, hgot, want)):
        assert g == h == w, (name, t, {k: (g[k], h[k], w[k]) for k in w if not g[k] == h[k] == w[k]})
        assert_identities(g)
    assert raw == after.raw() == host.raw()  # a reclaim's bytes; a census and a refused reclaim: unchanged
    if want_rc == ESTATE:
        assert raw == view.raw()


# ---------------------------------------------------------------------------------------------- 2. a blank engine stays blank
@pytest.mark.parametrize("wl", [W.STORE, W.TATP, W.SMALLBANK])
def test_a_blank_engine_reports_zeros_and_stays_blank(wl):
    kw = dict(n_rows=64) if wl == W.STORE else dict(n_rows=64, log_entries=1 << 12)
    e = _engine(wl, **kw)
    for reclaim in (False, True):  # nothing to reclaim: still blank
        rep = e.state_verify(reclaim=reclaim)
        assert len(rep) == NTAB[wl]
        for t, r in enumerate(rep):
            assert r["pool_cap"] == e.hash_size(t) // 4 + 4096
            assert all(v == 0 for k, v in r.items() if k != "pool_cap"), r
    twin = _engine(wl, **kw)
    twin.populate(50)
    buf, n, st = twin.state_export(0, 1)
    assert e.state_import(buf, n)["rows"] == st["rows"] > 0  # the import's own rule says it was blank
    assert e.state_digest() == twin.state_digest()
    _clean(e)
    e.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 3. chains, holes, recycled entries
def test_the_chained_store_is_clean_and_the_numbers_agree_with_the_other_calls(chained):  # noqa: F811
    e = chained
    digest, image = e.state_digest(), e.state_export(0, 1)
    image = image[0][:image[1]].cpu().numpy().tobytes()
    (r,) = _clean(e)
    print(r)
    (st,) = e.state_stats()
    assert r["free_entries"] + r["pending_entries"] > 0  # or the case is void
    assert r["linked"] == st["overflow_entries"] > 0 and r["rows"] == digest[0]["rows"] == st["rows"]
    assert r["pool_top"] == st["pool_top"] and r["pool_cap"] == st["pool_cap"] == 4096
    assert e.state_verify() == [r]
    after = e.state_export(0, 1)
    assert e.state_digest() == digest and after[0][:after[1]].cpu().numpy().tobytes() == image  # nothing was modified
    s = recovery.verify_tables([e])
    assert s["ok"] and s["clean"] and s["tables"] == [r]


# ---------------------------------------------------------------------------------------------- 4. tatp passes, both pend sets
def test_tatp_is_clean_after_every_pass_and_refused_with_a_batch_announced():
    e = _engine(W.TATP, n_rows=2000, log_entries=1 << 16)
    e.populate(2000)
    existing = [e.dump_rows(t)[0] for t in range(5)]
    seen = {"free_entries": 0, "pending_entries": 0}
    for p in range(5):
        e.submit(_tatp_trace([e.dump_rows(t)[0] for t in range(5)], 3000, seed=40 + p))
        rep = _clean(e)
        st, dg = e.state_stats(), e.state_digest()
        for r, s, d in zip(rep, st, dg):
            assert r["rows"] == s["rows"] == d["rows"] and r["linked"] == s["overflow_entries"]
        for k in seen:
            seen[k] += sum(r[k] for r in rep)
    print(seen)
    assert seen["pending_entries"] > 0 and seen["free_entries"] > 0  # frees were pushed and a rotation made them poppable
    assert e.stats()["pool_exhausted"] == 0
    trace = _tatp_trace(existing, 3000, seed=50)
    n = len(trace) // 2
    a, b = _up(trace[:n]), _up(trace[n:2 * n])
    e.submit_device(a, n, None, 0, ahead=(b, n, None))
    out = (_lib.TableVerify * 5)()
    assert e._L.dint_state_verify(e._h, out, 5, 0, None) == ESTATE and b"announced" in e._L.dint_last_error()
    assert e._L.dint_state_verify(e._h, out, 5, RECLAIM, None) == ESTATE
    e.submit_device(b, n)
    e.sync()
    _clean(e)
    e.close()


# ---------------------------------------------------------------------------------------------- 5. the home rule against the routing
def test_smallbank_and_a_three_shard_tatp_set_have_every_row_at_home():
    sb = _engine(W.SMALLBANK, n_rows=5000, log_entries=1 << 12)
    sb.populate(5000)
    sb.submit(tracegen.sb_random(4000, seed=9, n_acct_touch=300))
    rep = _clean(sb)
    assert [r["rows"] for r in rep] == [5000, 5000] and all(r["misplaced_rows"] == 0 for r in rep)
    sb.close()
    shards = [_engine(W.TATP, n_rows=2005, log_entries=1 << 12, shard_index=s, shard_count=3) for s in range(3)]
    assert all(shards[0].hash_size(t) % 3 for t in range(5))  # bucket counts that are no multiple of 3
    for e in shards:
        e.populate(2005)  # (a shard keeps the rows that are home to it)
    per = [_clean(e) for e in shards]
    s = recovery.verify_tables(shards)
    assert s["ok"] and s["clean"] and s["engines"] == per
    for t in range(5):
        assert s["tables"][t]["rows"] == sum(p[t]["rows"] for p in per) == sum(len(e.dump_rows(t)[0]) for e in shards) > 0
        assert s["tables"][t]["misplaced_rows"] == 0 and s["tables"][t]["pool_cap"] == sum(p[t]["pool_cap"] for p in per)
        assert s["tables"][t]["linked"] == sum(p[t]["linked"] for p in per)
    assert s["tables"][0]["rows"] == 2005
    for e in shards:
        e.close()


# ---------------------------------------------------------------------------------------------- 6. after an import and a rehash
def test_import_and_rehash_leave_a_compact_pool(chained):  # noqa: F811
    src = chained
    buf, n, _ = src.state_export(0, 1)
    imp = _engine(W.STORE, n_rows=64, pool_entries=4096)
    imp.state_import(buf, n)
    reh = _engine(W.STORE, n_rows=16, pool_entries=4096)
    reh.state_rehash([src])
    for e in (imp, reh):
        (r,) = _clean(e)
        assert r["free_entries"] == r["pending_entries"] == r["unaccounted"] == 0 and r["linked"] == r["pool_top"] > 0
        assert r["rows"] == src.state_digest()[0]["rows"]
        e.close()


# ---------------------------------------------------------------------------------------------- 7. reclaim on a sound engine
def test_reclaim_on_a_sound_engine_changes_nothing_and_later_passes_answer_as_a_twin():
    def make():
        e = _engine(W.STORE, n_rows=64, pool_entries=2048)
        rng = np.random.default_rng(5)
        keys = tracegen.store_key(rng.permutation(600)[:, None], np.arange(1, 4)[None, :], 0).ravel()
        rng.shuffle(keys)
        e.load_rows(0, keys, np.arange(len(keys), dtype="<u4"), _vals(keys, 1))
        _delete_rows(e, keys[::3])
        _store_insert(e, tracegen.store_key(3_000_000 + np.arange(200), 1, 0), 2)
        return e, keys

    (e, keys), (twin, _) = make(), make()
    digest, image = e.state_digest(), e.state_export(0, 1)
    image = image[0][:image[1]].cpu().numpy().tobytes()
    (r,) = e.state_reclaim()
    assert r["reclaimed"] == 0 and r["stray_rows_cleared"] == 0 and is_clean(r) and r["free_entries"] + r["pending_entries"] > 0
    after = e.state_export(0, 1)
    assert e.state_digest() == digest == twin.state_digest() and after[0][:after[1]].cpu().numpy().tobytes() == image
    fresh = tracegen.store_key(5_000_000 + np.arange(400), 2, 0)
    answers = []
    for x in (e, twin):
        m = np.zeros(len(fresh), wire.STORE_MSG)
        m["type"], m["key"], m["val"] = wire.Store.INSERT, fresh, _vals(fresh, 7)
        ins = x.submit(m).tobytes()
        _delete_rows(x, np.concatenate([keys[1::6], fresh[::2]]))
        answers.append((ins, _store_read(x, np.concatenate([keys, fresh])).tobytes(), [d.tobytes() for d in x.dump_rows(0)]))
    assert answers[0] == answers[1] and e.state_digest() == twin.state_digest()
    assert _clean(e) == _clean(twin)
    e.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    for e in (_engine(W.FASST, n_slots=1000), _engine(W.TPL, n_slots=1000), _engine(W.LOG, log_entries=1 << 10)):
        for call in (e.state_verify, e.state_reclaim):
            with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
                call()
        e.close()
    e = _engine(W.TATP, n_rows=100)
    out = (_lib.TableVerify * 5)()
    assert e._L.dint_state_verify(e._h, out, 4, 0, None) == EINVAL and b"room for" in e._L.dint_last_error()
    assert e._L.dint_state_verify(e._h, None, 5, 0, None) == EINVAL
    assert e._L.dint_state_verify(e._h, out, 5, 2, None) == EINVAL  # an unknown flag
    assert e._L.dint_state_verify(e._h, out, 5, 0, None) == 5 and out[4].pool_cap == e.hash_size(4) // 4 + 4096
    e.close()
