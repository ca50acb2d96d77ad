"""GPU parity of k_log_append (dint_amd/csrc/k_log.hip) at its tile and pass edges: the last pass the 256-request tile
takes and the first of the 1024-request tile, 1024 full big tiles, a ring that a pass fills exactly, a tail that wraps
inside a tile, a submit of two passes that uses both tile sizes and both sets of tile counts.  Every case compares the
reply bytes, ALL ring bytes, the tail, the bad-request counter and the number of passes with the CPU oracle
(log_server/udp/server.cc:73-88) -- the ring is the kernel's real output: a reply is the request with one byte patched
and says nothing about where the record went.  The drain of a log engine (dint_log_drain / dint_log_drain_device) is held
to a numpy restatement built from the requests alone.  Integer work: byte for byte."""
import functools

import numpy as np
import pytest

import tracegen
from dint_amd import wire
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
W = wire.Workload

# dint_amd/csrc/k_log.hip: LOG_TB_SMALL, LOG_TB_BIG, LOG_SMALL_MAX = LOG_TB_SMALL * 1024; engine.hip: DINT_KV_PASS
TB_SMALL, TB_BIG = 256, 1024
SMALL_MAX = TB_SMALL * 1024   # 262,144: the largest pass of 256-request tiles (1024 of them)
PASS_MAX = 1 << 20            # a log engine's largest pass is min(PASS_MAX, ring entries)

PATTERNS = ["every17th", "empty_big_tiles", "lane63", "lane0", "none_valid"]


def _engine(*a, **k):
    from dint_amd.engine import Engine

    return Engine(*a, **k)


def _up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _commits(n, seed):
    """n COMMIT requests, all valid; shared between the cases (read-only)"""
    m = tracegen.log_random(n, seed=seed)
    m.setflags(write=False)
    return m


def _requests(n, seed, pattern):
    m = _commits(n, seed).copy()
    i = np.arange(n)
    if pattern == "every17th":          # the pattern of test_log_vs_oracle_with_wrap
        m["type"][3::17] = 5
    elif pattern == "empty_big_tiles":  # two whole 1024-request tiles (eight of 256) without a record, in the middle of the look-back
        m["type"][3 * TB_BIG:5 * TB_BIG] = 5
    elif pattern == "lane63":           # one record per wave, from its last lane
        m["type"][i % 64 != 63] = 5
    elif pattern == "lane0":            # ... from its first lane
        m["type"][i % 64 != 0] = 5
    elif pattern == "none_valid":
        m["type"][:] = 5
    else:
        raise ValueError(pattern)
    return m


def _passes(n, cap):
    return -(-n // min(PASS_MAX, cap))


def _check(eng, o, cap, n_batches):
    """ring (every byte), tail, the bad-request counter and the number of passes against the oracle"""
    ring, tail = eng.read_log(cap)
    assert tail == o.tail
    got = np.frombuffer(ring.tobytes(), "u1").reshape(cap, 64)
    same = (got == o.ring).all(axis=1)
    assert same.all(), (int((~same).sum()), np.nonzero(~same)[0][:8])
    st = eng.stats()
    assert st["bad_requests"] == o.errors
    assert st["batches"] == n_batches
    assert st["missing_keys"] == 0 and st["pool_exhausted"] == 0


def _run_host(cap, submits, pattern):
    """`submits` = request counts, one Engine.submit each on ONE engine; returns (engine, oracle, request arrays)"""
    eng, o = _engine(W.LOG, log_entries=cap), orc.LogOracle(cap)
    assert eng.pass_max == min(PASS_MAX, cap)
    reqs, batches = [], 0
    for k, n in enumerate(submits):
        req = _requests(n, 11 + k, pattern)
        got, want = eng.submit(req), o.replay(req)
        assert got.tobytes() == want.tobytes(), k
        batches += _passes(n, cap)
        reqs.append(req)
    _check(eng, o, cap, batches)
    return eng, o, reqs


# ---------------------------------------------------------------- the two tile sizes at their border
def test_last_pass_of_the_small_tile():
    """n = 262,144: 1024 tiles of 256, the look-back of the last one reads the maximum of 1023 counts"""
    _run_host(300_007, [SMALL_MAX], "every17th")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_first_pass_of_the_big_tile(pattern):
    """n = 262,145: 257 tiles of 1024 (16 waves each), the last one holds ONE request"""
    _, o, _ = _run_host(300_007, [SMALL_MAX + 1], pattern)
    if pattern == "none_valid":
        assert o.tail == 0 and not o.ring.any() and o.errors == SMALL_MAX + 1
    if pattern == "lane63":
        assert o.tail == (SMALL_MAX + 1) // 64


@pytest.mark.parametrize("pattern", PATTERNS)
def test_1024_full_big_tiles_then_a_tail_that_wraps_inside_a_tile(pattern):
    """n = 2^20 (1024 full tiles of 1024: every count word, the longest look-back), then 300,000 more on the same engine:
    they start at the tail the first pass left and run over the end of the ring in the middle of a tile"""
    cap = PASS_MAX + 7
    _, o, _ = _run_host(cap, [PASS_MAX, 300_000], pattern)
    if pattern == "every17th":
        assert o.tail == 220_665  # 986,895 + 282,353 records mod 1,048,583
    if pattern == "none_valid":  # nothing appended: the replies are the requests
        assert o.tail == 0 and not o.ring.any() and o.errors == PASS_MAX + 300_000


def test_a_pass_that_fills_the_ring_exactly():
    """ring = pass = 2^20 valid requests, twice: the tail comes back to where it was, every slot is overwritten"""
    cap = PASS_MAX
    eng, o = _engine(W.LOG, log_entries=cap), orc.LogOracle(cap)
    for k in range(2):
        req = _commits(PASS_MAX, 11 + k)
        assert eng.submit(req).tobytes() == o.replay(req).tobytes(), k
        assert eng.read_log(0)[1] == 0 == o.tail
    _check(eng, o, cap, 2)
    assert (o.ring[:, :8] == np.frombuffer(_commits(PASS_MAX, 12)["key"].tobytes(), "u1").reshape(-1, 8)).all()


def test_one_submit_of_a_big_tile_pass_and_a_small_tile_pass():
    """n = 600,000 into a ring of 500,001: a pass of 500,001 (big tiles) and one of 99,999 (small tiles) in ONE submit --
    the two specialisations take turns on the two sets of tile counts, the second pass wraps the ring"""
    _run_host(500_001, [600_000], "every17th")


# ---------------------------------------------------------------- device buffers: in place and into a reply tensor
@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "separate"])
@pytest.mark.parametrize("n,cap", [(SMALL_MAX + 1, 300_007), (600_000, 500_001)])
def test_submit_device_big_tiles(n, cap, inplace):
    """the same two shapes through dint_submit_device.  600,000 / 500,001: the second pass starts 500,001 x 53 bytes into
    the arrays, an odd address -- its tiles come in and leave byte by byte"""
    import torch

    req = _requests(n, 11, "every17th")
    eng, o = _engine(W.LOG, log_entries=cap), orc.LogOracle(cap)
    want = o.replay(req)
    d = _up(req)
    out = d if inplace else torch.full_like(d, 0xEE)
    assert d.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    eng.submit_device(d, n, None if inplace else out)
    eng.sync()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    if not inplace:
        assert d.cpu().numpy().tobytes() == req.tobytes()  # the requests are untouched
    _check(eng, o, cap, _passes(n, cap))


# ---------------------------------------------------------------- the drain of a log engine
def _records(*reqs):
    """the canonical 64-byte records of the valid requests, in request order -- from the requests alone (not the oracle):
    key | val[40] | ver | 12 zero bytes"""
    out = []
    for m in reqs:
        v = m[m["type"] == wire.Log.COMMIT]
        r = np.zeros(len(v), wire.LOG_REC)
        r["key"], r["val"], r["ver"] = v["key"], v["val"], v["ver"]
        out.append(r)
    return np.concatenate(out)


def test_drain_after_a_big_pass_host_and_device_share_one_cursor():
    import torch

    cap, n = 300_007, SMALL_MAX + 1
    eng, o, (req,) = _run_host(cap, [n], "every17th")
    want = _records(req)
    assert len(want) == o.tail  # (no wrap yet)
    head, lost = eng.log_drain(1000)  # a buffer smaller than what is pending: the oldest 1000, the rest stays
    assert lost == 0 and head.tobytes() == want[:1000].tobytes()
    buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    k, lost = eng.log_drain_device(buf, cap)
    assert (k, lost) == (len(want) - 1000, 0)
    assert buf[:k * 64].cpu().numpy().tobytes() == want[1000:].tobytes()
    rest, lost = eng.log_drain()
    assert len(rest) == 0 and lost == 0
    assert eng.log_drain_device(buf, cap) == (0, 0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_drain_after_the_ring_lapped_the_reader(device):
    """ring 300,007; drain; two passes of 262,145 (493,448 records) without a drain: the ring holds the newest 300,007,
    `lost` is the rest (include/dint_abi.h: records the ring overwrote before they were drained) -- as
    test_gpu_log_replay.py pins it for tatp: n == ring entries, n + lost == records since the previous drain"""
    import torch

    cap, n = 300_007, SMALL_MAX + 1
    eng, o = _engine(W.LOG, log_entries=cap), orc.LogOracle(cap)
    first = _requests(1000, 5, "every17th")
    assert eng.submit(first).tobytes() == o.replay(first).tobytes()
    rec, lost = eng.log_drain()
    assert lost == 0 and rec.tobytes() == _records(first).tobytes()
    reqs = [_requests(n, 11 + k, "every17th") for k in range(2)]
    for r in reqs:
        assert eng.submit(r).tobytes() == o.replay(r).tobytes()
    want = _records(*reqs)
    assert len(want) > cap
    if device:
        buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
        k, lost = eng.log_drain_device(buf, cap)
        got = buf[:k * 64].cpu().numpy().tobytes()
    else:
        rec, lost = eng.log_drain()
        k, got = len(rec), rec.tobytes()
    assert k == cap and k + lost == len(want)
    assert got == want[-cap:].tobytes()  # the newest of them, oldest first
    rest, lost = eng.log_drain()
    assert len(rest) == 0 and lost == 0
    _check(eng, o, cap, 3)


def test_reset_rewinds_ring_tail_and_drain_cursor():
    cap, n = 300_007, SMALL_MAX + 1
    eng, _, _ = _run_host(cap, [n], "lane63")
    eng.log_drain(100)  # the cursor stands inside the log
    eng.reset()
    ring, tail = eng.read_log(cap)
    assert tail == 0 and not np.frombuffer(ring.tobytes(), "u1").any()
    assert eng.stats()["batches"] == 0 and eng.stats()["bad_requests"] == 0
    req = _requests(n, 21, "every17th")
    o = orc.LogOracle(cap)
    assert eng.submit(req).tobytes() == o.replay(req).tobytes()
    _check(eng, o, cap, 1)
    rec, lost = eng.log_drain()
    assert lost == 0 and rec.tobytes() == _records(req).tobytes()
