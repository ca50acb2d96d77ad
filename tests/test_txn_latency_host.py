"""Transaction latency of the closed-loop clients on the host (include/dint_driver.h struct dint_driver_latency): the round
trips the host driver reports against a derivation from the statistics it always had (tests/txn_latency.py), pinned to the
recordings of the reference's own clients; the tick bin rule against a numpy restatement; the percentile rule against sorted
samples; the round-trip count's saturation in a stand-alone program under the sanitizers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import txn_latency as tl
from dint_amd import _lib, wire
from dint_amd import driver as drv
from dint_amd.driver import Driver, latency_percentiles, merge_latency
from oracle import oracle as orc
from test_client_golden import load_block

_EINVAL = -1  # DINT_EINVAL (include/dint_abi.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
W = wire.Workload


def _wl(wl):
    return W.TATP if wl == "tatp" else W.SMALLBANK


def _check_one_client(d, der, what):
    lat, st = d.latency(), d.stats()
    tl.assert_rt_equal(lat, der.table, what)
    tl.check_against_stats(lat, st)
    assert lat["epochs"] == st["epochs"] and lat["tick_khz"] == 0
    assert not any(np.asarray(lat[k]).any() for k in tl.TICK_KEYS), what
    assert der.max_per_epoch == 1, what  # no client finishes more than one transaction per epoch


@pytest.mark.parametrize("wl", ["tatp", "smallbank"])
def test_round_trips_of_the_recorded_block_are_the_derived_table(wl):
    """every client of tests/golden/clients_block.npz on a one-client driver, fed the recorded replies: latency() equals the
    table derived from the stats() deltas, client by client and type by type, and the block's sum is the pinned table"""
    g0, n_rows, counts, req, rep = load_block(wl)
    tables = []
    for c in range(len(counts)):
        d, der, cur = Driver(_wl(wl), 1, n_rows, first_client=g0 + c), tl.Deriver(), [0, 0, 0]
        for e in range(counts.shape[1]):
            out = d.next()
            der.step(d.stats())
            assert [len(o) for o in out] == counts[c, e].tolist()
            d.consume([rep[c][s][cur[s]:cur[s] + len(out[s])].copy() for s in range(3)])
            for s in range(3):
                cur[s] += len(out[s])
        _check_one_client(d, der, (wl, g0 + c))
        tables.append(d.latency())
    whole = tl.total(tables)
    assert tl.by_round_trips(whole) == tl.BLOCK_TABLE[wl]
    meta = json.loads(str(np.load(os.path.join(G, "clients_block.npz"))["meta"]))
    if "committed" in meta and wl in meta["committed"]:
        assert int(whole["round_trips"].sum()) == meta["committed"][wl]
    # rt_sum and rt_max follow from the table
    r = np.arange(tl.RT_BINS, dtype=np.uint64)
    assert (whole["rt_sum"] == (whole["round_trips"] * r).sum(axis=1)).all()
    assert whole["rt_max"].tolist() == [int(np.nonzero(h)[0].max()) if h.any() else 0 for h in whole["round_trips"]]


@pytest.mark.parametrize("wl", ["tatp", "smallbank"])
def test_round_trips_of_the_recorded_single_clients_are_the_derived_table(wl):
    z = np.load(os.path.join(G, "clients.npz"))
    meta = json.loads(str(z["meta"]))
    dt = wire.MSG_DTYPE[_wl(wl)]
    for gid in meta["clients"][wl]:
        req = [np.frombuffer(z[f"{wl}_{gid}_s{s}_req"].tobytes(), dt) for s in range(3)]
        rep = [np.frombuffer(z[f"{wl}_{gid}_s{s}_rep"].tobytes(), dt) for s in range(3)]
        d, der, cur = Driver(_wl(wl), 1, meta["n_rows"][wl], first_client=gid), tl.Deriver(), [0, 0, 0]
        while True:
            out = d.next()
            der.step(d.stats())
            if any(cur[s] + len(out[s]) > len(req[s]) for s in range(3)):
                break  # the recording was cut inside this phase
            d.consume([rep[s][cur[s]:cur[s] + len(out[s])].copy() for s in range(3)])
            for s in range(3):
                cur[s] += len(out[s])
        _check_one_client(d, der, (wl, gid))
        lat = d.latency()
        assert lat["round_trips"].sum() > 0 and lat["aborted_round_trips"].sum() > 0


def _oracles(wl, n_rows):
    cls = orc.TatpOracle if wl == W.TATP else orc.SmallbankOracle
    return [cls(n_rows, log_entries=100_000) for _ in range(3)]


@pytest.mark.parametrize("wl,n_rows,zipf", [(W.TATP, 2000, 0.8), (W.SMALLBANK, 3000, None)])
def test_a_driver_of_many_clients_sums_its_clients(wl, n_rows, zipf):
    """96 clients in one driver against three CPU oracle shards: its latency is the sum of the per-client derivations (96
    one-client drivers in lock step, each handed its own replies), and two halves merged are the whole"""
    n, epochs = 96, 60
    big, halves = Driver(wl, n, n_rows, zipf_theta=zipf), [Driver(wl, 48, n_rows, first_client=k * 48, zipf_theta=zipf) for k in range(2)]
    ones = tl.LockstepSingles(wl, n, n_rows, zipf_theta=zipf)
    ora = _oracles(wl, n_rows)
    for e in range(epochs):
        req, want = big.next(), ones.next()
        hreq = [h.next() for h in halves]
        for s in range(3):
            assert req[s].tobytes() == want[s].tobytes(), (e, s)
            assert np.concatenate([hreq[0][s], hreq[1][s]]).tobytes() == req[s].tobytes(), (e, s)
        rep = [ora[s].replay(req[s]) if len(req[s]) else req[s] for s in range(3)]
        big.consume(rep)
        ones.consume(rep)
        halves[0].consume([rep[s][:len(hreq[0][s])].copy() for s in range(3)])
        halves[1].consume([rep[s][len(hreq[0][s]):].copy() for s in range(3)])
    lat, st = big.latency(), big.stats()
    tl.assert_rt_equal(lat, ones.table(), "whole")
    tl.check_against_stats(lat, st)
    assert lat["round_trips"].sum() > 100 and lat["aborted_round_trips"].sum() > 0
    hl = [h.latency() for h in halves]
    tl.assert_rt_equal(hl[0], ones.table(0, 48), "first half")
    tl.assert_rt_equal(hl[1], ones.table(48, 96), "second half")
    merged = merge_latency(hl)
    tl.assert_rt_equal(merged, lat, "merged")
    assert merged["epochs"] == epochs and merged["tick_khz"] == 0


# ------------------------------------------------------------------------------------------------------------ the bin rule
def _np_bin(v):
    """log-linear: below 16 the value; above, 8 bins per power of two; the last bin saturates"""
    v = int(v)
    if v < 16:
        return v
    e = v.bit_length() - 1
    return min(16 + (e - 4) * 8 + ((v >> (e - 3)) & 7), tl.TICK_BINS - 1)


def _np_lo(b):
    if b < 16:
        return b
    e, sub = 4 + (b - 16) // 8, (b - 16) % 8
    return (8 + sub) << (e - 3)


def test_tick_bin_rule():
    assert drv.LAT_TICK_BINS == tl.TICK_BINS and drv.LAT_RT_BINS == tl.RT_BINS
    sat = _np_lo(tl.TICK_BINS - 1)  # the first value of the saturating bin
    vals = [0, 15, 16, 17, 1 << 63, (1 << 64) - 1, sat - 1, sat, sat + 1]
    k = 0
    while (1 << k) <= 2 * sat:
        vals += [(1 << k) - 1, 1 << k, (1 << k) + 1]
        k += 1
    vals += [_np_lo(b) for b in range(tl.TICK_BINS)] + [_np_lo(b) - 1 for b in range(1, tl.TICK_BINS + 1)]
    vals = sorted(set(vals))
    bins = [drv.tick_bin(v) for v in vals]
    assert bins == [_np_bin(v) for v in vals]
    assert all(a <= b for a, b in zip(bins, bins[1:])) and bins[0] == 0 and bins[-1] == tl.TICK_BINS - 1  # monotone
    assert drv.tick_bin(1 << 63) == tl.TICK_BINS - 1
    assert [drv.tick_bin_lo(b) for b in range(tl.TICK_BINS + 1)] == [_np_lo(b) for b in range(tl.TICK_BINS + 1)]
    for v, b in zip(vals, bins):
        assert drv.tick_bin_lo(b) <= v
        if b < tl.TICK_BINS - 1:  # below saturation
            assert v < drv.tick_bin_lo(b + 1), (v, b)
    for b in range(16, tl.TICK_BINS - 1):  # a bin is at most 12.5 % wide
        lo, hi = drv.tick_bin_lo(b), drv.tick_bin_lo(b + 1)
        assert (hi - lo) * 8 <= lo
    assert drv.tick_bin_lo(tl.TICK_BINS) >= 100_000_000 * 10  # ten seconds and more at 100 MHz


# ------------------------------------------------------------------------------------------------------------ percentiles
def _lat_from_samples(samples_by_type, khz=100_000):
    """a latency dict whose tick histogram holds the given samples (ticks), per type"""
    lat = {"ticks": np.zeros((8, tl.TICK_BINS), np.uint64), "tick_sum": np.zeros(8, np.uint64), "tick_max": np.zeros(8, np.uint64),
           "tick_khz": khz, "epochs": 0, **tl.empty()}
    for t, xs in samples_by_type.items():
        for x in xs:
            lat["ticks"][t, _np_bin(x)] += 1
            lat["tick_sum"][t] += x
            lat["tick_max"][t] = max(int(lat["tick_max"][t]), x)
    return lat


def _sorted_rule(samples, p):
    return int(np.sort(np.asarray(samples, dtype=np.uint64))[min(int(p * len(samples) / 100), len(samples) - 1)])


@pytest.mark.parametrize("name", ["one", "thousand", "last-bin", "two-types"])
def test_percentiles_follow_the_sorted_samples(name):
    rng = np.random.default_rng(7)
    if name == "one":
        by_type = {3: [777]}
    elif name == "thousand":  # p = 99.9 of n = 1000: index 999, the largest sample, alone in its bin
        by_type = {0: list(rng.integers(100, 5000, 999)) + [1_000_000]}
    elif name == "last-bin":
        by_type = {1: [1 << 40] * 5, 2: [1 << 50] * 3}
    else:
        by_type = {0: list(rng.integers(16, 100_000, 400)), 4: list(rng.integers(0, 40, 37))}
    by_type = {t: [int(x) for x in xs] for t, xs in by_type.items()}
    lat = _lat_from_samples(by_type)
    ps = (0, 50, 99, 99.9, 100)
    for types in [None] + [[t] for t in by_type]:
        samples = [x for t, xs in by_type.items() if types is None or t in types for x in xs]
        got = latency_percentiles(lat, "ticks", ps=ps, types=types)
        assert got["n"] == len(samples)
        for p in ps:
            want_bin = _np_bin(_sorted_rule(samples, p))  # the bin of the sample the reference's rule picks
            assert got["p"][p] == pytest.approx(_np_lo(want_bin) / 100.0), (name, types, p)  # its lower bound, in us at 100 MHz
        assert got["avg"] == pytest.approx(sum(samples) / len(samples) / 100.0)
        assert got["max"] == pytest.approx(max(samples) / 100.0)
    if name == "thousand":
        assert latency_percentiles(lat, "ticks", ps=(99.9,))["p"][99.9] == _np_lo(_np_bin(1_000_000)) / 100.0
    # round trips: the bin is the value
    rt = tl.empty()
    rs = [int(x) for x in rng.integers(1, 9, 1000)]
    for r in rs:
        tl.add(rt, 2, True, r)
    tl.add(rt, 2, False, 30)  # aborted transactions are not sampled
    rt.update(tick_khz=0, epochs=0)
    got = latency_percentiles(rt, "round_trips", ps=ps)
    assert got["n"] == 1000 and got["avg"] == pytest.approx(sum(rs) / 1000) and got["max"] == max(rs)
    assert [got["p"][p] for p in ps] == [_sorted_rule(rs, p) for p in ps]
    assert latency_percentiles(rt, "round_trips", types=[5]) == {"n": 0, "avg": None, "max": None, "p": {50: None, 99: None, 99.9: None}}
    with pytest.raises(ValueError):
        latency_percentiles(rt, "ticks")  # a host driver keeps no ticks


# ---------------------------------------------------------------------------------------------------------------- flags
def test_unknown_driver_flags_are_refused():
    L = drv._bind()
    for flags, rc in [(0, 0), (drv.DRIVER_LATENCY, 0), (2, -1), (drv.DRIVER_LATENCY | 4, -1), (1 << 31, -1)]:
        cfg = drv.DriverConfig(workload=int(W.TATP), n_clients=4, n_rows=100, flags=flags)
        h = C.c_void_p()
        got = L.dint_driver_create(C.byref(cfg), C.byref(h))
        assert (got == 0) == (rc == 0) and (got == 0 or got == _EINVAL), (flags, got)
        if got == 0:
            L.dint_driver_destroy(h)
    assert C.sizeof(drv.DriverConfig) == 64 and drv.DriverConfig.flags.offset == 32  # reserved[0] of the layout before
    assert C.sizeof(drv.DriverLatency) == 8 * (2 * 8 * 32 + 16 + 8 * 240 + 16 + 2)


# ------------------------------------------------------------------------------------------------------------- saturation
def test_round_trip_count_saturates_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/native/txn_latency_main.cc with the host code of txn_driver.cc and txn_latency.h under AddressSanitizer and UBSan: a
    client whose round-trip byte stands at 254 goes through more phases; its transaction lands in bin 31 with rt_max 255, and
    the next one counts from zero.  Nothing of it is loaded into python"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "txn_latency_main")
    # host code only: the sanitizers go to the host side of the compile (-Xarch_host), as tests/test_state_locks_host.py does
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "txn_latency_main.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
