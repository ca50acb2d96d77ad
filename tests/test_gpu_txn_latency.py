"""Transaction latency of the GPU-resident closed-loop clients (csrc/k_txn.hip with DINT_DRIVER_LATENCY, csrc/txn_latency.h):
the round trips against the host driver's (which tests/test_txn_latency_host.py pins to a derivation from older statistics and
to the reference clients' recordings), the request stream still bit-identical with the flag on, and the ticks of the device
clock bounded exactly by the epoch stamps the kernels leave.  No absolute time is asserted."""
import numpy as np
import pytest

import client_edges as ce
import txn_latency as tl
from dint_amd import _lib, wire
from dint_amd.driver import Driver, GpuDriver, merge_latency, tick_bin
from test_client_golden import load_block

pytestmark = pytest.mark.gpu
W = wire.Workload
TB = ce.TXG_TB           # clients per workgroup of the product's k_txn_emit
SMALL = ce.SMALL_TB      # ... and of dint_amd/libdint_txn_small.so
ROWS = {W.TATP: (3000, 0.8), W.SMALLBANK: (5000, None)}  # small tables: conflicts, so aborts as well as commits


def _shapes(tb):
    return [1, 63, 65, tb - 1, tb, tb + 1, 2 * tb + 1]


def _serve(gb, gpu, cap, xs):
    """the rest of GpuLoop.epochs(1): the three servers answer in place, the clients take the replies"""
    for s, eng in enumerate(gb.engines):
        eng.stream_wait(xs)
        eng.submit_segments(gpu.batch_ptr[s], 1, cap, cap * gb.msg, gpu.counts_ptr + 4 * s, 0)
        eng.stream_signal(xs)
    gpu.consume(xs)


def _host_epoch(host, ga, cap):
    """one epoch of the host driver behind batches of `cap` slots: what does not fit is not sent, and the client takes its own
    request (ord 0) for the answer -- what k_txn_emit does with a message that finds no room.  Returns the full batches."""
    want = host.next()
    rep = ga.submit([w[:cap] for w in want])
    full = []
    for s in range(3):
        lost = want[s][cap:].copy()
        lost["ord"] = 0
        full.append(np.concatenate([rep[s], lost]))
    host.consume(full)
    return want


def _check_ticks_cover_round_trips(lat):
    assert lat["tick_khz"] > 0
    assert lat["ticks"].sum(axis=1).tolist() == lat["round_trips"].sum(axis=1).tolist()
    assert ((lat["tick_sum"] > 0) == (lat["round_trips"].sum(axis=1) > 0)).all()
    assert (lat["tick_max"] * lat["round_trips"].sum(axis=1) >= lat["tick_sum"]).all()


def _run_pair(wl, clients, epochs, cap=None, monkeypatch=None, fuse=1, waves=None, small=False, first=11):
    """a GpuDriver with the latency flag and a host Driver side by side, each through its own three GPU shard servers; the
    streams compared epoch by epoch.  Returns (host, gpu, loop, run): run(n) goes on for n more epochs."""
    from dint_amd.replay import GpuLoop, ShardGroup

    monkeypatch.setenv("DINT_TXN_FUSE", str(fuse))
    if waves is not None:
        monkeypatch.setenv("DINT_TXN_WAVES", str(waves))
    n_rows, zipf = ROWS[wl]
    ga, gb = ShardGroup(wl, n_rows, log_entries=100_000), ShardGroup(wl, n_rows, log_entries=100_000)
    host = Driver(wl, clients, n_rows, first_client=first, zipf_theta=zipf)
    cap = cap or 4 * clients + 64
    if small:
        with ce.small_txn_build():
            gpu = GpuDriver(wl, clients, n_rows, cap, first_client=first, zipf_theta=zipf, latency=True)
    else:
        gpu = GpuDriver(wl, clients, n_rows, cap, first_client=first, zipf_theta=zipf, latency=True)
    loop = GpuLoop(gb, gpu)
    xs = loop.stream.cuda_stream

    def run(n):
        for e in range(n):
            want = _host_epoch(host, ga, cap)
            gpu.next(xs)
            loop.stream.synchronize()
            got = gpu.read_batches()
            for s in range(3):
                assert got[s].tobytes() == want[s][:cap].tobytes(), (e, s, len(got[s]), len(want[s]))
            _serve(gb, gpu, cap, xs)
        loop.sync()

    run(epochs)
    return host, gpu, loop, run


def _compare(host, gpu):
    hl, gl, hs, gs = host.latency(), gpu.latency(), host.stats(), gpu.stats()
    tl.assert_rt_equal(gl, hl)
    for k in ("txns", "committed", "by_type", "committed_by_type"):
        assert gs[k] == hs[k], k
    tl.check_against_stats(gl, gs)
    _check_ticks_cover_round_trips(gl)
    assert gl["epochs"] == hl["epochs"] == gs["epochs"]
    return gl


SHAPE_CASES = [(wl, small, n, fuse) for wl in (W.TATP, W.SMALLBANK) for small in (False, True)
               for n in _shapes(SMALL if small else TB) for fuse in (1, 0)]


@pytest.mark.parametrize("wl,small,clients,fuse", SHAPE_CASES,
                         ids=[f"{wl.name.lower()}-tb{SMALL if small else TB}-{n}-fuse{fuse}" for wl, small, n, fuse in SHAPE_CASES])
def test_round_trips_equal_the_host_drivers(wl, small, clients, fuse, monkeypatch):
    host, gpu, _, _ = _run_pair(wl, clients, 40, monkeypatch=monkeypatch, fuse=fuse, small=small)
    gl = _compare(host, gpu)
    assert gpu.stats()["overflow"] == 0 and gl["round_trips"].sum() > 0


@pytest.mark.parametrize("wl,small,clients,waves", [(W.TATP, False, TB + 1, 3), (W.SMALLBANK, False, 2 * TB + 1, 4), (W.TATP, False, 65, 5),
                                                    (W.SMALLBANK, True, SMALL + 1, 3), (W.TATP, True, 2 * SMALL + 1, 5)])
def test_round_trips_in_every_register_budget_variant(wl, small, clients, waves, monkeypatch):
    host, gpu, _, _ = _run_pair(wl, clients, 40, monkeypatch=monkeypatch, waves=waves, small=small)
    _compare(host, gpu)


@pytest.mark.parametrize("wl", ["tatp", "smallbank"])
def test_the_recorded_block_in_one_launch_gives_the_pinned_table(wl):
    """the 96 reference clients of tests/golden/clients_block.npz (first gid not at a wavefront boundary) on one GpuDriver, fed
    the recorded replies: exactly the table tests/test_txn_latency_host.py derives for the same recording"""
    import torch
    from test_gpu_lock_loop import _h2d

    Wl = W.TATP if wl == "tatp" else W.SMALLBANK
    g0, n_rows, counts, req, rep = load_block(wl)
    assert g0 % 64 != 0
    n, E = counts.shape[:2]
    off = np.concatenate([np.zeros((n, 1, 3), np.int64), np.cumsum(counts, axis=1, dtype=np.int64)], axis=1)
    cap = int(counts.sum(axis=0).max()) + 7
    gpu = GpuDriver(Wl, n, n_rows, cap, first_client=g0, latency=True)
    st = torch.cuda.Stream()
    xs = st.cuda_stream
    for e in range(E):
        gpu.next(xs)
        st.synchronize()
        for s in range(3):
            _h2d(gpu.batch_ptr[s], np.concatenate([rep[c][s][off[c, e, s]:off[c, e + 1, s]] for c in range(n)]))
        gpu.consume(xs)
    st.synchronize()
    lat, gs = gpu.latency(), gpu.stats()
    assert gs["messages"] == int(counts.sum()) and gs["overflow"] == 0
    assert tl.by_round_trips(lat) == tl.BLOCK_TABLE[wl]
    tl.check_against_stats(lat, gs)
    _check_ticks_cover_round_trips(lat)
    r = np.arange(tl.RT_BINS, dtype=np.uint64)
    assert (lat["rt_sum"] == (lat["round_trips"] * r).sum(axis=1)).all()
    assert lat["rt_max"].tolist() == [int(np.nonzero(h)[0].max()) if h.any() else 0 for h in lat["round_trips"]]


@pytest.mark.parametrize("wl,clients,fuse", [(W.TATP, 6000, 1), (W.SMALLBANK, 4000, 0)])
def test_a_full_batch_counts_the_lost_phase_as_a_round_trip(wl, clients, fuse, monkeypatch):
    """cap below an epoch's largest batch: a client whose message found no room waits the epoch all the same, on the device as
    in a host driver behind batches of the same size"""
    n_rows, zipf = ROWS[wl]
    first = Driver(wl, clients, n_rows, first_client=11, zipf_theta=zipf).next()
    cap = sorted(len(b) for b in first)[1]
    assert cap >= 2 and max(len(b) for b in first) > cap
    host, gpu, _, _ = _run_pair(wl, clients, 30, cap=cap, monkeypatch=monkeypatch, fuse=fuse)
    assert gpu.stats()["overflow"] > 0
    _compare(host, gpu)


@pytest.mark.parametrize("wl,clients", [(W.TATP, TB + 1), (W.SMALLBANK, 700)])
def test_reset_opens_a_window_and_keeps_running_transactions_whole(wl, clients, monkeypatch):
    host, gpu, loop, run = _run_pair(wl, clients, 15, monkeypatch=monkeypatch)
    before = host.latency()
    assert _compare(host, gpu)["round_trips"].sum() > 0
    gpu.latency_reset(loop.stream.cuda_stream)
    z = gpu.latency()
    assert not any(np.asarray(z[k]).any() for k in tl.RT_KEYS + tl.TICK_KEYS) and z["epochs"] == 15 and z["tick_khz"] > 0
    run(1)  # whatever finishes in this epoch began before the reset: its round trips are counted from its own beginning
    d1 = tl.minus(host.latency(), before)
    tl.assert_rt_equal(gpu.latency(), d1, "first epoch of the window", keys=tuple(d1))
    assert d1["round_trips"][:, 2:].sum() > 0
    run(9)
    lat = gpu.latency()
    tl.assert_rt_equal(lat, tl.minus(host.latency(), before), "window", keys=tuple(d1))
    _check_ticks_cover_round_trips(lat)
    assert (lat["rt_max"] <= host.latency()["rt_max"]).all()
    assert lat["rt_max"].tolist() == [int(np.nonzero(h)[0].max()) if h.any() else 0 for h in lat["round_trips"]]


def test_ticks_lie_between_the_epoch_stamps():
    """The kernel of epoch f runs between stamp[f] and stamp[f + 1] (kernels of one driver are stream-ordered), so a transaction
    of r round trips that finished in epoch f took between stamp[f - 1] - stamp[f - r] and stamp[f + 1] - stamp[f - r] ticks: per
    epoch and type, the growth of the tick histogram has the total of the round trips' growth and lies in those bins."""
    from dint_amd.replay import GpuLoop, ShardGroup

    clients, n_rows, E = 2048, 20_000, 24
    g = ShardGroup(W.TATP, n_rows, log_entries=400_000)
    gpu = GpuDriver(W.TATP, clients, n_rows, 4 * clients + 64, zipf_theta=0.8, latency=True)
    loop = GpuLoop(g, gpu)
    lats = []
    for f in range(E + 1):
        loop.epochs(1)
        lats.append(gpu.latency())
    stamps, n_ep = gpu.read_stamps()
    loop.sync()
    assert n_ep == E + 1 and (stamps[:E + 1] > 0).all() and (stamps[E + 1:] == 0).all()
    stamp = [int(x) for x in stamps[:E + 1]]
    assert all(a < b for a, b in zip(stamp, stamp[1:]))
    assert lats[-1]["tick_khz"] > 0
    grew = 0
    for f in range(1, E):
        d_rt = lats[f]["round_trips"].astype(np.int64) - lats[f - 1]["round_trips"].astype(np.int64)
        d_tk = lats[f]["ticks"].astype(np.int64) - lats[f - 1]["ticks"].astype(np.int64)
        assert d_rt.min() >= 0 and d_tk.min() >= 0
        assert d_tk.sum(axis=1).tolist() == d_rt.sum(axis=1).tolist(), f
        for t in range(8):
            rs = [int(r) for r in np.nonzero(d_rt[t])[0]]
            assert all(1 <= r <= f for r in rs), (f, t, rs)
            spans = [(tick_bin(stamp[f - 1] - stamp[f - r]), tick_bin(stamp[f + 1] - stamp[f - r])) for r in rs]
            for b in np.nonzero(d_tk[t])[0]:
                assert any(lo <= b <= hi for lo, hi in spans), (f, t, int(b), rs, spans)
            if all(spans[i][1] < spans[i + 1][0] for i in range(len(spans) - 1)):  # the spans do not touch: mass per r
                for r, (lo, hi) in zip(rs, spans):
                    assert int(d_tk[t, lo:hi + 1].sum()) == int(d_rt[t, r]), (f, t, r)
                    grew += int(d_rt[t, r])
    assert grew > clients  # the per-r check did run
    assert int(lats[E - 1]["tick_max"].max()) <= stamp[E] - stamp[0]  # (the kernel of epoch E - 1 ended before the last stamp)
    _check_ticks_cover_round_trips(lats[-1])


@pytest.mark.parametrize("wl,clients", [(W.TATP, 1500), (W.SMALLBANK, 1000)])
def test_two_client_groups_merge_to_the_host_run(wl, clients):
    from dint_amd.replay import GpuLoop, ShardGroup

    n_rows, zipf = ROWS[wl]
    epochs, cap = 40, 4 * clients + 64
    a, b = ShardGroup(wl, n_rows, log_entries=400_000), ShardGroup(wl, n_rows, log_entries=400_000)
    hosts = [Driver(wl, clients, n_rows, first_client=k * clients, zipf_theta=zipf) for k in range(2)]
    for _ in range(epochs):
        for h in hosts:
            h.consume(a.submit(h.next()))
    gpus = [GpuDriver(wl, clients, n_rows, cap, first_client=k * clients, zipf_theta=zipf, latency=True) for k in range(2)]
    loop = GpuLoop(b, gpus)
    loop.epochs(epochs)
    loop.sync()
    for h, g in zip(hosts, gpus):
        tl.assert_rt_equal(g.latency(), h.latency())
    merged = merge_latency([g.latency() for g in gpus])
    tl.assert_rt_equal(merged, merge_latency([h.latency() for h in hosts]))
    _check_ticks_cover_round_trips(merged)
    assert merged["round_trips"].sum() == sum(g.stats()["committed"] for g in gpus) > 0


def test_flags():
    """without DINT_DRIVER_LATENCY the three latency calls are DINT_ESTATE (-5) and the driver runs as before; a flag bit that
    no flag names is DINT_EINVAL"""
    gpu = GpuDriver(W.TATP, 65, 1000, 512)
    gpu.next(0)
    for call in (gpu.latency, gpu.latency_reset, gpu.read_stamps):
        with pytest.raises(_lib.DintError, match="-5"):
            call()
    assert gpu.stats()["messages"] > 0
    for flags in (2, 1 | 8, 1 << 31):
        with pytest.raises(_lib.DintError, match="-1"):
            GpuDriver(W.TATP, 65, 1000, 512, flags=flags)
    on = GpuDriver(W.TATP, 65, 1000, 512, latency=True)
    on.next(0)
    st, n = on.read_stamps()
    assert n == 1 and st[0] > 0 and not st[1:].any()
