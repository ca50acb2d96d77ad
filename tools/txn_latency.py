#!/usr/bin/env python3
"""Committed-transaction latency of the closed loop that never leaves the GPU: what the reference's clients print at the end of
a run (CollectStat, tatp/caladan/client_udp_shard.cc:94-107, :1148-1182) -- throughput, goodput, average / median / 99th / 99.9th
percentile latency of committed transactions -- from GPU-resident clients (dint_amd.driver.GpuDriver with latency=True) and the
three shard servers of a dint_amd.replay.GpuLoop.  Latency in microseconds of the device clock (a percentile is the lower bound
of its histogram bin, at most 12.5 % below the sample) and in round trips, per transaction type and overall; the histograms are
reset after the warm-up epochs (the reference's stat_started window).

  tools/txn_latency.py                                   tatp, 524,288 clients, 1M subscribers, Zipf 0.8
  tools/txn_latency.py --sweep 4096,16384,65536,262144   latency against throughput over client counts
  tools/txn_latency.py --no-latency                      the same loop without the flag (the rate the flag costs against)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dint_amd import wire  # noqa: E402
from dint_amd.driver import GpuDriver, latency_percentiles, merge_latency  # noqa: E402
from dint_amd.replay import GpuLoop, ShardGroup  # noqa: E402

TXN_NAMES = {
    "tatp": ["get_subscriber", "get_new_destination", "get_access", "update_subscriber", "update_location", "insert_call_fwd", "delete_call_fwd"],
    "smallbank": ["amalgamate", "balance", "deposit_checking", "send_payment", "transact_saving", "write_check"],
}
PS = (50, 99, 99.9)


def run(grp, wl, clients, n_rows, zipf, groups, warmup, epochs, latency=True):
    """one closed loop: `warmup` epochs, the histograms reset, `epochs` timed epochs.  Returns a dict of the figures."""
    per = clients // groups
    cap = min(min(e.pass_max for e in grp.engines), int(0.75 * per) + 4096)
    gds = [GpuDriver(wl, per, n_rows, cap, first_client=g * per, zipf_theta=zipf, latency=latency) for g in range(groups)]
    loop = GpuLoop(grp, gds)
    loop.epochs(warmup)
    if latency:
        for g, st in zip(gds, loop.streams):
            g.latency_reset(st.cuda_stream)
    loop.sync()
    s0 = [g.stats() for g in gds]
    t0 = time.perf_counter()
    loop.epochs(epochs)
    loop.sync()
    dt = time.perf_counter() - t0
    s1 = [g.stats() for g in gds]
    txns = sum(b["txns"] - a["txns"] for a, b in zip(s0, s1))
    committed = sum(b["committed"] - a["committed"] for a, b in zip(s0, s1))
    out = {"clients": per * groups, "groups": groups, "epochs": epochs, "us_per_epoch": dt / epochs * 1e6,
           "throughput_Mtxn_s": txns / dt / 1e6, "goodput_Mtxn_s": committed / dt / 1e6,
           "overflow": sum(s["overflow"] for s in s1), "latency": latency}
    if latency:
        lat = merge_latency([g.latency() for g in gds])
        out["tick_khz"] = lat["tick_khz"]
        out["aborted"] = int(lat["aborted_round_trips"].sum())
        names = TXN_NAMES["tatp" if wl == wire.Workload.TATP else "smallbank"]
        rows = {"all": None, **{n: [t] for t, n in enumerate(names)}}
        out["rows"] = {name: {"us": latency_percentiles(lat, "ticks", PS, types), "round_trips": latency_percentiles(lat, "round_trips", PS, types)}
                       for name, types in rows.items()}
        # the window holds every transaction that committed in it, whenever it began
        assert out["rows"]["all"]["us"]["n"] == out["rows"]["all"]["round_trips"]["n"] == committed, (out["rows"]["all"], committed)
    del loop, gds
    return out


def _f(v, spec):
    return "-" if v is None else format(v, spec)


def report(r):
    print(f"clients {r['clients']} ({r['groups']} group{'s' * (r['groups'] > 1)}), {r['epochs']} epochs of {r['us_per_epoch']:.1f} us: "
          f"throughput {r['throughput_Mtxn_s']:.2f} Mtxn/s, goodput {r['goodput_Mtxn_s']:.2f} Mtxn/s, overflow {r['overflow']}"
          + ("" if r["latency"] else "  (latency off)"))
    if not r["latency"]:
        return
    print(f"latency of committed transactions (device clock {r['tick_khz'] / 1000:.0f} MHz; {r['aborted']} aborted ones are not sampled)")
    print(f"  {'transaction':<20}{'committed':>11}{'avg us':>10}{'p50 us':>10}{'p99 us':>10}{'p99.9 us':>10}{'max us':>10}   "
          f"{'avg rt':>7}{'p50':>5}{'p99':>5}{'p99.9':>6}{'max':>5}")
    for name, row in r["rows"].items():
        u, t = row["us"], row["round_trips"]
        print(f"  {name:<20}{u['n']:>11}{_f(u['avg'], '10.1f')}{_f(u['p'][50], '10.1f')}{_f(u['p'][99], '10.1f')}{_f(u['p'][99.9], '10.1f')}"
              f"{_f(u['max'], '10.1f')}   {_f(t['avg'], '7.2f')}{_f(t['p'][50], '5')}{_f(t['p'][99], '5')}{_f(t['p'][99.9], '6')}{_f(t['max'], '5')}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["tatp", "smallbank"], default="tatp")
    ap.add_argument("--clients", type=int, default=524288)
    ap.add_argument("--rows", type=int, default=1_000_000, help="subscribers / accounts")
    ap.add_argument("--zipf", type=float, default=0.8, help="Zipf theta of the keys; 0 = the reference's own distribution")
    ap.add_argument("--groups", type=int, default=1, help="client groups that take turns at the servers")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=1, help="runs per client count, each from fresh clients and freshly populated servers")
    ap.add_argument("--sweep", default="", help="comma-separated client counts: the latency-against-throughput table")
    ap.add_argument("--no-latency", action="store_true", help="drivers without DINT_DRIVER_LATENCY: the loop's rate alone")
    ap.add_argument("--json", action="store_true", help="one JSON line per run as well")
    a = ap.parse_args()
    wl = wire.Workload.TATP if a.workload == "tatp" else wire.Workload.SMALLBANK
    counts = [int(x) for x in a.sweep.split(",") if x] or [a.clients]
    grp = ShardGroup(wl, a.rows, log_entries=8_000_000)
    grp.snapshot()
    table = []
    for c in counts:
        for k in range(a.repeats):
            grp.restore()
            r = run(grp, wl, c, a.rows, a.zipf or None, a.groups, a.warmup, a.epochs, latency=not a.no_latency)
            report(r)
            if a.json:
                print(json.dumps(r))
            table.append(r)
    if len(table) > 1:
        print(f"\n{'clients':>9}{'Mtxn/s':>9}{'good':>8}{'us/epoch':>10}" + ("" if a.no_latency else f"{'avg us':>9}{'p50 us':>9}{'p99 us':>9}{'p99.9 us':>10}{'avg rt':>8}"))
        for r in table:
            line = f"{r['clients']:>9}{r['throughput_Mtxn_s']:>9.2f}{r['goodput_Mtxn_s']:>8.2f}{r['us_per_epoch']:>10.1f}"
            if r["latency"]:
                u, t = r["rows"]["all"]["us"], r["rows"]["all"]["round_trips"]
                line += f"{_f(u['avg'], '9.1f')}{_f(u['p'][50], '9.1f')}{_f(u['p'][99], '9.1f')}{_f(u['p'][99.9], '10.1f')}{_f(t['avg'], '8.2f')}"
            print(line)


if __name__ == "__main__":
    main()
