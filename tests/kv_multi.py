"""Launch sets of several kv engines (dint_submit_segments_multi / _ahead): the step schedules and the segment layout (test
tooling, numpy only; tests/test_gpu_kv_multi.py runs them on the GPU, tests/test_kv_multi_host.py checks on the host that
every schedule holds what it is about).

A set is a list of tests/kv_collide.py's cached cases, one per engine and all of one workload.  Its schedule is a stagger:
engine k runs its pass j - k at step j and nothing before or after, so the first and the last steps have engines with every
segment empty beside engines with work, and the middle steps engines of very different sizes (14,000 beside 6,000 beside
500).  The geometry is the same at every step of a schedule (an announcement needs that): three segments per engine, a pass
of n requests in segment 0 (ceil(n / 2)) and segment 2 (the rest), segment 1 empty."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import kv_collide as kc
from dint_amd import wire

W = wire.Workload
N_SEG = 3
SEG_CAP = {W.STORE: 8192, W.TATP: 8192, W.SMALLBANK: 20480}
PAD = 0xCD


def _segmented(req: np.ndarray, cuts, cap, hdr=64):
    """lay `req` out as len(cuts)-1 segments of capacity `cap` with a header in front of each"""
    msg = req.dtype.itemsize
    stride = hdr + (cap * msg + 63) // 64 * 64
    nseg = len(cuts) - 1
    buf = np.full(nseg * stride, PAD, np.uint8)  # padding slots hold garbage
    for k in range(nseg):
        part = req[cuts[k]:cuts[k + 1]]
        buf[k * stride:k * stride + 4] = np.array([len(part)], "<u4").view(np.uint8)
        buf[k * stride + hdr:k * stride + hdr + len(part) * msg] = np.frombuffer(part.tobytes(), np.uint8)
    return buf, stride, nseg


def _unsegment(buf, cuts, stride, dtype, hdr=64):
    msg = dtype.itemsize
    return np.concatenate([np.frombuffer(buf[k * stride + hdr:k * stride + hdr + (cuts[k + 1] - cuts[k]) * msg].tobytes(), dtype)
                           for k in range(len(cuts) - 1)])


def padding_untouched(out, cuts, stride, msg, hdr=64) -> bool:
    """the "padding is never written" check: every byte behind a segment's live requests still holds the padding byte"""
    return all((out[k * stride + hdr + (cuts[k + 1] - cuts[k]) * msg:(k + 1) * stride] == PAD).all() for k in range(len(cuts) - 1))


def cuts_of(n: int):
    """a pass of n requests: segment 0 takes ceil(n / 2), segment 1 nothing, segment 2 the rest"""
    return [0, (n + 1) // 2, (n + 1) // 2, n]


SETS = {
    "tatp3": lambda: [kc.tatp_hot_pair(False, "cold"), kc.tatp_rem_pair(), kc.tatp_cf_pair(0.3, True)],
    "tatp4": lambda: SETS["tatp3"]() + [kc.tatp_hot_pair(True, "equal")],
    "tatp2": lambda: [SETS["tatp3"]()[0], kc.tatp_chunks()],  # seven passes beside three: one engine idles for long
    "store3": lambda: [kc.store_hot_pair("warm"), kc.store_rem_pair(), kc.store_hot_pair("cold", exists=False)],
    "store5": lambda: SETS["store3"]() + [kc.store_chunks(), kc.store_hot_pair("equal")],  # over DINT_KV_MULTI_MAX: the fallback
    "sb3": lambda: [kc.sb_hot_pair(False, "cold"), kc.sb_hot_pair(True, "warm"), kc.sb_hot_pair(False, "warm", both_rows=True)],
    "sb2": lambda: [SETS["sb3"]()[0], kc.sb_chunks()],
}
BIG = {W.STORE: 6000, W.TATP: 6000, W.SMALLBANK: 20_000}  # "a full engine" beside an idle one


@dataclass
class Schedule:
    name: str
    cases: list
    seg_cap: int
    steps: list   # steps[j][k]: the pass engine k runs at step j, or None

    @property
    def wl(self):
        return self.cases[0].wl

    @property
    def dtype(self):
        return self.cases[0].passes[0].dtype

    @property
    def stride(self):
        return 64 + (self.seg_cap * self.dtype.itemsize + 63) // 64 * 64

    def live(self, j, k) -> int:
        p = self.steps[j][k]
        return 0 if p is None else len(self.cases[k].passes[p])

    def cuts(self, j, k):
        return cuts_of(self.live(j, k))

    def buffers(self, j, k):
        """(the buffer engine k is handed at step j, the buffer it must leave): requests / the oracle's replies in the layout
        above; an idle engine's buffer is three empty segments and stays as it is"""
        p = self.steps[j][k]
        c = self.cases[k]
        empty = np.zeros(0, self.dtype)
        cuts = self.cuts(j, k)
        a = _segmented(empty if p is None else c.passes[p], cuts, self.seg_cap)[0]
        b = a if p is None else _segmented(c.want[p], cuts, self.seg_cap)[0]
        return a, b


def schedule(name: str, cases=None, seg_cap: int = 0) -> Schedule:
    cases = SETS[name]() if cases is None else cases
    assert len({c.wl for c in cases}) == 1
    n_steps = max(k + len(c.passes) for k, c in enumerate(cases))
    steps = [[j - k if 0 <= j - k < len(c.passes) else None for k, c in enumerate(cases)] for j in range(n_steps)]
    return Schedule(name, cases, seg_cap or SEG_CAP[cases[0].wl], steps)


@functools.lru_cache(None)
def cached(name: str, seg_cap: int = 0):
    """the schedule of the set `name` and its host buffers [step][engine] = (in, out), built once per process and never written"""
    s = schedule(name, seg_cap=seg_cap)
    bufs = [[s.buffers(j, k) for k in range(len(s.cases))] for j in range(len(s.steps))]
    for row in bufs:
        for a, b in row:
            a.flags.writeable = False
            b.flags.writeable = False
    return s, bufs
