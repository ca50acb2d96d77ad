"""The log ring's tail words, appended count and drain cursor under announced, kept and cancelled batches and drains
(dint_amd/csrc/log_ring.h through dint_log_ring_host, include/dint_driver.h) against a plain model: the log is a Python list of
record ids, a cancel pops the cancelled batch's records off its end, a drain hands out the slice behind the cursor.  The model
has no ring, no modulus and no second tail word; the engine (engine.hip: ahead_cancel, log_drain_locked) and the partition stage
(k_kv_dev.h) call the log_ring.h functions the host form walks.  tests/test_gpu_ahead_cancel.py holds the engine itself to the
oracle over the same cases.

The contract (include/dint_abi.h, dint_submit_device_ahead): after a cancelled announcement tail, appended count and cursor are
as if the batch had never been seen; records drained between announcement and cancel were the caller's to discard, and the
stream goes on with the first record appended after the cancel -- nothing lost, nothing repeated."""
import itertools

import numpy as np
import pytest

from dint_amd import _lib

PASS, ANNOUNCE, KEEP, CANCEL, DRAIN = range(5)
EINVAL = -1


def _walk(cap, ops):
    L = _lib.load()
    a = np.ascontiguousarray(np.array(ops, np.uint32).reshape(-1, 2))
    out = np.zeros(6 * len(a) + sum(min(int(x), cap) for c, x in ops if c == DRAIN) + 8, np.uint64)
    w = L.dint_log_ring_host(cap, a.ctypes.data, len(a), out.ctypes.data, len(out))
    assert w >= 0, L.dint_last_error()
    res, at = [], 0
    for c, _ in ops:
        tail, appended, drained, other = (int(x) for x in out[at:at + 4])
        at += 4
        got = None
        if c == DRAIN:
            n, lost = int(out[at]), int(out[at + 1])
            got = ([int(x) for x in out[at + 2:at + 2 + n]], lost)
            at += 2 + n
        res.append((tail, appended, drained, other, got))
    assert at == w
    return res


class _Model:
    """the log as a list of ids in append order: the records of the batches that were answered or are announced (a cancelled
    batch's records leave the list, also when a drain has handed them out already)"""

    def __init__(self, cap):
        self.cap, self.log, self.next_id, self.cursor, self.pending, self.gone = cap, [], 1, 0, None, 0

    def append(self, m):
        self.log += list(range(self.next_id, self.next_id + m))
        self.next_id += m

    def op(self, c, x):
        if c == PASS:
            self.append(x)
        elif c == ANNOUNCE:
            self.append(x)
            self.pending = x
        elif c == KEEP:
            self.pending = None
        elif c == CANCEL:
            # the batch's records are in the ring although it is taken back: what they overwrote before it was drained is gone
            over = max(0, len(self.log) - self.cursor - self.cap)
            self.cursor += over
            self.gone += over
            if self.pending:
                del self.log[len(self.log) - self.pending:]
            self.cursor = min(self.cursor, len(self.log))
            self.pending = None
        elif c == DRAIN:
            lapped = max(0, len(self.log) - self.cursor - self.cap)
            self.cursor += lapped
            lost, self.gone = lapped + self.gone, 0
            out = self.log[self.cursor:self.cursor + x]
            self.cursor += len(out)
            return out, lost
        return None

    def tail(self):
        """what dint_read_log returns: the ring position behind the answered batches"""
        return (len(self.log) - (self.pending or 0)) % self.cap


def _check(cap, ops):
    m = _Model(cap)
    for k, ((c, x), (tail, appended, drained, other, got)) in enumerate(zip(ops, _walk(cap, ops))):
        want = m.op(c, x)
        where = (cap, ops[:k + 1])
        assert tail == m.tail(), where
        assert appended == len(m.log), where
        assert drained == m.cursor, where
        if m.pending is not None:  # the word the announced partition wrote: behind its records
            assert other == len(m.log) % cap, where
        if c == DRAIN:
            assert got == want, where
        if c == CANCEL:
            assert other == tail, where  # both words say where the ring stands


def _counts(cap):
    return sorted({0, 1, max(cap - 1, 0), cap})


@pytest.mark.parametrize("cap", [1, 2, 255, 256])
def test_a_cancelled_announcement_leaves_tail_count_and_cursor_as_if_never_seen(cap):
    """cancelled batches of 0, 1, cap - 1 and cap log records -- cap moves the tail once round the ring, so the two tail words
    are equal and only the batch's own count says what to take back --, at both parities of the pass number, with and without
    a drain between announcement and cancel, followed by a batch of fewer, as many and more records than the cancelled one"""
    for m, parity, window, after in itertools.product(_counts(cap), (0, 1), (False, True), _counts(cap)):
        ops = [(PASS, min(3, cap))] + [(PASS, min(5, cap))] * parity + [(DRAIN, 4 * cap)]
        ops += [(PASS, min(2, cap)), (ANNOUNCE, m)]
        if window:
            ops.append((DRAIN, 4 * cap))
        ops += [(CANCEL, 0), (DRAIN, 4 * cap), (PASS, after), (DRAIN, 4 * cap), (PASS, min(1, cap)), (DRAIN, 4 * cap)]
        _check(cap, ops)


@pytest.mark.parametrize("cap", [1, 2, 255, 256])
def test_kept_announcements_and_cancels_in_a_chain(cap):
    """announce, keep, announce from the kept pass, cancel, announce again ..: the ring goes round several times, drains of a
    few records at a time in between (a cursor in the middle of the ring), and drains that come too late (lost > 0)"""
    rng = np.random.default_rng(cap)
    ops, announced = [(PASS, min(cap, 7))], False
    for _ in range(400):
        r = rng.random()
        x = int(rng.choice(_counts(cap) + [int(rng.integers(0, cap + 1))]))
        if announced:
            ops.append((KEEP, 0) if r < 0.5 else (CANCEL, 0) if r < 0.8 else (DRAIN, int(rng.integers(0, 2 * cap + 1))))
            announced = ops[-1][0] == DRAIN
            if ops[-1][0] == KEEP and rng.random() < 0.5:
                ops.append((ANNOUNCE, x))
                announced = True
        elif r < 0.4:
            ops += [(PASS, x), (ANNOUNCE, int(rng.integers(0, cap + 1)))]
            announced = True
        elif r < 0.7:
            ops.append((PASS, x))
        else:
            ops.append((DRAIN, int(rng.integers(0, 2 * cap + 1))))
    if announced:
        ops.append((CANCEL, 0))
    ops.append((DRAIN, 4 * cap))
    _check(cap, ops)
    assert sum(c == CANCEL for c, _ in ops) > 20 and sum(x for c, x in ops if c in (PASS, ANNOUNCE)) > 4 * cap


def test_the_distance_of_the_tail_words_is_not_the_cancelled_count():
    """what ahead_cancel used to subtract, (tail[c ^ 1] + cap - tail[c]) % cap, is 0 for a batch of exactly cap records: the walk
    shows the two words equal before the cancel, and the appended count back at its old value after it"""
    cap = 256
    res = _walk(cap, [(PASS, 10), (DRAIN, 1000), (ANNOUNCE, cap), (CANCEL, 0), (PASS, 3), (DRAIN, 1000)])
    assert res[1][4] == (list(range(1, 11)), 0)
    assert res[2][0] == res[2][3] == 10 and res[2][1] == 10 + cap
    assert res[3][:4] == (10, 10, 10, 10)
    assert res[5][4] == ([cap + 11, cap + 12, cap + 13], 0)


def test_what_a_cancelled_batch_overwrote_before_it_was_drained_is_reported_lost():
    """the batch's records stay in the ring although it is taken back: 10 records wait when a batch of cap records is announced and
    cancelled -- none of the 10 is left, and the next drain says so instead of handing out the cancelled batch's bytes"""
    cap = 256
    res = _walk(cap, [(PASS, 10), (ANNOUNCE, cap), (CANCEL, 0), (DRAIN, 1000), (PASS, 2), (DRAIN, 1000)])
    assert res[2][:4] == (10, 10, 10, 10)
    assert res[3][4] == ([], 10)
    assert res[5][4] == ([cap + 11, cap + 12], 0)


def test_arguments():
    L = _lib.load()
    out = np.zeros(64, np.uint64)

    def call(cap, ops, out_cap=64):
        a = np.array(ops, np.uint32).reshape(-1, 2)
        return L.dint_log_ring_host(cap, a.ctypes.data, len(a), out.ctypes.data, out_cap)

    assert call(0, [(PASS, 0)]) == EINVAL
    assert call(4, [(PASS, 5)]) == EINVAL and b"dint_log_ring_host" in L.dint_last_error()  # (a pass is clamped to the ring)
    assert call(4, [(ANNOUNCE, 1)]) == EINVAL  # no pass for the announcement to ride in
    assert call(4, [(PASS, 1), (KEEP, 0)]) == EINVAL and call(4, [(PASS, 1), (CANCEL, 0)]) == EINVAL
    assert call(4, [(PASS, 1), (ANNOUNCE, 1), (PASS, 1)]) == EINVAL and call(4, [(PASS, 1), (ANNOUNCE, 1), (ANNOUNCE, 1)]) == EINVAL
    assert call(4, [(PASS, 1), (7, 0)]) == EINVAL
    assert call(4, [(PASS, 4), (DRAIN, 9)], out_cap=13) == EINVAL and call(4, [(PASS, 4), (DRAIN, 9)], out_cap=14) == 14
    assert L.dint_log_ring_host(4, None, 0, None, 0) == 0 and L.dint_log_ring_host(4, None, 1, None, 0) == EINVAL
