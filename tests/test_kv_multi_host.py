"""Host checks of the launch-set schedules of tests/kv_multi.py (no GPU): they are conditions on the inputs of
tests/test_gpu_kv_multi.py and must hold before anything runs on a GPU -- a schedule that never puts an idle engine beside a
full one, or a tiny one beside a large one, would let the block ranges of k_kv_pass go untested without anyone noticing."""
import numpy as np
import pytest

import kv_multi as km

NAMES = sorted(km.SETS)


@pytest.mark.parametrize("name", NAMES)
def test_every_segment_fits_and_the_layout_round_trips(name):
    s, bufs = km.cached(name)
    msg = s.dtype.itemsize
    assert s.stride >= 64 + s.seg_cap * msg
    for j in range(len(s.steps)):
        for k, c in enumerate(s.cases):
            cuts = s.cuts(j, k)
            assert all(0 <= b - a <= s.seg_cap for a, b in zip(cuts[:-1], cuts[1:])), (j, k, cuts)
            assert cuts[2] == cuts[1] and cuts[1] == (cuts[3] + 1) // 2  # segment 1 is empty, segment 0 holds ceil(n / 2)
            a, b = bufs[j][k]
            assert len(a) == len(b) == km.N_SEG * s.stride
            cnt = [int(a[i * s.stride:i * s.stride + 4].view("<u4")[0]) for i in range(km.N_SEG)]
            assert cnt == [cuts[i + 1] - cuts[i] for i in range(km.N_SEG)]
            assert km.padding_untouched(a, cuts, s.stride, msg) and km.padding_untouched(b, cuts, s.stride, msg)
            p = s.steps[j][k]
            if p is None:
                assert cnt == [0, 0, 0] and (a[4:64] == km.PAD).all()
                continue
            assert km._unsegment(a, cuts, s.stride, s.dtype).tobytes() == c.passes[p].tobytes()
            assert km._unsegment(b, cuts, s.stride, s.dtype).tobytes() == c.want[p].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_every_engine_meets_each_of_its_passes_once_and_in_order(name):
    s = km.schedule(name)
    assert len({c.wl for c in s.cases}) == 1
    for k, c in enumerate(s.cases):
        seen = [row[k] for row in s.steps]
        assert [p for p in seen if p is not None] == list(range(len(c.passes)))
        assert seen[:k] == [None] * k and all(p is not None for p in seen[k:k + len(c.passes)])  # the stagger: nothing before, nothing after
        assert len(c.want) == len(c.passes)


@pytest.mark.parametrize("name", NAMES)
def test_an_idle_engine_stands_beside_a_full_one(name):
    s = km.schedule(name)
    sizes = [[s.live(j, k) for k in range(len(s.cases))] for j in range(len(s.steps))]
    assert any(min(row) == 0 and max(row) >= km.BIG[s.wl] for row in sizes), sizes
    for row in (sizes[0], sizes[-1]):  # the first and the last step
        assert min(row) == 0 and max(row) > 0, sizes


def _ratio(name):
    s = km.schedule(name)
    best = 0.0
    for j in range(len(s.steps)):
        live = [n for n in (s.live(j, k) for k in range(len(s.cases))) if n]
        if len(live) > 1:
            best = max(best, max(live) / min(live))
    return best


@pytest.mark.parametrize("name", [n for n in NAMES if n != "tatp2"])
def test_a_small_engine_stands_beside_one_ten_times_its_size(name):
    assert _ratio(name) >= 10


def test_tatp2_has_a_small_engine_beside_one_eight_times_its_size():
    """tatp2 cannot reach the factor of ten the other sets are held to: its two engines' passes meet as 900 | 300,
    3,000 | 1,000 and 500 | 4,000 and the hot-pair engine is alone from then on -- the staggered pass sizes of the cases leave
    8 (4,000 beside 500) as the largest ratio.  What the set is for is the long idle stretch (four steps of one engine alone),
    asserted above for every set and here once more."""
    assert _ratio("tatp2") >= 8
    s = km.schedule("tatp2")
    assert sum(s.live(j, 1) == 0 and s.live(j, 0) > 0 for j in range(len(s.steps))) >= 4


def test_the_geometry_is_one_kernel_pass_and_the_largest_passes_fit():
    for name in NAMES:
        s = km.schedule(name)
        assert km.N_SEG * s.seg_cap <= 1 << 20  # (a kv engine's largest kernel pass)
        assert max(len(p) for c in s.cases for p in c.passes) <= 2 * s.seg_cap
    assert len(km.SETS["store5"]()) == 5 and len(km.SETS["tatp4"]()) == 4


def test_segment_layout_on_odd_sizes():
    dt = np.dtype([("a", "<u4"), ("b", "u1", 3)])
    for n in (0, 1, 2, 7, 33):
        x = np.zeros(n, dt)
        x["a"] = np.arange(n)
        cuts = km.cuts_of(n)
        buf, stride, nseg = km._segmented(x, cuts, 20)
        assert nseg == 3 and stride == 64 + 192 and len(buf) == 3 * stride
        assert km._unsegment(buf, cuts, stride, dt).tobytes() == x.tobytes()
        assert km.padding_untouched(buf, cuts, stride, dt.itemsize)
