"""The lane map's slot arithmetic (brs_state.hpp: lane_slot) compiled for the host: it must be a permutation of the lane slots
for any bucket counts, start every expensive bucket on a wave boundary while there are far lanes to fill the gaps, and fill
the most expensive buckets first when there are not."""
import numpy as np
import pytest

from tests.lane_map_cases import WAVE, compile_lanemap, layout, owner_of


def _compile(tmp_path_factory, cap):
    return compile_lanemap(tmp_path_factory.mktemp("lanemap"), cap)


@pytest.fixture(scope="module", params=[64, 16, 7])
def lm(request, tmp_path_factory):
    return _compile(tmp_path_factory, request.param)


def expensive_order(L):
    return [L.lm_bucket_order(o) for o in range(L.lm_nbucket() - 1)]


def gaps(L, cnt):
    """far lanes needed to fill every expensive bucket's last wave (cap off, buckets in slot order from a boundary)"""
    return sum((-c) % WAVE for b, c in enumerate(cnt) if b != L.lm_far())


def test_bucket_order_is_a_permutation(lm):
    far = lm.lm_far()
    order = expensive_order(lm)
    assert sorted(order + [far]) == list(range(lm.lm_nbucket()))


def test_random_counts_are_permutations(lm):
    rng = np.random.default_rng(0)
    nb = lm.lm_nbucket()
    for t in range(400):
        scale = rng.choice([3, 40, 300, 5000])
        cnt = rng.integers(0, scale, size=nb)
        cnt[rng.random(nb) < 0.3] = 0  # empty buckets
        if t % 4 == 0:
            cnt[lm.lm_far()] = rng.integers(0, 70)  # too few far lanes to fill every gap
        if cnt.sum() == 0:
            cnt[0] = 1
        layout(lm, cnt)


def test_expensive_buckets_start_on_wave_boundaries(lm):
    """with far lanes to spare, every expensive bucket starts on a wave boundary, in slot order, and no wave holds two
    expensive buckets; N need not be a multiple of 64"""
    rng = np.random.default_rng(1)
    far, order, cap = lm.lm_far(), expensive_order(lm), lm.lm_rare_cap()
    for _ in range(200):
        cnt = rng.integers(0, 900, size=lm.lm_nbucket())
        cnt[rng.random(len(cnt)) < 0.2] = 0
        cnt[far] = gaps(lm, cnt) + 64 * sum(-(-c // cap) for b, c in enumerate(cnt) if b & 2) + rng.integers(0, 100)
        owner, per = layout(lm, cnt)
        starts = [int(per[b].min()) for b in order if cnt[b]]
        assert all(s % WAVE == 0 for s in starts), (cnt.tolist(), starts)
        assert starts == sorted(starts), "buckets out of slot order"
        for w in range(0, len(owner), WAVE):
            kinds = set(owner[w:w + WAVE].tolist()) - {far}
            assert len(kinds) <= 1, f"wave {w // WAVE} holds buckets {kinds}"


@pytest.mark.parametrize("cap", [32, 7])
def test_wheel_cap(cap, tmp_path_factory):
    """BRS_RARE_CAP < 64: a wheel bucket (key bit 1) holds at most that many lanes per wave while there are far lanes to fill
    the waves; the buckets without a wheel keep whole waves"""
    lm = _compile(tmp_path_factory, cap)
    assert lm.lm_rare_cap() == cap
    cnt = np.array([5000, 300, 700, 150, 9000, 900, 3, 60])
    owner, per = layout(lm, cnt)
    for w in range(0, len(owner), WAVE):
        o = owner[w:w + WAVE]
        for b in (2, 3, 6, 7):
            assert (o == b).sum() <= cap
    for b in (2, 3, 6, 7):
        assert len(np.unique(per[b] // WAVE)) == -(-cnt[b] // cap)
    # the most expensive bucket comes first, its lanes spread evenly over its waves
    assert (owner[:WAVE] == 3).sum() == -(-cnt[3] // -(-cnt[3] // cap))


def test_no_dilution_at_run_time_cap_64(tmp_path_factory):
    """brs_step passes cap 64 for launches of more waves than the GPU has SIMDs: wheel buckets keep whole waves"""
    lm = _compile(tmp_path_factory, 16)
    cnt = np.array([5000, 300, 700, 150, 9000, 900, 3, 60])
    _, per = layout(lm, cnt, 64)
    for b in (2, 3, 6, 7):
        assert len(np.unique(per[b] // WAVE)) == -(-cnt[b] // WAVE)
        assert per[b].min() % WAVE == 0


def test_dilution_with_too_few_far_lanes(tmp_path_factory):
    """a wheel bucket that the far lanes left cannot dilute to the cap is spread over as many whole waves as they allow"""
    lm = _compile(tmp_path_factory, 8)
    cnt = np.array([3000, 0, 1000, 0, 2000, 0, 0, 0])  # 1000 wheel lanes at 8 per wave would need 7000 far lanes
    owner, per = layout(lm, cnt)
    waves = np.unique(per[2] // WAVE)
    assert len(waves) == (1000 + 2000) // WAVE and waves[0] == 0 and np.all(np.diff(waves) == 1)
    assert max((owner[w * WAVE:(w + 1) * WAVE] == 2).sum() for w in waves) == -(-1000 // len(waves))
    assert per[0].min() % WAVE == 0


def test_too_few_far_lanes_fills_the_most_expensive_first(lm):
    far, order = lm.lm_far(), expensive_order(lm)
    cnt = np.zeros(lm.lm_nbucket(), dtype=np.int64)
    cnt[order[0]], cnt[order[1]], cnt[order[2]], cnt[0] = 70, 100, 10, 1000
    cnt[far] = (-70) % WAVE + 5  # enough for the first bucket's gap only
    owner, per = layout(lm, cnt)
    assert per[order[1]].min() % WAVE == 0 and per[order[0]].min() == 0
    # nothing to fill with: the buckets follow each other back to back, in slot order
    cnt[far] = 0
    owner, per = layout(lm, cnt)
    pos = 0
    for b in order:
        if cnt[b]:
            assert np.array_equal(np.sort(per[b]), np.arange(pos, pos + cnt[b]))
            pos += cnt[b]


def test_owner_of_is_the_layout_at_a_run_time_cap(tmp_path_factory):
    """lane_map_cases.owner_of (what the GPU tests hold the device map to): the default build at a run-time cap lays the
    buckets out like a build compiled with that cap"""
    cnt = np.array([5000, 300, 700, 150, 9000, 900, 3, 60])
    for cap in (64, 16, 7):
        assert np.array_equal(owner_of(cnt, cap), layout(_compile(tmp_path_factory, cap), cnt)[0])
