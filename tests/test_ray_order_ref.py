"""tests/ray_order_ref.py proved without a GPU: the incremental walk of vr_regroup_kernel visits the pairs it is meant
to, the index lists are large enough for every patch count and set size, the block's size is its layout's end, and the
restatement of a patch's run agrees with a brute-force enumeration."""
import numpy as np
import pytest

from tests import ray_order_ref as ror


def test_walk_visits_pair_64_step_plus_lane_and_covers_every_pair_once():
    for sf in range(2, ror.MAX_FRAMES + 1):
        seen = []
        for step, lanes in enumerate(ror.regroup_walk(sf)):
            for lane, (px, f) in enumerate(lanes):
                assert 0 <= f < sf and 0 <= px < 64, (sf, step, lane, px, f)
                assert px * sf + f == 64 * step + lane, (sf, step, lane, px, f)
                seen.append(px * sf + f)
        assert seen == list(range(64 * sf)), sf


def test_index_lists_hold_every_patch_of_their_list():
    """A list takes ceil(P / 8) patches of at most 64 * sf entries (a multiple of every group size)."""
    P = np.arange(1, 4097, dtype=np.int64)[:, None]
    sf = np.arange(2, ror.MAX_FRAMES + 1, dtype=np.int64)[None, :]
    n = P * sf
    cap = 8 * n + 64 * sf
    assert (cap < 1 << 32).all()                                      # (pm_list_cap does not wrap in this range)
    assert cap[7, 3] == ror.pm_list_cap(8 * 5, 5) and cap[0, 0] == ror.pm_list_cap(2, 2)
    need = (P + ror.LISTS - 1) // ror.LISTS * 64 * sf
    assert (cap >= need).all()
    for group in ror.GROUPS:                                          # a full run needs no padding in any group
        assert (64 * sf % group == 0).all()
    # ... and a ray list every record of its items: items q with q % 8 == k, at most 64 records each
    for items in (1, 7, 8, 9, 40, 5120):
        assert ror.live_list_cap(items) >= -(-items // ror.LISTS) * 64


@pytest.mark.parametrize("n,sf", [(2, 2), (40, 2), (100, 5), (20 * 256, 256), (4096 * 256, 256), (16384 * 32, 32),
                                  (3 * 10 ** 7, 3)])
def test_block_words_equal_the_layouts_end(n, sf):
    parts = ror.block_layout(n, sf)
    assert parts[0][1] == 0
    for (_, _, end), (_, start, _) in zip(parts, parts[1:]):
        assert end == start                                           # no gap, no overlap
    assert [p[0] for p in parts[:2]] == ["ballots", "first"] and parts[2][1] == 3 * n
    assert parts[-1][2] == ror.pm_block_words(n, sf)
    # the host uses the order only where the block fits 32-bit indices: there the device's 32-bit capacity is the
    # layout's, and the last entry's index fits as well
    if ror.pm_block_words(n, sf) <= 0xFFFFFFFF:
        assert ror.pm_list_cap(n, sf) == ror.pm_list_cap(n, sf, None)
        assert 3 * n + (ror.LISTS - 1) * ror.pm_list_cap(n, sf) + ror.pm_list_cap(n, sf) - 1 < 1 << 32


def test_padded_length():
    for total in range(0, 200):
        assert ror.padded_length(total, 1) == total
        for g in (32, 64):
            p = ror.padded_length(total, g)
            assert p % g == 0 and total <= p < total + g


@pytest.mark.parametrize("sf", [2, 3, 5, 8, 9, 63, 64, 65, 256])
def test_restatement_against_brute_force(sf):
    rng = np.random.default_rng(1000 + sf)
    for trial in range(20):
        density = rng.random()
        bits = rng.random((sf, 64)) < density
        if trial == 0:
            bits[:] = True
        if trial == 1:
            bits[:] = False
        if trial == 2:
            bits[1:] = False                                          # live in one frame only
        ballots = [sum(1 << px for px in range(64) if bits[f, px]) for f in range(sf)]
        firsts = [int(v) * 64 for v in rng.permutation(1 << 12)[:sf]]  # (records of different items never overlap)
        got = ror.expected_run(ballots, firsts)
        assert got == ror.brute_force_run(ballots, firsts)
        assert len(got) == int(bits.sum())
        assert [(px, f) for _, px, f in got] == sorted((px, f) for _, px, f in got)
        assert len({at for at, _, _ in got}) == len(got)


def test_expected_runs_and_split():
    sf, patches, group = 3, 19, 32
    rng = np.random.default_rng(7)
    ballot = np.array([int(rng.integers(0, 1 << 63)) if rng.random() < 0.7 else 0 for _ in range(sf * patches)],
                      dtype=np.uint64)
    ballot[3 * sf:4 * sf] = 0                                         # a patch dead in every frame
    first = np.arange(sf * patches, dtype=np.int64) * 64
    runs = ror.expected_runs(sf, ballot, first, group)
    assert 3 not in runs and all(len(r) % group == 0 for r in runs.values())
    for k in range(ror.LISTS):
        mine = {p: r for p, r in runs.items() if p % ror.LISTS == k}
        order = sorted(mine, reverse=True)                            # any order of the runs will do
        entries = np.concatenate([mine[p] for p in order]) if order else np.zeros(0, np.uint32)
        assert ror.split_runs(entries, mine) == order
        if order:
            bad = entries.copy()
            bad[0], bad[1] = entries[1], entries[0]                   # two entries swapped: not the restatement's run
            with pytest.raises(AssertionError):
                ror.split_runs(bad, mine)
            with pytest.raises(AssertionError):                       # a run cut short
                ror.split_runs(entries[:-1], mine)
