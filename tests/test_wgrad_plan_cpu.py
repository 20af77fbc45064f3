"""The deferred weight-gradient flush (bridgeqa_amd/fusion_wgrad.py) on plain numbers and CPU tensors: which launch a second
row source rides in, and that the launch planner never sees it.  _ext.gemm_grouped is replaced by a recorder; nothing runs."""
import types

import pytest
import torch

from bridgeqa_amd import fusion_wgrad as W


@pytest.fixture()
def recorder(monkeypatch):
    """flush_deferred_items with its launches and its planner recorded: (launches, plans); a launch = (tile, [problem dicts])"""
    from bridgeqa_amd import _ext
    launches, plans = [], []
    monkeypatch.setattr(_ext, "gemm_grouped", lambda probs, flags, epi, tile: launches.append((tile, probs)))
    monkeypatch.setattr(_ext, "colsum_grouped", lambda mats: [torch.zeros(m.shape[-1]) for m in mats])
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=256))
    real_plan = W.plan_big_launches

    def plan(tiles, cus, *a, **kw):
        plans.append((list(tiles), cus))
        return real_plan(tiles, cus, *a, **kw)
    monkeypatch.setattr(W, "plan_big_launches", plan)
    return launches, plans


def _twin_items(n_pairs, B=16, L1=64, L2=20, N=512, D=256, bias=True):
    """n_pairs parked twin K/V records: primary (B, L1, N) rows of a (B, L1 + L2, N) gradient, second source the other L2"""
    W.begin_deferred_wgrad()
    for _ in range(n_pairs):
        g = torch.zeros(B, L1 + L2, N, dtype=torch.bfloat16)
        ws = [torch.nn.Parameter(torch.zeros(N // 2, D)) for _ in range(2)]
        bs = [torch.nn.Parameter(torch.zeros(N // 2)) for _ in range(2)] if bias else None
        W._park_two(g[:, :L1], torch.zeros(B * L1, D, dtype=torch.bfloat16), g[:, L1:], torch.zeros(B * L2, D, dtype=torch.bfloat16), ws, bs)
    return W.take_deferred_wgrad()


def test_a_big_primary_takes_its_second_source_along(recorder):
    launches, plans = recorder
    items = _twin_items(3)
    W.flush_deferred_items(items)
    assert [t for t, _ in launches] == [256]                       # one launch: no adder behind it
    probs = launches[0][1]
    assert len(probs) == 3
    for pr, k in zip(probs, (0, 2, 4)):
        assert pr["Q"] is items[k][0] and pr["P"] is items[k][1]
        assert pr["Q2"] is items[k + 1][0] and pr["P2"] is items[k + 1][1]
        assert pr["Q2"].shape == (16, 20, 512) and "accum" not in pr and pr["colsum"].shape == (512,)
    # the planner counted the primaries' tiles alone: 512 / 256 x 256 / 256 = 2 each -- a segment adds none
    assert plans == [([2, 2, 2], 256)]


def test_the_plan_is_the_one_without_second_sources(recorder, monkeypatch):
    launches, plans = recorder
    W.flush_deferred_items(_twin_items(3))
    monkeypatch.setattr(W, "_TWO_SOURCE", [False])
    W.flush_deferred_items(_twin_items(3))
    assert plans[0] == plans[1]
    assert [t for t, _ in launches] == [256, 256, 64]              # switched off: the adder launch of before
    adder = launches[2][1]
    assert len(adder) == 3 and all(pr["accum"] is True and "P2" not in pr for pr in adder)
    assert all("P2" not in pr for pr in launches[1][1])
    for pr, prim in zip(adder, launches[1][1]):                    # onto the primary's stored gradient and bias gradient
        assert pr["out"] is prim["out"] and pr["colsum"] is prim["colsum"]


def test_a_primary_off_the_256_tile_launch_keeps_the_adder(recorder):
    launches, plans = recorder
    # 16 x 8 = 128 primary rows: below BIG_ROWS, and a batched-row view has no mid class => the 64-tile kernel, adder behind
    W.flush_deferred_items(_twin_items(2, L1=8))
    assert not plans
    assert [t for t, _ in launches] == [64, 64]
    assert all("P2" not in pr for _, probs in launches for pr in probs)
    assert all(pr.get("accum") for pr in launches[1][1]) and not any(pr.get("accum") for pr in launches[0][1])


def test_a_moved_primary_keeps_the_adder(recorder, monkeypatch):
    """what plan_big_launches sends to the 64-tile kernel is no longer on the 256-tile launch: its second source is added"""
    launches, plans = recorder
    monkeypatch.setattr(W, "plan_big_launches", lambda tiles, cus, *a, **kw: ([[0, 1]], [2]))
    items = _twin_items(3)
    W.flush_deferred_items(items)
    assert [t for t, _ in launches] == [256, 64, 64]
    assert [("P2" in pr) for pr in launches[0][1]] == [True, True]
    assert len(launches[1][1]) == 1 and "P2" not in launches[1][1][0]
    assert len(launches[2][1]) == 1 and launches[2][1][0]["accum"] is True and launches[2][1][0]["out"] is launches[1][1][0]["out"]


def test_split_for_table_deals_the_problems_and_fits_the_table():
    # the twin K/V flush: 24 two-source problems need 48 entries of 36 -> two launches of 12, long and short ones in both
    g = list(range(100, 124))
    assert W.split_for_table(g, [True] * 24) == [g[0::2], g[1::2]]
    assert W.split_for_table(g[:18], [True] * 18) == [g[:18]]                 # 36 entries: one launch
    assert W.split_for_table(g, [False] * 24) == [g]
    assert W.split_for_table([], []) == [[]]
    # every pattern: each problem exactly once, every launch within the table -- also where an even deal would not fit
    for n, two in ((36, [True] + [False] * 35), (37, [k % 2 == 0 for k in range(37)]), (30, [k < 20 for k in range(30)]),
                   (36, [k % 2 == 0 for k in range(36)]), (5, [True] * 5)):
        group = list(range(n))
        for cap in (36, 6):
            chunks = W.split_for_table(group, two, max_entries=cap)
            assert sorted(k for c in chunks for k in c) == group
            assert all(c and len(c) + sum(two[k] for k in c) <= cap for c in chunks), (n, cap, chunks)


def test_a_flush_of_more_pairs_than_a_table_holds_is_dealt(recorder):
    launches, plans = recorder
    W.flush_deferred_items(_twin_items(20))
    assert plans == [([2] * 20, 256)]                                  # planned as one launch of 40 tiles ...
    assert [t for t, _ in launches] == [256, 256]                     # ... issued as two that fit the table
    assert [len(p) for _, p in launches] == [10, 10] and all("P2" in pr for _, p in launches for pr in p)


def test_plan_big_launches_on_plain_numbers():
    # the ViT flush: 48 problems, 1296 tiles on 256 CUs -- a few of the smallest problems leave for five whole rounds
    tiles = [27] * 12 + [36] * 24 + [9] * 12     # qkv, fc1 + fc2, proj of 12 blocks
    groups, moved = W.plan_big_launches(tiles, 256)
    assert sorted([k for g in groups for k in g] + list(moved)) == list(range(48))
    assert sum(tiles) == 1296 and 1 <= len(moved) <= 5
    assert all(len(g) <= 36 for g in groups) and all(tiles[k] == 9 for k in moved)
    assert sum(-(-sum(tiles[k] for k in g) // 256) for g in groups) == 5
    # the twin K/V flush: 24 problems of 18 tiles, nothing to gain by moving
    assert W.plan_big_launches([18] * 24, 256) == ([list(range(24))], [])
