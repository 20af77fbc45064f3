"""tests/mlp_eval_ref.py without a GPU: the reference's conditions hold on every case of the GPU tables (so a GPU run never
discovers a bad input); the blocked fp32 emulation of the kernel passes the very checks the kernel is held to -- inside the
bound on the bound tier, bit-equal on the exact tier, the staged tile element for element, fused equal to chained --; and each
planted defect is rejected by them, while the whole-tensor norms of tests/test_mlp_eval_gpu.py accept most of them.
`pytest -s` prints the worst |err| / tol per form and the old norms' verdict on every defect."""
import functools

import pytest
import torch

import mlp_eval_ref as M

_WORST = {}
_SHARES = {"bf16-exact": 1.0, "alive": 1.0, "alive (ReLU cases) max": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nemulation, largest |err| / tol per form: " + "  ".join("%s %.3g" % kv for kv in sorted(_WORST.items())))
    print("exact tier, smallest shares: " + "  ".join("%s %.3g" % kv for kv in _SHARES.items()))


def _cpu(launch):
    def run(layers, tail=None, grouped=None, rows=None, pool=False):
        return launch(layers, tail=tail, grouped=grouped, rows=rows, pool=pool)
    return run


@pytest.mark.parametrize("c", M.ROWS_CASES + M.GROUPED_CASES, ids=M.case_id)
def test_single_layer_conditions_and_emulation(c):
    hold = M.Hold(M.case_id(c), _WORST)
    shares = M.hold_single(c, _cpu(M.emulate), hold)
    hold.assert_ok()
    if c["tier"] == "exact":
        share, alive = shares
        _SHARES["bf16-exact"] = min(_SHARES["bf16-exact"], share)
        _SHARES["alive"] = min(_SHARES["alive"], alive)
        if c["relu"]:
            _SHARES["alive (ReLU cases) max"] = max(_SHARES["alive (ReLU cases) max"], alive)
        assert share >= M.BF16_EXACT_SHARE, "only %.4f of the outputs have bf16(z) == z" % share
        assert alive >= M.ALIVE_SHARE, "only %.3f of the outputs are positive" % alive


@pytest.mark.parametrize("c", M.TAIL_CASES, ids=M.case_id)
def test_tail_emulation(c):
    hold = M.Hold(M.case_id(c), _WORST)
    M.hold_tail(c, _cpu(M.emulate), hold)
    hold.assert_ok()


@pytest.mark.parametrize("c", M.PROBE_CASES, ids=M.case_id)
def test_probe_emulation(c):
    hold = M.Hold(M.case_id(c), _WORST)
    x = M.hold_probe(c, _cpu(M.emulate), hold)
    hold.assert_ok()
    K = 3 + c["C"] if "C" in c else c["K"]
    assert x.shape[1] == M.ceil32(K) and bool((x[:, K:] == 0).all()) and bool(torch.isfinite(x.float()).all())


@pytest.mark.parametrize("c", M.CHAIN_CASES, ids=M.case_id)
def test_chain_emulation(c):
    hold = M.Hold(M.case_id(c), _WORST)
    M.hold_chain(c, _cpu(M.emulate), hold)
    hold.assert_ok()


def test_tables_reach_every_mechanism():
    """what the issue lists, counted on the tables"""
    rows = [c for c in M.ROWS_CASES if c["tier"] == "bound"]
    assert {c["R"] for c in rows} == set(M.ROWS_R) and {c["K"] for c in rows} == set(M.ROWS_K)
    assert {(c["K"], c["n"]) for c in rows} >= {(K, n) for K in M.ROWS_K for n in M.WIDTHS}
    for flag in ("relu", "affine", "bias", "ldx_gap", "ldw_gap"):
        assert {c[flag] for c in rows} == {True, False}, flag
    gr = [c for c in M.GROUPED_CASES if c["tier"] == "bound"]
    assert {(c["C"], (c["B"], c["M"], c["S"])) for c in gr} == {(C, b) for C in M.GROUPED_C for b in M.GROUPED_BMS}
    assert {c["radius"] for c in gr} == {0.2, 0.4} and {c["normalize"] for c in gr} == {True, False}
    assert {c["radius"] for c in M.GROUPED_CASES if c["tier"] == "exact"} == {0.5}
    assert all(50 <= c["N"] <= 700 for c in M.GROUPED_CASES)
    assert {(c["n_tail"], c["tail_bias"]) for c in M.TAIL_CASES} == {(n, b) for n in M.TAIL_N for b in (True, False)}
    assert {c["C"] for c in M.PROBE_CASES if "C" in c} == set(M.GROUPED_C)
    assert {c["K"] for c in M.PROBE_CASES if "K" in c} == set(M.ROWS_K)
    for key in ("K", "C"):         # rows and grouped (unpooled and pooled), each also with the tail
        for with_tail in (False, True):
            assert {c["widths"] for c in M.CHAIN_CASES if key in c and bool(c.get("n_tail")) == with_tail} == set(M.CHAIN_WIDTHS)
    # a (3, 5, 16) case has a 64-row tile that spans two scenes; the grouped inputs hold what the issue asks of idx
    gi = M.grouped_input(0, 3, 5, 16, 7, 50, "bound", 0.2, True)
    idx = gi["idx"]
    B, Mm, S = M.GROUPED_BMS[-1]
    R = B * Mm * S
    assert any(r0 // (Mm * S) != min(r0 + M.TM - 1, R - 1) // (Mm * S) for r0 in range(0, R, M.TM))
    assert int(idx.min()) == 0 and int(idx.max()) == 49 and bool((idx[..., 8:-1] == idx[..., :1]).all())
    assert bool(torch.isnan(gi["cloud"][..., -2:]).all()) and bool(torch.isfinite(gi["cloud"][..., :-2]).all())


# ---- planted defects ------------------------------------------------------------------------------------------------------------
def _g(id_, B, Mm, S, C, n, relu=True):
    return dict(id=id_, tier="bound", B=B, M=Mm, S=S, C=C, N=173, n=n, radius=0.2, normalize=True, relu=relu, affine=True,
                bias=True, ldw_gap=False)


_ROWS = dict(id=9002, tier="bound", R=301, K=256, n=256, relu=True, affine=True, bias=True, ldx_gap=False, ldw_gap=False)
_TAIL = dict(id=9006, tier="bound", R=301, K=256, n=256, n_tail=259, tail_bias=True)
_CHAIN = dict(id=9007, tier="bound", R=301, K=256, widths=(256, 256))
# name: (case, the hold function, the defect)
DEFECTS = {
    "one gathered row takes its neighbour's index": (_g(9000, 2, 37, 16, 132, 64), M.hold_single, ("neighbour", 5 * 16 + 2)),
    "the batch index of a straddling tile comes from its first row": (_g(9001, 3, 5, 16, 7, 64), M.hold_single, ("batch_first_row",)),
    "the last k-step dropped for one 16 x 16 tile": (_ROWS, M.hold_single, ("drop_kstep", 1, 3)),
    "t of one channel formed without the conv bias": (_ROWS, M.hold_single, ("no_bias", 7)),
    "one group pooled over S - 1 rows": (_g(9004, 2, 37, 16, 132, 64), M.hold_single, ("pool_short", 2 * 37 - 1)),
    "a pooled max that starts from 0": (_g(9005, 2, 37, 16, 132, 64, relu=False), M.hold_single, ("pool_from_0", 11)),
    "tail column 256 of 259 left at zero": (_TAIL, M.hold_tail, ("tail_col", 256)),
    "the intermediate activation kept in fp32": (_CHAIN, M.hold_chain, ("f32_intermediate",)),
}


def _natural(c, launch):
    """the output the old tests look at: pooled for a grouped case, the tail's or the last layer's rows otherwise"""
    x, K, kw = M.case_rows(c)
    if "widths" in c:
        layers, tail = M.chain_specs(c)
    else:
        layers = [M.layer_spec(c["id"], K, c["n"], "bound", c.get("relu", True), c.get("affine", True), c.get("bias", False), False)]
        tail = M.tail_spec(c["id"], c["n"], c["n_tail"], c["tail_bias"]) if c.get("n_tail") else None
    S = c.get("S", 0)
    return launch(layers, tail=tail, pool=bool(S), **kw), M.fp32_composition(x, layers, tail, S)


@functools.lru_cache(maxsize=None)
def _plant(name):
    """(the new comparison's failures with the defect planted, the old norms' verdict on it)"""
    c, hold_fn, defect = DEFECTS[name]
    clean = M.Hold(name, {})
    hold_fn(c, _cpu(M.emulate), clean)
    clean.assert_ok()
    planted = M.Hold(name, {})
    bad = _cpu(functools.partial(M.emulate, defect=defect))
    hold_fn(c, bad, planted)
    out, ref32 = _natural(c, bad)
    emu, _ = _natural(c, _cpu(M.emulate))
    return planted.fails, M.old_norms_accept(out, emu, ref32)


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_is_rejected(name):
    fails, old = _plant(name)
    print("\n%s: the new comparison rejects it (%d findings); the old norms %s it" % (name, len(fails), "ACCEPT" if old else "reject"))
    assert fails, "the planted defect passed: " + name


def test_old_norms_accept_at_least_four_of_the_defects():
    accepted = [name for name in DEFECTS if _plant(name)[1]]
    print("\nthe old norms accept %d of %d: %s" % (len(accepted), len(DEFECTS), "; ".join(accepted)))
    assert len(accepted) >= 4
    assert all(_plant(name)[0] for name in DEFECTS)


def test_old_norms_restated():
    assert M.OLD_NORMS == dict(emulation=3e-3, fp32=1e-2)
    a = torch.ones(4, 4)
    assert M.old_norms_accept(a, a, a) and not M.old_norms_accept(a * 1.02, a, a)
