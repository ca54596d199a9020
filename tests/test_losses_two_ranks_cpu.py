"""tests/losses_two_ranks_cases.py checked against itself, without a GPU: the CPU emulation of two ranks stays inside the derived
bounds on every route tests/test_losses_two_ranks_gpu.py runs, every mutation of the data-parallel arrangement leaves them on
every route it applies to, and the float64 references agree with each other where the losses' docstrings say the losses do."""
import functools

import pytest
import torch

from tests import losses_two_ranks_cases as K
from tests import supcon_cases as S
from tests import supcon_ml_cases as ML


@functools.lru_cache(maxsize=None)
def _reference(form):
    inp = K.inputs()
    ref = K.reference(form, inp["na"], inp["nb"], K.meta_of(form, inp))
    return ref, K.caller_view(ref, inp["za"], inp["zb"], inp["na"], inp["nb"])


@functools.lru_cache(maxsize=None)
def _ratios(form, mutation=None):
    ref, view = _reference(form)
    return K.ratios(ref, view, K.emulate_two_ranks(form, mutation))


def _show(r):
    return " ".join(f"{k}={v:.3g}" for k, v in r.items())


def test_the_plan_puts_positives_on_the_other_rank():
    inp = K.inputs()
    lab, (lo1, hi1) = inp["labels"], K.SHARDS[1]
    assert K.SHARDS == [(0, 151), (151, 301)]
    first, second = set(lab[:lo1].tolist()), set(lab[lo1:hi1].tolist())
    used = {c for c in first | second if c >= 0}
    assert used and all(c in first and c in second for c in used)             # every class has members in both shards
    assert 0 in used and max(used) < 64
    assert {-1, -7} <= first and {-1, -7} <= second
    a, b = K.PAIR_ROWS
    assert a < lo1 <= b and int((lab == K.PAIR_CLASS).sum()) == 2              # its only other member lives on the other rank
    words = inp["words"]
    assert torch.equal(ML.pack_torch(inp["multi_hot"]), words)
    assert bool((words < 0).any()) and bool((words == 0).any())               # class 63 (the sign bit) and empty sets
    ov, ja = ML.weights(words, words, 0, "overlap"), ML.weights(words, words, 0, "jaccard")
    assert bool(((ov == 1) & (ja > 0) & (ja < 1)).any())                      # partial overlap: the weightings differ
    assert bool(((ja > 0) & (ja < 1))[:lo1, lo1:].any())                      # ... across the seam too
    za, na = inp["za"].float(), inp["na"].float()
    assert not torch.allclose(za.norm(dim=1), torch.ones(K.N), atol=0.1)
    assert torch.equal(za / torch.exp2(za.norm(dim=1, keepdim=True).log2().round()), na)     # the scales are powers of two


@pytest.mark.parametrize("route", K.ROUTE_IDS)
def test_emulation_inside_the_bounds(route):
    form = K.ROUTES[route][3]
    r = _ratios(form)
    print(f"losses_two_ranks_emulation route {route} (form {form}): {_show(r)}")
    assert not K.outside(r), r
    results = K.emulate_two_ranks(form)
    assert results[0]["loss"] == results[1]["loss"]


# (a route without a self key, without column statistics or without labels has no such thing to break)
@pytest.mark.parametrize("route,mutation", [(route, mutation) for route in K.ROUTE_IDS for mutation in K.MUTATIONS
                                            if K.applies(mutation, K.ROUTES[route][3])])
def test_mutation_leaves_the_bounds(route, mutation):
    form = K.ROUTES[route][3]
    r = _ratios(form, mutation)
    print(f"losses_two_ranks_mutation route {route} (form {form}) {mutation}: {_show(r)}")
    assert K.outside(r), r


def test_every_mutation_applies_somewhere():
    for mutation in K.MUTATIONS:
        assert sum(K.applies(mutation, form) for form in K.FORMS) >= 2
    assert not K.applies("self_and_partner_swapped", "supcon_stream") and K.applies("self_and_partner_swapped", "pool_tile")


def test_pooled_references_without_labels_are_nt_xent():
    """pooled forms, every label -1 (or every set empty) == NT-Xent, in float64: loss, every term and dT"""
    inp = K.inputs()
    na, nb = inp["na"], inp["nb"]
    none = torch.full((K.N,), -1, dtype=torch.int64)
    empty = torch.zeros(K.N, dtype=torch.int64)
    pairs = (("ntxent_stream", None, "pool_stream", none), ("ntxent_tile", None, "pool_tile", none),
             ("ntxent_tile", None, "mlpool_tile_overlap", empty), ("ntxent_tile", None, "mlpool_tile_jaccard", empty))
    for f_nt, m_nt, f_pool, m_pool in pairs:
        nt, pool = K.reference(f_nt, na, nb, m_nt), K.reference(f_pool, na, nb, m_pool)
        assert abs(nt["loss"] - pool["loss"]) <= 1e-12 * abs(nt["loss"])
        assert max(abs(x - y) for x, y in zip(nt["dT"], pool["dT"])) <= 1e-12 * max(abs(x) for x in nt["dT"])
        for view in ("a", "b"):
            assert float((nt[view]["own"][0] - pool[view]["own"][0]).abs().max()) <= 1e-15
            for s_nt, s_pool in zip(nt[view]["shares"], pool[view]["shares"]):
                assert float((sum(v for v, _ in s_nt) - sum(v for v, _ in s_pool)).abs().max()) <= 1e-15
    # the streaming and the tile arrangement of one loss are one loss
    assert abs(K.global_loss("ntxent_stream", na, nb, None) - K.global_loss("ntxent_tile", na, nb, None)) <= 1e-12


def test_one_hot_sets_reference_is_the_single_label_reference():
    inp = K.inputs()
    na, nb, lab = inp["na"], inp["nb"], inp["labels"]
    words = K.one_hot_words(lab)
    assert torch.equal(words == 0, lab < 0)
    for f_lab, f_sets in (("supcon_stream", "ml_stream_overlap"), ("supcon_stream", "ml_stream_jaccard"), ("supcon_tile", "ml_tile_overlap"),
                          ("supcon_tile", "ml_tile_jaccard"), ("pool_tile", "mlpool_tile_overlap"), ("pool_tile", "mlpool_tile_jaccard")):
        one, two = K.reference(f_lab, na, nb, lab), K.reference(f_sets, na, nb, words)
        assert abs(one["loss"] - two["loss"]) <= 1e-12 * abs(one["loss"])
        assert max(abs(x - y) for x, y in zip(one["dT"], two["dT"])) <= 1e-12 * max(abs(x) for x in one["dT"])
        for view in ("a", "b"):
            if one[view]["own"] is not None:
                assert float((one[view]["own"][0] - two[view]["own"][0]).abs().max()) <= 1e-15
            if one[view]["shares"] is not None:
                for s1, s2 in zip(one[view]["shares"], two[view]["shares"]):
                    assert float((sum(v for v, _ in s1) - sum(v for v, _ in s2)).abs().max()) <= 1e-15
    # and the streaming and tile arrangements of the cross-view loss agree on the value
    assert abs(K.global_loss("supcon_stream", na, nb, lab) - K.global_loss("supcon_tile", na, nb, lab)) <= 1e-12
    m = S.match_matrix(lab, lab, 0)
    assert bool((m.sum(1) > 1).any())
