"""CPU-only tests of what tests/test_multiview_pairwise_gpu.py stands on (tests/multiview_pairwise_cases.py): the entry points of
multi-view InfoNCE with a temperature and a weight per pair load and refuse in their documented order; the Python surface checks
the per-pair arguments before it touches a device; the closed forms of the reference -- the per-pair dT among them -- are the
float64 autograd of the definition; an emulation of the design's arithmetic stays inside the derived bounds on every case and
plan; and the bounds have teeth -- the emulation with one broken rule leaves them on a named output of a named case and plan.
The refusals are host code: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import multiview_cases as C
from tests import multiview_pairwise_cases as Q

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_nce_multi_pp_workspace_bytes", "aecf_nce_multi_pp_pair_coef", "aecf_nce_multi_pp_pass1", "aecf_nce_multi_pp_loss",
         "aecf_nce_multi_pp_grads")
SMALL = ("V2", "V3A", "V8")         # V4 (2305 rows) is emulated once, below
CASE_PLAN = [(cid, plan) for cid in SMALL for plan in Q.PLANS] + [("V4", "K0")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, plan):
    c = C.make_case(cid)
    return Q.reference(c["x"], Q.make_mask(cid, plan), c["shards"], c["anchor"], Q.temperatures(cid), Q.weights(cid), C.score_errors(cid))


def _ratios(cid, plan, mutation=None, bf16=False):
    c = C.make_case(cid)
    ref, bnd = _want(cid, plan)
    out = Q.emulate(c["x"], Q.make_mask(cid, plan), c["shards"], c["anchor"], Q.temperatures(cid), Q.weights(cid), mutation=mutation,
                    bf16_out=bf16)
    if not bf16:
        out["dx_all_sum"] = sum(v.double() for v in out["dx_all"])
    return Q.ratios(out, ref, bnd, bf16=bf16)


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aecf_hip.h")).read()
    bound = {s[0] for s in _lib._SYMBOLS}
    for name in NAMES:
        assert getattr(lib, name) is not None and name in bound and name + "(" in header, name


def test_workspace_query_is_the_documented_layout(lib):
    for args in ((300, 300, 192, 3, -1), (1, 257, 128, 8, -1), (1215, 2305, 256, 3, -1), (300, 300, 192, 4, 2), (129, 257, 128, 3, -1)):
        got = lib.aecf_nce_multi_pp_workspace_bytes(*args)
        assert got == Q.workspace_bytes_py(*args) and got > lib.aecf_nce_multi_workspace_bytes(*args), args
    for args in ((300, 300, 96, 3, -1), (300, 300, 192, 9, -1), (300, 300, 192, 3, 3), (301, 300, 192, 3, -1)):
        assert lib.aecf_nce_multi_pp_workspace_bytes(*args) == 0, args


def test_refusals_in_order(lib):
    """sizes, then the shape support, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, f = 300, 192, lib.aecf_nce_multi_pp_workspace_bytes(300, 300, 192, 3, -1)
    pc = lambda cols=n, views=3, anchor=-1, pa=None, w=None, out=BAD: lib.aecf_nce_multi_pp_pair_coef(cols, views, anchor, pa, w, out, None)
    assert pc(cols=0) == BAD_DIMS and pc(cols=2 ** 31) == BAD_DIMS and pc(views=1, out=None) == BAD_DIMS and pc(views=9) == BAD_DIMS
    assert pc(anchor=3, out=None) == BAD_DIMS and pc(anchor=-2) == BAD_DIMS
    assert pc(out=None) == NULL_POINTER and pc(pa=BAD, w=BAD, out=None) == NULL_POINTER
    p1 = lambda rows=n, cols=n, dd=d, views=3, anchor=-1, t=BAD, mt=0.025, xl=BAD, xa=BAD, pl=BAD, pa=BAD, ws=BAD, wsb=f, cs=BAD: \
        lib.aecf_nce_multi_pp_pass1(rows, cols, dd, views, anchor, t, mt, xl, xa, pl, pa, 1, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS and p1(rows=n + 1, t=None) == BAD_DIMS
    assert p1(views=1, dd=96) == BAD_DIMS and p1(views=9) == BAD_DIMS and p1(anchor=3, xa=None) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED and p1(dd=4160, t=None) == UNSUPPORTED
    for name in ("t", "xl", "xa", "ws", "cs", "pl", "pa"):      # the presence bytes: both or neither
        assert p1(wsb=0, **{name: None}) == NULL_POINTER, name
    assert p1(wsb=f - 1) == WORKSPACE and p1(wsb=f - 1, pl=None, pa=None) == WORKSPACE
    assert p1(wsb=lib.aecf_nce_multi_workspace_bytes(300, 300, 192, 3, -1)) == WORKSPACE          # the one-temperature size is too small
    ls = lambda rows=n, off=0, dd=d, views=3, t=BAD, xl=BAD, xa=BAD, pl=BAD, pa=BAD, cs=BAD, ws=BAD, wsb=f, lr=BAD: \
        lib.aecf_nce_multi_pp_loss(rows, n, off, dd, views, -1, t, 0.025, xl, xa, pl, pa, cs, ws, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(off=1) == BAD_DIMS and ls(off=-1, dd=96) == BAD_DIMS and ls(views=9, t=None) == BAD_DIMS
    assert ls(dd=96, xa=None) == UNSUPPORTED
    for name in ("t", "xl", "xa", "cs", "ws", "lr", "pl", "pa"):
        assert ls(wsb=0, **{name: None}) == NULL_POINTER, name
    assert ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, off=0, dd=d, anchor=-1, gdt=_lib.AECF_F32, t=BAD, pcf=BAD, xl=BAD, xa=BAD, pl=None, ws=BAD, wsb=f, up=None, o1=BAD, \
        o2=BAD, dtp=None: lib.aecf_nce_multi_pp_grads(rows, n, off, dd, 3, anchor, t, 0.025, pcf, xl, xa, pl, ws, wsb, up, gdt, o1, o2, dtp,
                                                      None)
    assert gr(rows=-1) == BAD_DIMS and gr(off=1, o1=None) == BAD_DIMS and gr(anchor=3, dd=96) == BAD_DIMS
    assert gr(dd=96, pcf=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, t=None) == UNSUPPORTED
    for name in ("t", "pcf", "xl", "xa", "ws", "o1", "o2"):
        assert gr(wsb=0, **{name: None}) == NULL_POINTER, name
    assert gr(wsb=f - 1) == WORKSPACE and gr(wsb=f - 1, pl=BAD, up=BAD, dtp=BAD) == WORKSPACE


def test_python_argument_checks():
    """the per-pair arguments are judged by their form before a device is asked for: the embeddings here live on the CPU"""
    from aecf_amd import losses
    x = torch.zeros(8, 4, 64, dtype=torch.bfloat16)
    order = str(losses.multiview_pairs(4, None))
    for bad in (torch.full((5,), 0.07), torch.full((2, 2), 0.07), torch.full((7,), 0.07)):
        with pytest.raises(ValueError, match="P = 6") as e:
            losses.multiview_info_nce(x, temperature=bad)
        assert order in str(e.value)
    with pytest.raises(ValueError, match="P = 3") as e:
        losses.multiview_info_nce(x, temperature=torch.full((6,), 0.07), anchor=1)
    assert str(losses.multiview_pairs(4, 1)) in str(e.value)
    with pytest.raises(ValueError, match="P = 6"):
        losses.multiview_info_nce(x, temperature=[0.07] * 5)
    with pytest.raises(TypeError, match="float32"):
        losses.multiview_info_nce(x, temperature=torch.full((6,), 0.07, dtype=torch.float64))
    with pytest.raises(ValueError, match="lives on"):
        losses.multiview_info_nce(x, temperature=torch.empty(6, device="meta"))
    for bad in ([1.0, 1.0, -0.5, 1.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0, float("inf")]):
        with pytest.raises(ValueError, match="non-negative and finite"):
            losses.multiview_info_nce(x, pair_weights=bad)
    with pytest.raises(ValueError, match="P = 6"):
        losses.multiview_info_nce(x, pair_weights=[1.0] * 4)
    with pytest.raises(ValueError, match="P = 6"):
        losses.multiview_info_nce(x, pair_weights=torch.ones(5))
    with pytest.raises(ValueError, match="pair_weights live on"):
        losses.multiview_info_nce(x, pair_weights=torch.empty(6, device="meta"))
    with pytest.raises(TypeError, match="float32"):
        losses.multiview_info_nce(x, pair_weights=torch.ones(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="not differentiable"):
        losses.multiview_info_nce(x, pair_weights=torch.ones(6, requires_grad=True))
    # well-formed per-pair arguments pass these checks: the next one, the device of x, is reached
    for kw in (dict(temperature=[0.07] * 6, pair_weights=[1.0, 0.0, 2.0, 1.0, 1.0, 1.0]), dict(temperature=torch.full((6,), 0.07)),
               dict(temperature=torch.full((2, 3), 0.07), pair_weights=torch.ones(6)), dict(pair_weights=[0.0] * 6)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.multiview_info_nce(x, **kw)


def test_cases_are_what_they_claim():
    for cid in Q.CASES:
        c = C.make_case(cid)
        P = Q.n_pairs(cid)
        t, w = Q.temperatures(cid), Q.weights(cid)
        assert len(t) == len(w) == P and len(set(t)) == P and len(set(w)) == P
        assert t[-1] < Q.MIN_T and sum(v < Q.MIN_T for v in t) == 1 and t[0] == Q.f32(0.025) and abs(max(t) - 0.5) < 1e-6
        assert w[0] == 0.0 and all(v > 0 for v in w[1:])
        cnt, live = Q.K.pair_counts(Q.make_mask(cid, "KE"), c["anchor"])
        assert cnt[-1] == 0 and live == P - 1 and all(v > 0 for v in cnt[:-1])
        assert Q.pair_coefs(Q.make_mask(cid, "KE"), c["anchor"], w)[-1] == 0.0
    da, _ = C.roles(4, 2)
    assert da[0] == [(0, 2)]            # V3A: view 0 holds pair 0 alone


@pytest.mark.parametrize("cid,plan", [("V2", "K0"), ("V2", "KE"), ("V3A", "K2")])
def test_the_closed_forms_are_the_float64_autograd_of_the_definition(cid, plan):
    """x.grad = dx_loc + the shards' dx_all, temperature.grad = the shards' dT added up, the value; the clamped entry and the pair
    of weight 0 get exact zeros"""
    c = C.make_case(cid)
    absent = Q.make_mask(cid, plan)
    ref, _ = _want(cid, plan)
    x64 = c["x"].double().requires_grad_(True)
    t64 = torch.tensor(Q.temperatures(cid), dtype=torch.float64, requires_grad=True)
    loss = Q.definition(x64, absent, c["anchor"], t64, Q.weights(cid))
    loss.backward()
    gx = ref["dx_loc"] + ref["dx_all_sum"]
    assert float((x64.grad - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
    assert float((t64.grad - ref["dT_sum"]).abs().max()) <= 1e-10 * float(ref["dT_sum"].abs().max())
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    P = Q.n_pairs(cid)
    assert float(t64.grad[P - 1]) == 0.0 and float(ref["dT_sum"][P - 1]) == 0.0 and float(ref["dT_sum"][0]) == 0.0
    assert int((ref["dT_sum"] != 0).sum()) == P - 2


@pytest.mark.parametrize("cid,plan", CASE_PLAN)
def test_emulation_stays_inside_the_bounds(cid, plan):
    for bf16 in (False, True):
        r = _ratios(cid, plan, bf16=bf16)
        print(f"multiview_pairwise_emulation case {cid} plan {plan} {'bf16' if bf16 else 'f32'}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
        for name, v in r.items():
            assert v <= 1.0, (cid, plan, bf16, name, v)


# (mutation, case, plan, the output that leaves its bounds, the factor it must leave them by: about a tenth of what this emulation
# gives -- 4.1e5, 4.1e5, 3.6e4, 137, 145 and 1.2e7 bounds)
TEETH = [
    ("T_pair0", "V2", "K0", "loss_rows", 1e4),
    ("T_by_view", "V2", "K0", "loss_rows", 1e4),
    ("dT_per_view", "V2", "K0", "dT", 1e3),
    ("w_unnormalised", "V2", "K0", "dx_loc", 30.0),
    ("w_norm_all", "V2", "KE", "dx_all", 30.0),
    ("c_local", "V2", "K0", "dT", 1e5),
]


@pytest.mark.parametrize("mutation,cid,plan,output,factor", TEETH)
def test_the_bounds_have_teeth(mutation, cid, plan, output, factor):
    r = _ratios(cid, plan, mutation=mutation)
    print(f"multiview_pairwise_teeth {mutation} case {cid} plan {plan}: " + " ".join(f"{n}={v:.3g}" for n, v in r.items()))
    assert r[output] > factor, (mutation, output, r[output])
    clean = _ratios(cid, plan)
    assert all(v <= 1.0 for v in clean.values())
