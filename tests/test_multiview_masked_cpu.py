"""CPU-only tests of what tests/test_multiview_masked_gpu.py stands on (tests/multiview_masked_cases.py): the entry points of
multi-view InfoNCE with missing views load and refuse in their documented order; the Python surface checks the mask; the float64
reference by masking equals the float64 autograd of the compacted formulation; with every view present the reference is the
unmasked one; an emulation of the design's arithmetic stays inside the derived bounds on every case, plan and temperature; and
the bounds have teeth -- the emulation with one broken masking rule leaves them on a named output of a named case and plan.  The
refusals are host code: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import multiview_cases as C
from tests import multiview_masked_cases as K
from tests import nce_tile_cases as N

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_nce_multi_masked_workspace_bytes", "aecf_nce_multi_masked_pair_coef", "aecf_nce_multi_masked_pass1",
         "aecf_nce_multi_masked_loss", "aecf_nce_multi_masked_grads", "aecf_l2norm_masked_forward", "aecf_l2norm_masked_backward")
INF = float("inf")
CASE_PLAN_T = [(cid, plan, T) for cid in K.CASES for plan in K.PLANS for T in K.TEMPS]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, plan, T):
    c = C.make_case(cid)
    t = N.used_temperature(T)
    ref, bnd = K.reference(c["x"], K.make_mask(cid, plan), c["shards"], c["anchor"], t, C.score_errors(cid))
    return t, ref, bnd


def _ratios(cid, plan, T, mutation=None, bf16=False):
    c = C.make_case(cid)
    t, ref, bnd = _want(cid, plan, T)
    out = K.emulate(c["x"], K.make_mask(cid, plan), c["shards"], c["anchor"], t, mutation=mutation, bf16_out=bf16)
    if not bf16:
        out["dx_all_sum"] = sum(v.double() for v in out["dx_all"])
    return K.ratios(out, ref, bnd, bf16=bf16)


def test_symbols_are_declared_bound_and_exported(lib):
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aecf_hip.h")).read()
    bound = {s[0] for s in _lib._SYMBOLS}
    for name in NAMES:
        assert getattr(lib, name) is not None and name in bound and name + "(" in header, name


def test_workspace_query_is_the_unmasked_one(lib):
    for args in ((300, 300, 192, 3, -1), (1, 257, 128, 8, -1), (1215, 2305, 256, 3, -1), (300, 300, 192, 4, 2)):
        assert lib.aecf_nce_multi_masked_workspace_bytes(*args) == lib.aecf_nce_multi_workspace_bytes(*args) > 0
    for args in ((64, 64, 96, 3, -1), (65, 64, 64, 3, -1), (64, 64, 64, 9, -1), (64, 64, 64, 3, 3)):
        assert lib.aecf_nce_multi_masked_workspace_bytes(*args) == 0


def test_refusals_in_order(lib):
    """sizes, then the shape support, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, f = 300, 192, lib.aecf_nce_multi_masked_workspace_bytes(300, 300, 192, 3, -1)
    pc = lambda cols=n, views=3, anchor=-1, pa=BAD, out=BAD: lib.aecf_nce_multi_masked_pair_coef(cols, views, anchor, pa, out, None)
    assert pc(cols=0) == BAD_DIMS and pc(cols=2 ** 31) == BAD_DIMS and pc(views=1, pa=None) == BAD_DIMS and pc(views=9) == BAD_DIMS
    assert pc(anchor=3, out=None) == BAD_DIMS and pc(anchor=-2) == BAD_DIMS
    assert pc(pa=None) == NULL_POINTER and pc(out=None) == NULL_POINTER
    p1 = lambda rows=n, cols=n, dd=d, views=3, anchor=-1, t=BAD, mt=0.025, xl=BAD, xa=BAD, pl=BAD, pa=BAD, ws=BAD, wsb=f, cs=BAD: \
        lib.aecf_nce_multi_masked_pass1(rows, cols, dd, views, anchor, t, mt, xl, xa, pl, pa, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS and p1(rows=n + 1, pl=None) == BAD_DIMS
    assert p1(views=1, dd=96) == BAD_DIMS and p1(views=9) == BAD_DIMS and p1(anchor=3, pa=None) == BAD_DIMS
    assert p1(dd=96, pl=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED and p1(dd=4160, t=None) == UNSUPPORTED
    for name in ("t", "xl", "xa", "pl", "pa", "ws", "cs"):
        assert p1(wsb=0, **{name: None}) == NULL_POINTER, name
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, off=0, dd=d, views=3, t=BAD, xl=BAD, xa=BAD, pl=BAD, pa=BAD, cs=BAD, ws=BAD, wsb=f, lr=BAD: \
        lib.aecf_nce_multi_masked_loss(rows, n, off, dd, views, -1, t, 0.025, xl, xa, pl, pa, cs, ws, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(off=1) == BAD_DIMS and ls(off=-1, dd=96) == BAD_DIMS and ls(views=9, pl=None) == BAD_DIMS
    assert ls(dd=96, pa=None) == UNSUPPORTED
    for name in ("t", "xl", "xa", "pl", "pa", "cs", "ws", "lr"):
        assert ls(wsb=0, **{name: None}) == NULL_POINTER, name
    assert ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, off=0, dd=d, anchor=-1, gdt=_lib.AECF_F32, t=BAD, pcf=BAD, xl=BAD, xa=BAD, pl=BAD, ws=BAD, wsb=f, up=None, o1=BAD, \
        o2=BAD, dtp=None: lib.aecf_nce_multi_masked_grads(rows, n, off, dd, 3, anchor, t, 0.025, pcf, xl, xa, pl, ws, wsb, up, gdt, o1, o2,
                                                          dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(off=1, o1=None) == BAD_DIMS and gr(anchor=3, dd=96) == BAD_DIMS
    assert gr(dd=96, pcf=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, pl=None) == UNSUPPORTED
    for name in ("t", "pcf", "xl", "xa", "pl", "ws", "o1", "o2"):
        assert gr(wsb=0, **{name: None}) == NULL_POINTER, name
    assert gr(wsb=f - 1) == WORKSPACE                                    # (upstream and d_temperature may be NULL)
    nf = lambda rows=12, dd=64, views=3, dt=_lib.AECF_BF16, z=BAD, mk=BAD, zn=BAD, inv=BAD, pr=None: \
        lib.aecf_l2norm_masked_forward(rows, dd, views, dt, 1e-12, z, mk, zn, inv, pr, None)
    assert nf(rows=0) == BAD_DIMS and nf(dd=0) == BAD_DIMS and nf(views=0) == BAD_DIMS and nf(views=9, z=None) == BAD_DIMS
    assert nf(rows=13) == BAD_DIMS                                       # n % views
    assert nf(dt=_lib.AECF_F16, z=None) == UNSUPPORTED
    for name in ("z", "mk", "zn", "inv"):
        assert nf(**{name: None}) == NULL_POINTER, name                  # (presence may be NULL)
    nb = lambda rows=12, dd=64, dt=_lib.AECF_BF16, zn=BAD, inv=BAD, g=BAD, mk=BAD, dz=BAD: \
        lib.aecf_l2norm_masked_backward(rows, dd, dt, zn, inv, g, mk, dz, None)
    assert nb(rows=0) == BAD_DIMS and nb(dt=_lib.AECF_F16, zn=None) == UNSUPPORTED
    for name in ("zn", "inv", "g", "mk", "dz"):
        assert nb(**{name: None}) == NULL_POINTER, name


def test_python_mask_checks():
    """shape, dtype and device of the mask, checked like the function's other arguments, before anything runs"""
    import inspect
    from aecf_amd import losses
    assert list(inspect.signature(losses.multiview_info_nce).parameters)[-1] == "key_padding_mask"
    z = torch.zeros(4, 3, 128, dtype=torch.bfloat16)
    ok = torch.zeros(4, 3, dtype=torch.bool)
    for mask in (ok, ok.to(torch.uint8)):               # a good mask: the next check, the device of x, is reached
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.multiview_info_nce(z, key_padding_mask=mask)
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.multiview_info_nce([z[:, 0], z[:, 1], z[:, 2]], key_padding_mask=mask)
    for bad in (ok[:3], ok[:, :2], ok[0], ok[None], ok.T, [[False] * 3] * 4, "mask"):
        with pytest.raises(ValueError, match=r"key_padding_mask must be a \[b, M\] = \[4, 3\] tensor"):
            losses.multiview_info_nce(z, key_padding_mask=bad)
    for dt in (torch.int64, torch.float32, torch.int8, torch.bfloat16):
        with pytest.raises(TypeError, match="key_padding_mask must be bool or uint8"):
            losses.multiview_info_nce(z, key_padding_mask=ok.to(dt))
    with pytest.raises(ValueError, match="key_padding_mask lives on meta, the embeddings on cpu"):
        losses.multiview_info_nce(z, key_padding_mask=torch.zeros(4, 3, dtype=torch.bool, device="meta"))


def test_mask_plans_are_what_they_claim():
    for cid in K.CASES:
        c = C.make_case(cid)
        n, M, _ = c["x"].shape
        pr = C.pairs(M, c["anchor"])
        assert not K.make_mask(cid, "K0").any()
        k1 = K.make_mask(cid, "K1")
        assert k1[0].all() and (~k1[1]).sum() == 1 and 0.6 < float((~k1).float().mean()) < 0.8
        k2 = K.make_mask(cid, "K2")
        assert k2[:256, 1].all() and not k2[256:].any() and not k2[:, 0].any()
        cnt, live = K.pair_counts(K.make_mask(cid, "K3"), c["anchor"])
        assert cnt[0] == 0 and live == len(pr) - 1 and all(v > 0 for v in cnt[1:])
        cnt, live = K.pair_counts(K.make_mask(cid, "K4"), c["anchor"])
        assert cnt[0] == 1 and live == len(pr)
        k5 = K.make_mask(cid, "K5")
        tw = {rp for rp, _ in c["twins"]}
        assert int(k5.sum()) >= 1 and not k5[:, [v for v in range(M) if v != pr[0][1]]].any()
        assert all(int(g) in tw for g in torch.nonzero(k5[:, pr[0][1]]).flatten())
        assert K.presence_bytes(k1).dtype == torch.uint8 and int(K.presence_bytes(k1)[0]) == 0 and int(K.presence_bytes(k1)[1]) == 1
    for cid in K.SHARDED:                               # the shards of K1, K2 and K5 see different masks
        c = C.make_case(cid)
        for plan in ("K1", "K2", "K5"):
            a = K.make_mask(cid, plan)
            parts = [a[lo:hi] for lo, hi in c["shards"]]
            assert any(not torch.equal(parts[0][:min(len(parts[0]), len(q))], q[:min(len(parts[0]), len(q))]) for q in parts[1:]), (cid, plan)


@pytest.mark.parametrize("plan", K.PLANS)
@pytest.mark.parametrize("cid", ["V2", "V3", "V3A", "V8"])
def test_the_two_float64_formulations_agree(cid, plan):
    """masking (-inf logits outside V_p x V_p, coef_p = 0.5 / n_p / P') against float64 autograd of the mean over the non-empty
    pairs of info_nce on index_select-ed copies: loss, loss rows' weighted sum, the gradient on x and dL/dT, to 1e-12"""
    c = C.make_case(cid)
    T = 0.07
    absent = K.make_mask(cid, plan)
    ref, _ = K.reference(c["x"], absent, c["shards"], c["anchor"], T, C.score_errors(cid))
    x = c["x"].double().requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float64, requires_grad=True)
    loss = K.compacted_loss(x, absent, c["anchor"], t)
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12
    assert float((x.grad - (ref["dx_loc"] + ref["dx_all_sum"])).abs().max()) <= 1e-12
    assert abs(float(t.grad) - sum(ref["dT"])) <= 1e-12
    assert not bool(x.grad[absent].any()) and not bool((ref["dx_loc"] + ref["dx_all_sum"])[absent].any())
    if plan == "K4":
        assert abs(float(ref["loss_rows"][0].sum())) <= 1e-12           # a pair of one row: its loss is 0


def test_with_every_view_present_the_reference_is_the_unmasked_one():
    """values equal; bounds equal but for the one h of pair_coef in eps_w"""
    c = C.make_case("V3")
    t = N.used_temperature(0.07)
    ref0, bnd0 = C.reference(c["x"], c["shards"], c["anchor"], t, c["coef"] / 3, C.score_errors("V3"))
    ref, bnd = K.reference(c["x"], K.make_mask("V3", "K0"), c["shards"], c["anchor"], t, C.score_errors("V3"))
    for name in ("loss_rows", "dx_loc", "dx_all_sum"):
        assert float((ref[name] - ref0[name]).abs().max()) <= 1e-12, name
        assert bool((bnd[name] >= bnd0[name]).all()) and float((bnd[name] / bnd0[name].clamp_min(1e-300)).max()) <= 1.0 + 1e-3, name
    assert abs(ref["dT"][0] - ref0["dT"][0]) <= 1e-12 and bnd0["dT"][0] <= bnd["dT"][0] <= bnd0["dT"][0] * (1.0 + 1e-3)


@pytest.mark.parametrize("cid,plan,T", CASE_PLAN_T)
def test_emulation_stays_inside_the_bounds(cid, plan, T):
    r = _ratios(cid, plan, T)
    print(f"multiview_masked emulation case {cid} plan {plan} T {T}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    for name, v in r.items():
        assert v <= 1.0, (cid, plan, T, name, v)
    rb = _ratios(cid, plan, T, bf16=True)
    for name, v in rb.items():
        assert v <= 1.0, (cid, plan, T, "bf16", name, v)


# (mutation, case, plan, output, the factor by which the emulation left the bound when this test was written)
TEETH = [
    ("keys_kept", "V3", "K5", "loss_rows", 6.08e3),         # the absent twin stays in its partner's row denominator: ln 2
    ("keys_kept", "V2", "K1", "loss_rows", 7.75e3),
    ("rows_only", "V3", "K5", "loss_rows", 6.08e3),
    ("rows_only", "V2", "K2", "colsum", INF),               # an absent column must sum to an exact zero
    ("one_over_b_all", "V3", "K1", "dx_loc", 84.8),
    ("one_over_b_all", "V3", "K2", "dx_all", 107.0),
    ("P_for_P_live", "V3", "K3", "dx_loc", 52.2),
    ("P_for_P_live", "V3A", "K3", "loss", 86.2),
    ("row_mask_global", "V4", "K1", "loss_rows", INF),      # a row taken for present has no key: the log of an empty sum
    ("row_mask_global", "V2", "K2", "dx_loc", INF),
    ("partner_absent", "V3", "K1", "dx_loc", INF),          # -2 ct x_partner at a slot that must hold an exact zero
    ("partner_absent", "V2", "K2", "dx_loc", INF),
]


@pytest.mark.parametrize("mutation,cid,plan,output,factor", TEETH)
def test_the_bounds_have_teeth(mutation, cid, plan, output, factor):
    r = _ratios(cid, plan, 0.07, mutation=mutation)
    print(f"multiview_masked mutation {mutation} case {cid} plan {plan}: " + " ".join(f"{n}={v:.3g}" for n, v in r.items()))
    worst = r[output] if output in r else max(r.values())         # (an output that is not finite is reported alone, as inf)
    assert worst >= 2.0, (mutation, cid, plan, output, r)
    if factor is not None and factor != float("inf"):
        assert worst >= 0.5 * factor, (mutation, cid, plan, output, worst, factor)
