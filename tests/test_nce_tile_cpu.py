"""CPU-only tests of what tests/test_nce_tile_gpu.py stands on (tests/nce_tile_cases.py): the Python mirror of the tile forms'
geometry agrees with the library's workspace entry points (host code), every case has the geometry its row of the table
claims, the twins carry enough softmax weight at both temperatures, and the derived bounds have teeth -- an emulation of the
design's arithmetic stays inside them, the same emulation with one key or row lost or counted twice, or with the positive's
weight taken from the bf16 exponential, leaves them by a factor of ten at least.  The refusals of the aecf_nce_sym_* entry
points (order and codes, a workspace one byte short included) are host code too: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
ALL_IDS = list(C.DIRECTION) + list(C.SYMMETRIC)
SMALL_IDS = list(C.SMALL_DIRECTION + C.SMALL_SYMMETRIC)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _shapes(cid):
    """[(rows, cols, off, d)] of every call a case makes"""
    if cid in C.DIRECTION:
        return [C.DIRECTION[cid][0]]
    (n, d), shards, _, _ = C.SYMMETRIC[cid]
    return [(hi - lo, n, lo, d) for lo, hi in shards]


@functools.lru_cache(maxsize=None)
def _want(cid, T):
    c = C.make_case(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(c["a"], c["b"], c["off"], c["shards"], t, c["coef"], c["sym"], C.score_error(cid), keep=True)
    return t, ref, bnd


@functools.lru_cache(maxsize=None)
def _state(cid, T):
    c = C.make_case(cid)
    return C.emulate_pass1(c["a"], c["b"], c["shards"], C.used_temperature(T))


def test_workspace_bytes_match_the_mirror(lib):
    for cid in ALL_IDS:
        for rows, cols, _, d in _shapes(cid):
            want = C.workspace_bytes_py(rows, cols, d)
            assert lib.aecf_nce_sym_workspace_bytes(rows, cols, d) == want, (cid, rows)
            # aecf_nce_workspace_bytes answers the largest form: the tile term where no streaming kernel exists for d
            whole = lib.aecf_nce_workspace_bytes(rows, cols, d, _lib.AECF_BF16)
            stream = lib.aecf_nce_stream_workspace_bytes(rows, cols, d, _lib.AECF_BF16)
            assert whole == max(want, stream), (cid, rows)
    assert lib.aecf_nce_sym_workspace_bytes(300, 300, 100) == 0 and lib.aecf_nce_sym_workspace_bytes(0, 300, 128) == 0


def test_da_split_windows_named_by_the_issue():
    """one row tile, d <= 256: 13 splits of which 12 are live for 6657 <= cols <= 6912; 21 / 20 with a one-step last live split
    for 10753 <= cols <= 11008"""
    for cols in (6657, 6700, 6912):
        g = C.geometry(200, cols, 256)
        assert (g["splits"], g["live"]) == (13, 12)
    for cols in (10753, 10900, 11008):
        g = C.geometry(65, cols, 64)
        assert (g["splits"], g["live"], g["last"]) == (21, 20, 1)
    assert C.geometry(200, 6656, 256)["live"] == C.geometry(200, 6656, 256)["splits"]
    assert C.geometry(200, 6913, 256)["live"] == C.geometry(200, 6913, 256)["splits"]


@pytest.mark.parametrize("cid", ALL_IDS)
def test_case_has_the_geometry_it_claims(cid):
    claims = [C.DIRECTION[cid][1]] if cid in C.DIRECTION else C.SYMMETRIC[cid][2]
    shapes = _shapes(cid)
    assert len(claims) == len(shapes)
    for (rows, cols, off, d), claim in zip(shapes, claims):
        g = C.geometry(rows, cols, d)
        assert {k: g[k] for k in claim} == claim, (cid, rows)
        assert 0 <= off and off + rows <= cols and d % 64 == 0
        assert (g["live"] - 1) * g["per"] < g["Cp"] // 64 <= g["live"] * g["per"] and g["live"] <= g["splits"] <= 32
        # the tdot partials of the _dt path fit where pass 1 kept its row-sum partials
        assert g["splits"] * g["m_tiles"] * g["d_tiles"] <= g["n_tiles"] * g["Rp"]
    geoms = [C.geometry(r, c_, d) for r, c_, _, d in shapes]
    extra = {
        "D1": lambda: shapes[0][:2] == (1, 1),
        "D2": lambda: shapes[0][2] + shapes[0][0] == shapes[0][1] and geoms[0]["live"] < geoms[0]["splits"],
        "D3": lambda: geoms[0]["last"] == 1 and geoms[0]["live"] == geoms[0]["splits"] - 1,
        "D4": lambda: geoms[0]["map"] == "SPLITX" and geoms[0]["d_last"] < 256,
        "D5": lambda: shapes[0][0] == 256 + 1 and shapes[0][1] == 512 + 1 and geoms[0]["d_last"] == 64,
        "D6": lambda: geoms[0]["m_tiles"] > 4 and geoms[0]["n_tiles"] > 8 and geoms[0]["splits"] == 4,
        "S1": lambda: True,
        "S2": lambda: shapes[1][0] == 1 and shapes[1][2] == 256,
        "S3": lambda: geoms[0]["splits"] == 1,
        "S4": lambda: sorted(s[0] for s in shapes) == [65, 1025, 1215] and all(g["n_tiles"] == 10 for g in geoms),
        "S5": lambda: all(g["map"] == "SPLITX" for g in geoms) and geoms[1]["m_tiles"] == 16,
        "S6": lambda: all((g["splits"], g["live"]) == (13, 12) for g in geoms) and geoms[1]["da_units"] % 8 != 0,
    }
    assert extra[cid]()
    c = C.make_case(cid)
    a, b, twins = c["a"], c["b"], c["twins"]
    assert max(float((z.double().norm(dim=1) - 1).abs().max()) for z in (a, b)) < 2.0 ** -7       # unit rows, rounded to bf16
    assert len({x for x, _ in twins}) == len(twins) == len({r for _, r in twins})
    if cid in C.DIRECTION:
        rows, cols, off, d = shapes[0]
        named = [j for j in C.boundary_columns(cols, geoms) if not (off <= j < off + rows)]
        assert [j for j, _ in twins] == named and len(named) <= rows, cid          # every boundary column got its twin
        for j, r in twins:
            assert bool((b[j] == b[off + r]).all())
        assert len(twins) == dict(D1=0, D2=29, D3=44, D4=20, D5=3, D6=9)[cid]
    else:
        n = a.shape[0]
        spots = {r for r in C.ROW_EDGES + (n - 1,) if r < n} | {x for lo, hi in c["shards"] for x in (lo, hi - 1)}
        spots |= set(C.boundary_columns(n, geoms))
        if n > 1:
            assert {rp for rp, _ in twins} == spots, cid
        assert not ({r for _, r in twins} & spots)
        for rp, r in twins:
            assert bool((a[rp] == a[r]).all()) and bool((b[rp] == b[r]).all())


@pytest.mark.parametrize("cid", SMALL_IDS)
def test_twins_hold_a_quarter_of_their_softmax(cid):
    c = C.make_case(cid)
    off = c["off"]
    for T in C.TEMPS:
        ref = _want(cid, T)[1]
        for x, r in c["twins"]:
            if c["sym"]:
                # rows r and r' (= x) are one vector: each of them holds the same share of either's row and of either's column
                in_row = [ref["P_row"][r, x], ref["P_row"][r, r], ref["P_row"][x, x], ref["P_row"][x, r]]
                in_col = [ref["P_col"][r, x], ref["P_col"][x, x], ref["P_col"][x, r], ref["P_col"][r, r]]
            else:
                in_row, in_col = [ref["P_row"][r, x], ref["P_row"][r, off + r]], []
            for shares in (in_row, in_col):
                shares = [float(s) for s in shares]
                assert not shares or (min(shares) >= 0.25 and max(shares) - min(shares) <= 1e-9), (cid, T, x, r, shares)


@pytest.mark.parametrize("cid", SMALL_IDS)
def test_bounds_hold_the_emulation(cid):
    c = C.make_case(cid)
    for T in C.TEMPS:
        t, ref, bnd = _want(cid, T)
        got = C.emulate(c["a"], c["b"], c["off"], c["shards"], t, c["coef"], c["sym"], state=_state(cid, T))
        got["db_sum"] = sum(g.double() for g in got["db"])
        if not c["sym"]:
            del got["colsum"]                   # (a direction neither returns nor uses them)
        r = C.ratios(got, ref, bnd)
        sig = C.signal(ref, bnd)
        print(f"nce tile emulation {cid} T={T}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
              + " | value/bound " + " ".join(f"{n}={v:.3g}" for n, v in sig.items() if n in r))
        assert all(v <= 1.0 for v in r.values()), (cid, T, r)
        # an upstream scalar scales reference and bounds alike; bf16 outputs add 2^-8 |value|
        if cid in ("S3", "D5"):
            up = 0.375
            ref_u, bnd_u = C.reference(c["a"], c["b"], c["off"], c["shards"], t, c["coef"] * up, c["sym"], C.score_error(cid))
            got = C.emulate(c["a"], c["b"], c["off"], c["shards"], t, c["coef"], c["sym"], state=_state(cid, T), upstream=up)
            got = dict(da=got["da"].to(torch.bfloat16), db=[g.to(torch.bfloat16) for g in got["db"]])
            r = C.ratios(got, ref_u, bnd_u, bf16=True)
            assert all(v <= 1.0 for v in r.values()), (cid, T, r)


@pytest.mark.parametrize("cid", [i for i in SMALL_IDS if i not in ("D1", "S1")])
def test_bounds_catch_a_lost_or_doubled_key_or_row(cid):
    """A key that enters the row sums 0 times or twice and (symmetric) a row that enters the column sums 0 times or twice: the loss
    of the twin's partner row, and for a row its shard's column sums, leave their bounds tenfold at least."""
    c = C.make_case(cid)
    off = c["off"]
    for T in C.TEMPS:
        t, ref, bnd = _want(cid, T)
        worst = {}
        for x, r in c["twins"]:
            for kind in (("col", "row") if c["sym"] else ("col",)):
                for times in (0, 2):
                    bad = C.emulate(c["a"], c["b"], off, c["shards"], t, c["coef"], c["sym"], mutation=(kind, x, times), grads=False,
                                    state=_state(cid, T))
                    over = abs(float(bad["loss_rows"][r]) - float(ref["loss_rows"][r])) / float(bnd["loss_rows"][r])
                    if kind == "row":
                        over = min(over, C.ratios(dict(colsum=bad["colsum"]), ref, bnd)["colsum"])
                    worst[kind, times] = min(worst.get((kind, times), float("inf")), over)
                    assert over >= 10.0, (cid, T, kind, x, r, times, over)
        print(f"nce tile mutations {cid} T={T}: smallest excess " + " ".join(f"{k}x{t_}={v:.0f}" for (k, t_), v in worst.items()))


@pytest.mark.parametrize("cid", ["D5", "S2", "S3"])
def test_bounds_catch_a_positive_weight_taken_from_bf16(cid):
    """The ediag mutation at T = 0.07, judged on the positive's rows of da and db where the positive dominates: the rows without a
    twin, in the cases of a few hundred keys (module docstring of nce_tile_cases: with thousands of keys the derivation gives
    less than ten bounds, D4 and S4 reach 4 to 9).  The intact emulation is inside the same bounds on the same rows
    (test_bounds_hold_the_emulation)."""
    c = C.make_case(cid)
    off, T = c["off"], 0.07
    t, ref, bnd = _want(cid, T)
    bad = C.emulate(c["a"], c["b"], off, c["shards"], t, c["coef"], c["sym"], mutation=("ediag",), state=_state(cid, T))
    twin_rows = {r for _, r in c["twins"]} | ({x for x, _ in c["twins"]} if c["sym"] else set())
    plain = torch.tensor([r for r in range(c["a"].shape[0]) if r not in twin_rows])
    over_da = float(((bad["da"].double() - ref["da"]).abs() / bnd["da"])[plain].max())
    over_db = 0.0
    for (lo, hi), got, want, b in zip(c["shards"], bad["db"], ref["db"], bnd["db"]):
        sel = plain[(plain >= lo) & (plain < hi)] + off
        if sel.numel():
            over_db = max(over_db, float(((got.double() - want).abs() / b)[sel].max()))
    print(f"nce tile mutations {cid} T={T}: ediag da {over_da:.0f}x db {over_db:.0f}x")
    assert over_da >= 10.0 and over_db >= 10.0, (cid, over_da, over_db)


# ---- refusals of the sym entry points: order and codes ----
def _pass1(lib, dt, rows=300, cols=300, d=192, T=0.07, a=BAD, b=BAD, ws=BAD, short=0, cs=BAD, temp=BAD):
    wsb = lib.aecf_nce_sym_workspace_bytes(rows, cols, d if d > 0 and d % 64 == 0 else 64) - short
    if dt:
        return lib.aecf_nce_sym_pass1_dt(rows, cols, d, temp, T, a, b, ws, wsb, cs, None)
    return lib.aecf_nce_sym_pass1(rows, cols, d, T, a, b, ws, wsb, cs, None)


def _loss(lib, dt, rows=300, cols=300, off=0, d=192, T=0.07, a=BAD, b=BAD, cs=BAD, ws=BAD, short=0, lr=BAD, n_ent=0, ent=None,
          e_loss=None, temp=BAD):
    wsb = lib.aecf_nce_sym_workspace_bytes(rows, cols, d if d > 0 and d % 64 == 0 else 64) - short
    if dt:
        return lib.aecf_nce_sym_loss_dt(rows, cols, off, d, temp, T, a, b, cs, ws, wsb, lr, n_ent, 2, 0.7, ent, 1.0, e_loss, None, None)
    return lib.aecf_nce_sym_loss(rows, cols, off, d, T, a, b, cs, ws, wsb, lr, n_ent, 2, 0.7, ent, 1.0, e_loss, None, None)


def _grads(lib, dt, rows=300, cols=300, off=0, d=192, T=0.07, a=BAD, b=BAD, ws=BAD, short=0, gdt=_lib.AECF_BF16, da=BAD, db=BAD,
           temp=BAD):
    wsb = lib.aecf_nce_sym_workspace_bytes(rows, cols, d if d > 0 and d % 64 == 0 else 64) - short
    if dt:
        return lib.aecf_nce_sym_grads_dt(rows, cols, off, d, temp, T, 0.001, a, b, ws, wsb, None, gdt, da, db, None, None)
    return lib.aecf_nce_sym_grads(rows, cols, off, d, T, 0.001, a, b, ws, wsb, None, gdt, da, db, None)


@pytest.mark.parametrize("dt", [False, True])
def test_sym_entry_points_refuse_in_order(lib, dt):
    """sizes -> what is not built (d, the temperature bound, the gradient dtype) -> NULL pointers -> the workspace, each before
    the next: a call wrong in two ways reports the earlier one, and nothing is launched (the pointers are bogus)."""
    for call in (_pass1, _loss, _grads):
        assert call(lib, dt, short=1) == WORKSPACE                                   # one byte short, all else valid
        assert call(lib, dt, rows=0, d=100) == BAD_DIMS and call(lib, dt, cols=0, a=None) == BAD_DIMS
        assert call(lib, dt, d=0) == BAD_DIMS and call(lib, dt, T=0.0, d=100) == BAD_DIMS
        assert call(lib, dt, T=float("nan") if dt else -1.0) == BAD_DIMS
        assert call(lib, dt, d=100, a=None) == UNSUPPORTED and call(lib, dt, d=4160, short=1) == UNSUPPORTED
        assert call(lib, dt, T=0.02, b=None, short=1) == UNSUPPORTED                 # the tile forms' bound, before pointers
        assert call(lib, dt, a=None, short=1) == NULL_POINTER and call(lib, dt, b=None) == NULL_POINTER
        assert call(lib, dt, ws=None, short=1) == NULL_POINTER
        if dt:
            assert call(lib, dt, temp=None, short=1) == NULL_POINTER and call(lib, dt, temp=None, d=100) == UNSUPPORTED
    # pass 1: more local rows than keys; its column sums are required
    assert _pass1(lib, dt, rows=301, d=100) == BAD_DIMS and _pass1(lib, dt, cs=None, short=1) == NULL_POINTER
    for call in (_loss, _grads):
        assert call(lib, dt, off=-1, d=100) == BAD_DIMS and call(lib, dt, rows=200, off=101, a=None) == BAD_DIMS
        assert call(lib, dt, rows=200, off=100, short=1) == WORKSPACE                # off + rows == cols is the last valid offset
    assert _loss(lib, dt, n_ent=-1, d=100) == BAD_DIMS
    assert _loss(lib, dt, cs=None, short=1) == NULL_POINTER and _loss(lib, dt, lr=None, short=1) == NULL_POINTER
    assert _loss(lib, dt, n_ent=5, ent=None, e_loss=BAD, short=1) == NULL_POINTER
    assert _loss(lib, dt, n_ent=5, ent=BAD, e_loss=None, short=1) == NULL_POINTER
    assert _loss(lib, dt, n_ent=5, ent=BAD, e_loss=BAD, short=1) == WORKSPACE
    assert _loss(lib, dt, n_ent=0, ent=None, e_loss=None, short=1) == WORKSPACE
    assert _grads(lib, dt, gdt=_lib.AECF_F16, a=None) == UNSUPPORTED and _grads(lib, dt, gdt=_lib.AECF_F16, rows=0) == BAD_DIMS
    assert _grads(lib, dt, gdt=_lib.AECF_F32, short=1) == WORKSPACE
    assert _grads(lib, dt, da=None, short=1) == NULL_POINTER and _grads(lib, dt, db=None, short=1) == NULL_POINTER


def test_fwd_bwd_takes_the_tile_form_only_with_its_workspace(lib):
    """aecf_nce_fwd_bwd[_dt] at a width with no streaming kernel (d = 192): with the tile workspace one byte short the tile form
    is not taken and no other form exists for ragged cols -- refused as unsupported, nothing launched"""
    rows, cols, off, d = C.DIRECTION["D4"][0]
    wsb = lib.aecf_nce_sym_workspace_bytes(rows, cols, d)
    assert lib.aecf_nce_stream_workspace_bytes(rows, cols, d, _lib.AECF_BF16) == 0
    assert lib.aecf_nce_fwd_bwd(rows, cols, off, d, _lib.AECF_BF16, 0.07, 1.0 / cols, BAD, BAD, BAD, BAD, BAD, BAD, wsb - 1,
                                None) == UNSUPPORTED
    assert lib.aecf_nce_fwd_bwd_dt(rows, cols, off, d, _lib.AECF_BF16, BAD, 0.025, 1.0 / cols, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
                                   wsb - 1, None) == UNSUPPORTED
