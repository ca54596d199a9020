"""CPU-only tests of what tests/test_sig_tile_gpu.py stands on (tests/sig_tile_cases.py): every case has the geometry its row of
the table claims, the Python mirrors of the workspace size and of EPI_SIG's block-uniform predicate agree with the library (host
code) and with a brute-force statement, the float32 restatement of sig_terms keeps to its share of the bounds across the clamp,
and the derived bounds have teeth -- an emulation of the design's arithmetic stays inside them on every element of every
output, the same emulation with one key lost or doubled, a padded row or column let in, the positive misplaced, a band tile
sent down the plain path, or dbias summed from the rounded g leaves them by a factor of two at least."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import sig_tile_cases as C

IDS = list(C.CASES)
CASE_PARAMS = [(cid, T, bias) for cid in IDS for T, bias in C.PARAMS]
# where the dbias_bf16 mutation is judged (module docstring of sig_tile_cases): at (0.1, -10), where the positives carry the sum of g
TWIN_COUNTS = dict(G1=0, G2=6, G3=7, G4=8, G5=4, G6=29, G7=44, G8=20, G9=11, G10=10, G11=0)
DBIAS_BF16_JUDGED = {(cid, C.PARAMS[0]) for cid in IDS}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, T, bias, upstream=1.0):
    c = C.make_case(cid)
    t, bs = C.used_temperature(T), C.used_temperature(bias)
    ref, bnd = C.reference(c["a"], c["b"], c["off"], t, bs, c["coef"], upstream, C.score_error(cid), keep=True)
    return t, bs, ref, bnd


def _tiles(cid):
    (rows, cols, off, d), _, _ = C.CASES[cid]
    g = C.geometry(rows, cols, d)
    return rows, cols, off, [(mi, ni) for mi in range(g["m_tiles"]) for ni in range(g["n_tiles"])]


@pytest.mark.parametrize("cid", IDS)
def test_case_has_the_geometry_it_claims(cid):
    (rows, cols, off, d), claim, _ = C.CASES[cid]
    g = C.geometry(rows, cols, d)
    assert {k: g[k] for k in claim} == claim, cid
    assert 0 <= off and off + rows <= cols and d % 64 == 0 and 64 <= d <= 4096
    assert (g["live"] - 1) * g["per"] < g["Cp"] // 64 <= g["live"] * g["per"] and g["live"] <= g["splits"] <= 32
    assert g["splits"] * g["m_tiles"] * g["d_tiles"] <= 32 * 16 * g["m_tiles"]       # the tdot partials fit their piece
    assert C.workspace_bytes_py(rows, cols, d) < 9 << 20                            # small: G11's 8.5 MiB is the largest
    band = lambda j: off <= j < off + rows                                          # noqa: E731
    extra = {
        "G1": lambda: (rows, cols) == (1, 1),
        "G2": lambda: rows % 256 == 0 and cols % 256 == 0 and off == 256 and [t for t in _tiles(cid)[3]
                                                                              if C.special_tile(*t, rows, cols, off)] == [(0, 1)],
        "G3": lambda: off + rows == cols and off % 256 == 1,
        "G4": lambda: off % 256 == 255 and rows % 256 and cols % 256,
        "G5": lambda: g["m_tiles"] > 4 and rows == 1024 + 1,
        "G6": lambda: g["live"] == g["splits"] - 1 and off + rows == cols and g["n_tiles"] > 24,
        "G7": lambda: g["last"] == 1 and g["live"] == g["splits"] - 1 and g["n_tiles"] > 40,
        "G8": lambda: g["map"] == "SPLITX" and g["d_last"] < 256,
        "G9": lambda: band(2047) and band(2048) and cols % 256 == 0 and g["d_last"] == 64,
        "G10": lambda: rows == 256 + 1 and cols == 2048 + 1 and off % 256 == 0,
        "G11": lambda: d == 4096 and rows % 256 == 0 and cols % 256 == 0,
    }
    assert extra[cid]()
    c = C.make_case(cid)
    a, b, twins = c["a"], c["b"], c["twins"]
    assert max(float((z.double().norm(dim=1) - 1).abs().max()) for z in (a, b)) < 2.0 ** -7       # unit rows, rounded to bf16
    named = [j for j in C.boundary_columns(cols, [g]) if not band(j)]
    assert [j for j, _ in twins] == named and len(named) <= rows                    # every boundary column got its twin
    assert len({r for _, r in twins}) == len(twins)                                 # ... with a row of its own
    for j, r in twins:
        assert bool((b[j] == b[off + r]).all())
    assert len(twins) == TWIN_COUNTS[cid]
    for T, bias in C.PARAMS:
        t, bs, ref, bnd = _want(cid, T, bias)
        pos = ref["g"][torch.arange(rows), off + torch.arange(rows)]
        # cosine 0.8 in every row: the positives (and the twins, which copy them) share one logit up to the rounding to bf16
        assert float((pos - pos.mean()).abs().max()) < 0.05
        sig = C.signal(c, ref, bnd, c["coef"], t, show=f"{cid} T={T} bias={bias}")
        for j, r in twins:
            assert float(ref["m"][r, j] + ref["m"][r, off + r]) == pytest.approx(1.0, abs=1e-12)
        if twins:
            # conditions on the inputs and the bounds (no kernel output in them): every twin stands well clear of one bound in its
            # loss row and its column of db at both pairs, and in da at the library's defaults (ten of the twenty expected)
            assert sig["loss_rows"] >= 100.0 and sig["db"] >= 2.0, (cid, T, sig)
            if (T, bias) == C.PARAMS[0]:
                assert sig["da"] >= 10.0, (cid, sig)


@pytest.mark.parametrize("cid", IDS)
def test_special_tile_is_the_brute_force_statement(cid):
    """special <=> the tile holds a positive, a padded row or a padded column"""
    rows, cols, off, tiles = _tiles(cid)
    flags = []
    for mi, ni in tiles:
        r0, c0 = 256 * mi, 256 * ni
        brute = r0 + 256 > rows or c0 + 256 > cols or any(c0 <= off + i < c0 + 256 for i in range(r0, min(r0 + 256, rows)))
        assert C.special_tile(mi, ni, rows, cols, off) == brute, (cid, mi, ni)
        flags.append(brute)
    assert any(flags)
    if cid in C.ONE_RAGGED_ROW_TILE:
        assert rows < 256 and all(flags)            # one ragged row tile: the selects run everywhere
    else:
        assert not all(flags), cid                  # the plain path is reached


def test_workspace_bytes_match_the_mirror(lib):
    shapes = [C.CASES[cid][0] for cid in IDS] + [(8192, 65536, 8192, 768), (48, 300, 100, 128)]
    for rows, cols, _, d in shapes:
        assert lib.aecf_sig_workspace_bytes(rows, cols, d) == C.workspace_bytes_py(rows, cols, d), (rows, cols, d)


def test_sig_terms_restatement_against_float64():
    """sigmoid and softplus from the float32 restatement of sig_terms, for n over [-150, 150] with the clamp's neighbourhood and
    n <= -126 in the sweep, against float64 at x = n ln 2 (n as the float32 holds it: dl = 0): inside e_g and e_sp of the bounds"""
    n = torch.cat([torch.linspace(-150.0, 150.0, 30001), torch.tensor([125.999, 126.0, 126.001, -125.999, -126.0, -126.001, -126.5,
                                                                       -127.0, -140.0, -149.0, 0.0, 24.0, 24.5, 25.0, 30.0])]).float()
    sig, lg2, corr = C.sig_terms32(n)
    x = n.double() * 0.6931471805599453094
    want_sig, want_sp = torch.sigmoid(x), -torch.nn.functional.logsigmoid(-x)
    got_sp = lg2.double() * float(torch.tensor(C.LN2, dtype=torch.float32)) + corr.double()
    b_sig = want_sig * ((1.0 - want_sig) * 2.0 * C.H + 4.0 * C.H) + C.FLUSH
    b_sp = want_sig * 2.0 * C.H + 8.0 * C.H * want_sp + C.FLUSH
    r_sig = float(((sig.double() - want_sig).abs() / b_sig).max())
    r_sp = float(((got_sp - want_sp).abs() / b_sp).max())
    print(f"sig tile sig_terms restatement: sigmoid {r_sig:.3f} softplus {r_sp:.3f} of the per-element bound")
    assert bool(torch.isfinite(sig).all()) and bool(torch.isfinite(got_sp).all())
    assert r_sig <= 1.0 and r_sp <= 1.0, (r_sig, r_sp)
    assert float(sig[n >= 126.0].min()) == 1.0                  # past the clamp sigmoid is 1 and softplus is x


@pytest.mark.parametrize("cid,T,bias", CASE_PARAMS)
def test_bounds_hold_the_emulation(cid, T, bias):
    c = C.make_case(cid)
    t, bs, ref, bnd = _want(cid, T, bias)
    r = C.ratios(C.emulate(c, None, t, bs), ref, bnd)
    vb = C.value_over_bound(ref, bnd)
    print(f"sig tile emulation {cid} T={T} bias={bias}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={v:.3g}" for n, v in vb.items()))
    assert set(r) == set(C.OUTPUTS) and all(v <= 1.0 for v in r.values()), (cid, T, r)
    if cid in ("G4", "G8"):                                     # an upstream scalar scales reference and bounds; bf16 adds 2^-8 |value|
        up = 0.375
        _, _, ref_u, bnd_u = _want(cid, T, bias, up)
        got = C.emulate(c, None, t, bs, upstream=up)
        got = dict(got, da=got["da"].to(torch.bfloat16), db=got["db"].to(torch.bfloat16))
        r = C.ratios(got, ref_u, bnd_u, bf16=True)
        assert all(v <= 1.0 for v in r.values()), (cid, T, r)


def _mutations(cid):
    (rows, cols, off, d), _, _ = C.CASES[cid]
    c = C.make_case(cid)
    muts = [(kind, j, r) for j, r in c["twins"] for kind in ("drop", "twice")]
    if cols % 256:
        muts.append(("padcol",))
    if rows % 256:
        muts.append(("padrow",))
    muts.append(("shift",))
    _, _, _, tiles = _tiles(cid)
    band = [(mi, ni) for mi, ni in tiles if any(256 * ni <= off + i < 256 * ni + 256 for i in range(256 * mi, min(256 * mi + 256, rows)))]
    muts += [("plain", mi, ni) for mi, ni in band]
    muts.append(("dbias_bf16",))
    return muts


@pytest.mark.parametrize("cid,T,bias", CASE_PARAMS)
def test_bounds_catch_every_mutation(cid, T, bias):
    """Each mutation of the emulation leaves the bounds by a factor of two at least on one asserted output"""
    c = C.make_case(cid)
    t, bs, ref, bnd = _want(cid, T, bias)
    weakest = {}
    for mut in _mutations(cid):
        if mut[0] == "dbias_bf16" and (cid, (T, bias)) not in DBIAS_BF16_JUDGED:
            continue
        r = C.ratios(C.emulate(c, mut, t, bs), ref, bnd)
        best = max(r, key=r.get)
        assert r[best] >= 2.0, (cid, T, bias, mut, r)
        if mut[0] not in weakest or r[best] < weakest[mut[0]][0]:
            weakest[mut[0]] = (r[best], best)
    print(f"sig tile mutations {cid} T={T} bias={bias}: smallest excess "
          + " ".join(f"{k}={v:.3g}({n})" for k, (v, n) in weakest.items()))


def test_saturated_case_lands_on_both_sides_of_the_clamp():
    """the saturation case of the GPU suite: its marked elements put n = l log2 e within 1 of +-126 on both sides, and the emulation
    is inside the bounds there"""
    c = C.make_saturated()
    t, bs = C.used_temperature(C.SAT_T), C.SAT_BIAS
    s_err = C.score_error_of(c["a"], c["b"])
    ref, bnd = C.reference(c["a"], c["b"], c["off"], t, bs, c["coef"], 1.0, s_err, keep=True)
    S = c["a"].double() @ c["b"].double().T
    n = torch.stack([S[r, j] for r, j in c["marks"]]) / t * C.LOG2E
    for lo, hi in ((125.0, 126.0), (126.0, 127.0), (-126.0, -125.0), (-127.0, -126.0)):
        assert int(((n > lo) & (n < hi)).sum()) >= 2, (lo, hi, n)
    r = C.ratios(C.emulate(c, None, t, bs), ref, bnd)
    print("sig tile emulation saturated: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
