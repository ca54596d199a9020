"""CPU-only tests of what tests/test_nce_dense_gpu.py stands on (tests/nce_dense_cases.py): the Python mirror of the workspace
carve agrees with the library's entry point (host code), the case table walks every arm of launch_gemm_nt a dtype can reach, the
float64 reference is the gradient of the plain formula, and the derived bounds have teeth -- an emulation of the form's
arithmetic stays inside them, the same emulation with one fault (a key lost or doubled at a boundary, a misplaced positive, an
ignored offset, a dropped batch row, a dropped column sweep, an unscaled G, a missing dT partial, a dT kept under the clamp)
leaves them on the output named, and losing any sentinel column moves loss_rows or dk beyond its bound."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_dense_cases as C

CASE_IDS = list(C.CASES)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _reference(cid, T, min_t=None):
    c = C.make_case(cid)
    t = C.used_temperature(T)
    mt = None if min_t is None else C.used_temperature(min_t)
    ref = C.reference(c["q"], c["k"], c["off"], t, c["coef"], mt)
    bnd = C.bounds(ref, c["q"], c["k"], c["off"], c["coef"], C.score_error(cid))
    return t, mt, ref, bnd


def _emulate(cid, T, min_t=None, **kw):
    c = C.make_case(cid)
    t, mt, ref, bnd = _reference(cid, T, min_t)
    return C.ratios(C.emulate(c["q"], c["k"], c["off"], t, c["coef"], mt, **kw), ref, bnd)


def test_workspace_bytes_match_the_mirror(lib):
    need = lib.aecf_nce_workspace_bytes
    shapes = [(C.CASES[cid][0], C.CASES[cid][1]) for cid in CASE_IDS]
    shapes += [(dt, (r, c, 0, d)) for dt in (C.F32, C.BF16) for r, c, d in ((1, 64, 64), (3, 64, 192), (63, 128, 320), (129, 192, 64))]
    for dtype, (rows, cols, _, d) in shapes:
        code = _lib.AECF_BF16 if dtype == C.BF16 else _lib.AECF_F32
        mine, theirs = C.workspace_bytes_py(rows, cols, d, dtype), need(rows, cols, d, code)
        assert mine <= theirs, (dtype, rows, cols, d)
        if dtype == C.F32:                                       # no other form can be selected
            assert mine == theirs, (rows, cols, d)
        es = C.esize(dtype)                                      # the tdot scratch (rows floats) lies inside the kT region
        assert rows * 4 <= C.up256(d * cols * es)


def test_case_table_walks_every_arm(lib):
    seen = {C.F32: set(), C.BF16: set()}
    for cid, (dtype, (rows, cols, off, d), claimed, _) in C.CASES.items():
        got = C.arms(dtype, rows, cols, d)
        assert got == claimed, (cid, got)
        seen[dtype] |= set(got)
        assert 0 <= off and off + rows <= cols and cols % 64 == 0 and d % 64 == 0, cid
        # no other form takes the case: no streaming width, and (bf16) every temperature below the tile form's 0.025
        code = _lib.AECF_BF16 if dtype == C.BF16 else _lib.AECF_F32
        assert lib.aecf_nce_stream_workspace_bytes(rows, cols, d, code) == 0, cid
        if dtype == C.BF16:
            assert all(T < 0.025 for T in C.temps_of(cid)), cid
    assert seen[C.F32] == {"32", "128"}                          # float32 never reaches the weight-stationary kernel
    assert seen[C.BF16] == {"32", "128", "ws"}
    assert C.arms(C.F32, 200, 768, 640) == ("32", "32")
    checks = {
        "M1": lambda r, c, o, d: r == 1 and o == c - 1,
        "M2": lambda r, c, o, d: o + r == c and r % 32 and d == 192 and c == 192,
        "M3": lambda r, c, o, d: r == 64 + 1 and c == 256 + 64,
        "M4": lambda r, c, o, d: r == 4 * 32 + 2 and c > 4 * 256 and c % 256,
        "M5": lambda r, c, o, d: r == c and r % 128 == 0 and d % 128 == 0,
        "M6": lambda r, c, o, d: r == 7 * 128 + 104 and c == 8 * 128 + 64 and r > 256,
        "B1": lambda r, c, o, d: c != d or r != c,
        "B2": lambda r, c, o, d: c == 768 and d % 128 == 0 and r % 16 == 8,
        "B3": lambda r, c, o, d: c not in C.WS_K and d not in C.WS_K,
    }
    for cid, (_, shape, _, _) in C.CASES.items():
        assert checks[cid](*shape), cid


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_inputs_and_sentinels(cid):
    dtype, (rows, cols, off, d), _, _ = C.CASES[cid]
    c = C.make_case(cid)
    q, k, sent = c["q"], c["k"], c["sentinels"]
    assert q.dtype == dtype and k.dtype == dtype and c["coef"] == 0.5 / cols
    tol = 2.0 ** -7 if dtype == C.BF16 else 2.0 ** -22
    assert float((q.double().norm(dim=1) - 1).abs().max()) < tol and float((k.double().norm(dim=1) - 1).abs().max()) < tol
    if dtype == C.F32:                                           # full mantissas: the products are not exact
        assert not torch.equal(q, q.to(C.BF16).float())
    assert len({r for _, r, _ in sent}) == len(sent) == len({j for j, _, _ in sent})
    free = [j for j, _ in C.boundary_columns(cols) if not (off <= j < off + rows)]
    assert len(sent) == min(len(free), rows), (cid, len(sent))
    assert (len(sent) == 0) == (cid == "M5")
    for j, r, _ in sent:
        assert not (off <= j < off + rows) and torch.equal(k[j], k[off + r])
    for T in C.temps_of(cid):
        P = _reference(cid, T)[2]["P"]
        for j, r, _ in sent:
            assert float(P[r, j]) == float(P[r, off + r]) and float(P[r, j]) >= 0.25, (cid, T, j, r, float(P[r, j]))


@pytest.mark.parametrize("cid", ["M2", "M3"])
def test_reference_is_the_gradient_of_the_plain_formula(cid):
    c = C.make_case(cid)
    off, coef = c["off"], c["coef"]
    for T in C.temps_of(cid):
        t, _, ref, _ = _reference(cid, T)
        q, k = c["q"].double().requires_grad_(True), c["k"].double().requires_grad_(True)
        Tt = torch.tensor(t, dtype=torch.float64, requires_grad=True)
        i = torch.arange(q.shape[0])
        x = q @ k.T / Tt
        rows = torch.logsumexp(x, dim=1) - x[i, off + i]
        (coef * rows.sum()).backward()
        for name, got in (("loss_rows", rows.detach()), ("dq", q.grad), ("dk", k.grad)):
            assert float((got - ref[name]).abs().max()) <= 1e-12 * max(1.0, float(ref[name].abs().max())), (cid, T, name)
        assert abs(float(Tt.grad) - ref["dT"]) <= 1e-11 * max(1.0, abs(ref["dT"])), (cid, T)
    # the clamp: the reference of a T under min_t is that of min_t with dT = 0
    low = C.reference(c["q"], c["k"], off, C.used_temperature(0.005), coef, C.used_temperature(0.01))
    at = C.reference(c["q"], c["k"], off, C.used_temperature(0.01), coef, C.used_temperature(0.01))
    assert low["dT"] == 0.0 and at["dT"] != 0.0 and torch.equal(low["dq"], at["dq"]) and torch.equal(low["loss_rows"], at["loss_rows"])


@pytest.mark.parametrize("cid", C.SMALL)
def test_bounds_hold_the_emulation(cid):
    for T in C.temps_of(cid):
        _, _, ref, bnd = _reference(cid, T)
        intact = _emulate(cid, T)
        vb = C.value_over_bound(ref, bnd)
        print(f"nce dense emulation {cid} T={T}: " + " ".join(f"{n}={v:.3f}" for n, v in intact.items())
              + " | value/bound " + " ".join(f"{n}={vb[n]:.3g}" for n in intact))
        assert set(intact) == set(C.OUTPUTS)
        assert all(v <= 1.0 for v in intact.values()), (cid, T, intact)
    if cid == "M3":                                              # under the clamp: dT is exactly zero on both sides
        assert _emulate("M3", 0.005, 0.01)["dT"] == 0.0


# name: (the output it is judged on, the cases it is tried on, the switches of C.emulate, (T, min_t) or None: the case's first T)
MUTATIONS = {
    "positive taken at off + i + 1": ("loss_rows", ("M2", "M3", "B1"), dict(pos_shift=1), None),
    "row_offset ignored": ("loss_rows", ("M2", "M3", "B2"), dict(ignore_offset=True), None),
    "last batch row dropped from dk": ("dk", ("M2", "M4", "B2"), dict(drop_last_row_dk=True), None),
    "last partial column sweep dropped from the row sum": ("loss_rows", ("M3", "M4"), dict(drop_last_sweep=True), None),
    "G left unscaled by coef / T (dq)": ("dq", ("M3", "M5", "B1"), dict(unscaled=True), None),
    "G left unscaled by coef / T (dk)": ("dk", ("M3", "M5", "B1"), dict(unscaled=True), None),
    "last strided partial missing from dT": ("dT", ("M1", "M3", "M4", "M5"), dict(drop_last_partial=True), None),
    "dT not zeroed below the clamp": ("dT", ("M3", "M5"), dict(keep_dt_below_clamp=True), (0.05, 0.07)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_leaves_the_bounds(name):
    output, cids, switches, temps = MUTATIONS[name]
    worst = 0.0
    for cid in cids:
        T, min_t = temps or (C.temps_of(cid)[0], None)
        intact, bad = _emulate(cid, T, min_t), _emulate(cid, T, min_t, **switches)
        print(f"nce dense mutation '{name}' {cid} T={T}: {output} {intact[output]:.3f} -> {bad[output]:.3g}")
        assert intact[output] <= 1.0
        worst = max(worst, bad[output])
    assert worst > 1.0, (name, worst)


def test_every_sentinel_has_teeth():
    """a key lost (once per boundary kind and more: every sentinel of every case) or counted twice moves the loss of the
    sentinel's row or dk of its column beyond the bound"""
    kinds = set()
    for cid in CASE_IDS:
        c = C.make_case(cid)
        q, k, off = c["q"], c["k"], c["off"]
        for T in C.temps_of(cid):
            t, _, ref, bnd = _reference(cid, T)
            for n, (j, r, kind) in enumerate(c["sentinels"]):
                for what, kw in (("lost", dict(drop_col=j)), ("twice", dict(dup_col=j))):
                    if what == "twice" and n > 0 and cid not in C.SMALL:
                        continue                                 # (the large cases: one doubled key each)
                    bad = C.emulate(q, k, off, t, c["coef"], **kw)
                    over_loss = abs(float(bad["loss_rows"][r]) - float(ref["loss_rows"][r])) / float(bnd["loss_rows"][r])
                    over_dk = float(((bad["dk"][j].double() - ref["dk"][j]).abs() / bnd["dk"][j]).max())
                    print(f"nce dense teeth {cid} T={T} {kind} (column {j}, row {r}) {what}: loss {over_loss:.0f}x dk {over_dk:.0f}x")
                    assert max(over_loss, over_dk) > 1.0, (cid, T, j, r, what, over_loss, over_dk)
                kinds.add(kind)
    # every boundary kind of the table was lost once (column 1024 is M4's, M6's and B3's "first column of the last tile")
    assert kinds == {kind for _, kind in C.boundary_columns(2048)} - {"column 1024"}, kinds


def test_l2_bounds_hold_a_float32_emulation():
    """the l2norm bounds against a float32 / bf16 torch rendering of the two kernels, on every shape and special row"""
    eps = C.used_temperature(C.L2_EPS)
    for n, d in C.L2_SHAPES:
        for dtype in (C.F32, C.BF16):
            for z, kinds in C.l2_inputs(n, d, dtype):
                ref, bnd, _ = C.l2_forward_reference(z, eps)
                zf = z.float()
                inv = 1.0 / torch.clamp_min(torch.sqrt((zf * zf).sum(dim=1)), eps)
                zn = (zf * inv[:, None]).to(dtype)
                assert C.l2_ratio(zn, ref["zn"], bnd["zn"]) <= 1.0, (n, d, dtype, kinds)
                assert C.l2_ratio(inv, ref["inv_norm"], bnd["inv_norm"]) <= 1.0, (n, d, dtype, kinds)
                for r, kind in kinds.items():
                    if kind == "zero":
                        assert float(zn[r].float().abs().max()) == 0.0 and float(inv[r]) == float(torch.tensor(1.0) / torch.tensor(eps))
                    if kind == "tiny":
                        assert float(ref["inv_norm"][r]) == 1.0 / eps
                g = torch.Generator().manual_seed(n + d)
                dzn = torch.randn(n, d, generator=g)
                want, b_dz = C.l2_backward_reference(zn, inv, dzn)
                dot = (dzn * zn.float()).sum(dim=1, keepdim=True)
                dz = ((dzn - zn.float() * dot) * inv[:, None]).to(dtype)
                assert bool(torch.isfinite(dz.float()).all())
                assert C.l2_ratio(dz, want, b_dz) <= 1.0, (n, d, dtype, kinds)
                # teeth: a backward without the projection term leaves the bound on every row that is not all zero
                plain = (dzn * inv[:, None]).to(dtype)
                if any(kind != "zero" for kind in kinds.values()) or not kinds:
                    assert C.l2_ratio(plain, want, b_dz) > 1.0, (n, d, dtype, kinds)
