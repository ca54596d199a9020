"""CPU-only tests of what tests/test_nce_stream_gpu.py stands on (tests/nce_stream_cases.py): the Python mirror of the split rule
agrees with the library's workspace entry point (host code), every case has the split geometry its row of the table claims,
the sentinels carry enough softmax weight at every temperature used, and the derived bounds have teeth -- an emulation of the
kernel's arithmetic stays inside them, and the same emulation with one sentinel key dropped or counted twice leaves them by a
factor of ten at least."""
import functools
import os

import pytest

from aecf_amd import _lib
from tests import nce_stream_cases as C

CASE_IDS = list(C.CASES)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _reference(cid, T):
    c = C.make_case(cid)
    rows, cols = c["q"].shape[0], c["k"].shape[0]
    t, coef = C.used_temperature(T), 1.0 / cols
    ref = C.reference(c["q"], c["k"], c["off"], t, coef)
    bnd = C.bounds(ref, c["q"], c["k"], c["off"], t, coef, C.eps_x(C.score_error(cid), t, cols))
    return t, coef, ref, bnd


def test_workspace_bytes_match_the_mirror(lib):
    need = lib.aecf_nce_stream_workspace_bytes
    for cid, ((rows, cols, _, _), _, _) in C.CASES.items():
        for d in C.WIDTHS:
            assert need(rows, cols, d, _lib.AECF_BF16) == C.workspace_bytes_py(rows, cols, d), (cid, d)
        assert need(rows, cols, 192, _lib.AECF_BF16) == 0
        for d in C.WIDTHS:
            assert need(rows, cols, d, _lib.AECF_F32) == 0


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_has_the_geometry_it_claims(cid):
    (rows, cols, off, d), split, _ = C.CASES[cid]
    assert C.flash_split_py(rows, cols) == split
    rule, live, per, last = split
    assert per % 32 == 0 and (live - 1) * per < cols <= live * per and last == cols - (live - 1) * per and live <= rule
    assert 0 <= off and off + rows <= cols and d in C.WIDTHS
    tail = last % 32 or 32                                      # keys of the last tile of the last split
    checks = {
        "A": rows == 1 and cols == 1,
        "B": rows == 1 and live == 2 and off == cols - 1,
        "C": last == 12 * 32 + 1 and rows == 64 + 1,
        "D": live == 1 and tail == 12 and rows == 32 + 31,
        "E": live == 16 and last == 1,
        "F": last == 17 and off + rows == cols and d == 768,
        "G": last == 32 + 1 and d == 1024 and rows == 32 + 1,
        "H": (rule, live) == (32, 31),
    }
    assert checks[cid]
    c = C.make_case(cid)
    sent = c["sentinels"]
    assert len({r for _, r in sent}) == len(sent) == len({j for j, _ in sent})
    assert len(sent) == dict(A=0, B=1, C=5, D=4, E=4, F=5, G=4, H=5)[cid]       # as many as distinct rows and columns allow
    for j, r in sent:
        assert not (off <= j < off + rows) and bool((c["k"][j] == c["k"][off + r]).all())
    norms = [float((z.double().norm(dim=1) - 1).abs().max()) for z in (c["q"], c["k"])]
    assert max(norms) < 2.0 ** -7                               # unit rows, rounded to bf16


@pytest.mark.parametrize("cid", CASE_IDS)
def test_sentinels_hold_a_quarter_of_their_row(cid):
    c = C.make_case(cid)
    for T in C.TEMPS:
        P = _reference(cid, T)[2]["P"]
        for j, r in c["sentinels"]:
            share = float(P[r, j])
            assert share == float(P[r, c["off"] + r]) and share >= 0.25, (cid, T, j, r, share)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bounds_hold_the_emulation_and_catch_a_lost_or_doubled_key(cid):
    c = C.make_case(cid)
    q, k, off = c["q"], c["k"], c["off"]
    for T in C.TEMPS:
        t, coef, ref, bnd = _reference(cid, T)
        intact = C.ratios(C.emulate(q, k, off, t, coef), ref, bnd)
        print(f"nce stream emulation {cid} T={T}: " + " ".join(f"{n}={v:.3f}" for n, v in intact.items()))
        assert all(v <= 1.0 for v in intact.values()), (cid, T, intact)
        for j, r in c["sentinels"]:
            for times in (0, 2):
                bad = C.emulate(q, k, off, t, coef, column=j, times=times)
                over_loss = abs(float(bad["loss_rows"][r]) - float(ref["loss_rows"][r])) / float(bnd["loss_rows"][r])
                over_dk = float(((bad["dk_column"].double() - ref["dk"][j]).abs() / bnd["dk"][j]).max())
                print(f"  column {j} (row {r}) x{times}: loss {over_loss:.0f}x dk {over_dk:.0f}x")
                assert max(over_loss, over_dk) >= 10.0, (cid, T, j, r, times, over_loss, over_dk)
