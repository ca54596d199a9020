"""CPU-only tests of the pooled contrastive losses (NT-Xent, the supervised contrastive loss over both views):
aecf_supcon_pool_fwd_bwd is declared, bound and exported with the ABI version still 10; every refusal comes back in the
documented order (sizes -- the three conditions on self_offset among them --, width, NULL pointers, workspace size) before any
pointer is read or any kernel is launched -- the pointers handed over here are deliberately bogus; the Python surface refuses a
CPU tensor, the tile form with intra-view keys and labels for nt_xent; and what tests/test_supcon_pool_gpu.py stands on
(tests/supcon_pool_cases.py) has teeth: the case table has the split geometry it names, an emulation of the design's arithmetic
stays inside the bounds, and the same emulation without the exclusion, or with the excluded key counted as a positive, leaves
them."""
import functools
import os
import re

import pytest
import torch

from aecf_amd import _lib
from tests import nce_stream_cases as C
from tests import supcon_pool_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_pool_symbol_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    assert "aecf_supcon_pool_fwd_bwd" in declared and "aecf_supcon_pool_fwd_bwd" in _lib.SYMBOL_NAMES
    assert hasattr(lib, "aecf_supcon_pool_fwd_bwd")
    assert "aecf_supcon_pool_workspace_bytes" not in declared            # aecf_supcon_workspace_bytes answers for both calls
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def _call(lib, rows=256, cols=512, off=0, self_off=256, d=256, t=BAD, min_t=1e-3, q=BAD, k=BAD, lq=BAD, lk=BAD, lr=BAD, dq=BAD,
          dk=BAD, dt=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_supcon_pool_fwd_bwd(rows, cols, off, self_off, d, t, min_t, 1.0 / max(cols, 1), q, k, lq, lk, lr, dq, dk, dt, ws,
                                        wsb, None)


def test_pool_fwd_bwd_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too): those of aecf_supcon_fwd_bwd, then the three on self_offset
    for bad in (dict(rows=0), dict(cols=0), dict(d=0), dict(min_t=0.0), dict(min_t=-1.0), dict(off=-1), dict(off=257),
                dict(rows=513), dict(cols=2 ** 31), dict(self_off=-1), dict(self_off=257), dict(self_off=0),
                dict(off=100, self_off=100)):
        kw = dict(d=100, t=None, lq=None, wsb=0)
        kw.update(bad)
        assert _call(lib, **kw) == BAD_DIMS, bad
    assert _call(lib, off=256, self_off=0, d=100, wsb=0) == UNSUPPORTED     # (the offsets at their limits are sizes that pass)
    # 2. the width, before any pointer is looked at
    for d in (64, 100, 192, 2048):
        assert _call(lib, d=d, t=None, lk=None, wsb=0) == UNSUPPORTED, d
    # 3. NULL pointers: each of the required ones, the temperature and both label arrays included, and exactly one of dq / dk
    for name in ("t", "q", "k", "lq", "lk", "lr", "ws", "dq", "dk"):
        assert _call(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _call(lib, wsb=0, dq=None, dk=None) == NULL_POINTER              # a loss-only call takes no d_temperature
    # 4. then the workspace size: with gradients, without d_temperature, in the loss-only mode, and one byte short
    assert _call(lib, wsb=16) == WORKSPACE
    assert _call(lib, wsb=16, dt=None) == WORKSPACE
    assert _call(lib, wsb=16, dq=None, dk=None, dt=None) == WORKSPACE
    assert _call(lib, wsb=lib.aecf_supcon_workspace_bytes(256, 512, 256) - 1) == WORKSPACE


def test_python_argument_checks():
    from aecf_amd import losses
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.nt_xent(z, z)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.supervised_contrastive(z, z, lab, intra_view=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="nt_xent")
    with pytest.raises(ValueError, match="labels"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="nt_xent", labels=lab)
    with pytest.raises(ValueError, match="contrastive"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="simclr")
    # an option combination, refused before the tensors are looked at
    with pytest.raises(NotImplementedError, match="intra-view"):
        losses.supervised_contrastive(z, z, lab, low_memory=False, intra_view=True)
    with pytest.raises(NotImplementedError, match="intra-view"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised", labels=lab, low_memory=False,
                                intra_view=True)


# ---- the case table, the bounds and their teeth ----

@pytest.mark.parametrize("cid", P.CASE_IDS)
def test_case_table_has_the_geometry_it_names(cid):
    (rows, cols, off, self_off, d), split, _ = P.CASES[cid]
    assert C.flash_split_py(rows, cols) == split
    assert 0 <= off and off + rows <= cols and 0 <= self_off and self_off + rows <= cols and d in C.WIDTHS
    assert off + rows <= self_off or self_off + rows <= off                 # the two ranges do not overlap
    c = P.make_case(cid)
    assert torch.equal(c["k"][self_off:self_off + rows], c["q"])
    assert torch.equal(c["lk"][off:off + rows], c["lq"]) and torch.equal(c["lk"][self_off:self_off + rows], c["lq"])
    n = P.match_matrix(c["lq"], c["lk"], off, self_off).sum(dim=1)
    assert int(n.min()) >= 1
    _, live, per, last = split
    if cid == "P1":
        assert int(n[0]) == 1 and cols == 2
    if cid == "P4":                                                         # the last split is row 63's excluded key alone
        assert last == 1 and (live - 1) * per == self_off + 63
    if cid == "P5":                                                         # the last sub-tile is row 199's excluded key alone
        assert last == 17 and (live - 1) * per + 16 == self_off + 199 == cols - 1
    if cid == "P7":
        assert off + rows == cols


@functools.lru_cache(maxsize=None)
def _setup(cid, T):
    c = P.make_case(cid)
    q, k, off, self_off = c["q"], c["k"], c["off"], c["self_off"]
    excl = P.excluded(q.shape[0], k.shape[0], self_off)
    M = P.match_matrix(c["lq"], c["lk"], off, self_off)
    t, coef = C.used_temperature(T), 1.0 / k.shape[0]
    ref = P.reference(q, k, M, excl, t, coef)
    bnd = P.bounds(ref, q, k, M, t, coef, C.eps_x(P.score_error(cid), t, k.shape[0]))
    return c, excl, M, t, coef, {n: ref[n] for n in ("loss_rows", "dq", "dk", "dT")}, bnd


@pytest.mark.parametrize("cid", P.CASE_IDS)
def test_bounds_hold_the_emulation_and_catch_a_lost_exclusion(cid):
    from tests import supcon_cases as S
    for T in P.TEMPS:
        c, excl, M, t, coef, ref, bnd = _setup(cid, T)
        q, k = c["q"], c["k"]
        for n in ("loss_rows", "dq", "dk"):
            assert bool(torch.isfinite(ref[n]).all()) and bool(torch.isfinite(bnd[n]).all()), (cid, T, n)
        intact = C.ratios(P.emulate(q, k, M, excl, t, coef), ref, bnd)
        print(f"supcon_pool emulation {cid} T={T}: " + " ".join(f"{n}={v:.3f}" for n, v in intact.items()))
        assert all(v <= 1.0 for v in intact.values()), (cid, T, intact)
        # 1. the exclusion forgotten: the anchor itself, at the highest score 1/T, enters the maximum, the sum and the weights
        over = C.ratios(P.emulate(q, k, M, torch.zeros_like(excl), t, coef), ref, bnd)
        print(f"  without the exclusion: " + " ".join(f"{n}={v:.3g}" for n, v in over.items()))
        assert over["loss_rows"] >= 10.0 and over["dk"] >= 10.0, (cid, T, over)
        assert over["dq"] >= 10.0 and over["dT"] > 1.0, (cid, T, over)
        # 2. the label match taken before the exclusion: the excluded key of a labeled row counts as a positive
        with_self = S.match_matrix(c["lq"], c["lk"], c["off"])
        assert int(with_self.sum()) > int(M.sum())
        over = C.ratios(P.emulate(q, k, with_self, excl, t, coef), ref, bnd)
        print(f"  the excluded key as a positive: " + " ".join(f"{n}={v:.3g}" for n, v in over.items()))
        assert over["loss_rows"] >= 10.0 and over["dk"] >= 10.0, (cid, T, over)
