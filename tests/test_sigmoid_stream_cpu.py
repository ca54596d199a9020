"""CPU-only tests of the streaming sigmoid contrastive entry points: aecf_sig_stream_workspace_bytes / aecf_sig_stream_fwd_bwd are
declared, bound and exported with the ABI version still 10; the workspace is O(rows d) and does not grow with the column
count beyond the split count; and every refusal comes back in the documented order (sizes, width, NULL pointers, workspace
size) before any pointer is read or any kernel is launched -- the pointers handed over here are deliberately bogus."""
import os
import re

import pytest

from aecf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_sig_stream_workspace_bytes", "aecf_sig_stream_fwd_bwd"]
WIDTHS = (128, 256, 384, 512, 768, 1024)
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_stream_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def test_workspace_bytes_names_the_widths_served(lib):
    need = lib.aecf_sig_stream_workspace_bytes
    for d in (64, 192, 2048):
        assert need(333, 333, d) == 0
    for rows, cols, d in [(0, 333, 256), (333, 0, 256), (-1, 333, 256), (333, -1, 256), (333, 333, 0), (333, 333, -128)]:
        assert need(rows, cols, d) == 0
    for d in WIDTHS:
        assert need(333, 333, d) > 0
        assert need(1, 1, d) > 0


def test_workspace_is_rows_by_d_not_rows_by_cols(lib):
    need = lib.aecf_sig_stream_workspace_bytes
    small = need(8192, 65536, 768)
    assert 0 < small < lib.aecf_sig_workspace_bytes(8192, 65536, 768) // 8
    assert need(8192, 1048576, 768) <= 2 * small              # no growth with cols beyond the split count


def _call(lib, rows=256, cols=256, off=0, d=256, t=BAD, min_t=1e-3, bias=BAD, a=BAD, b=BAD, lr=BAD, dbias=BAD, dt=BAD, da=BAD, db=BAD,
          ws=BAD, wsb=1 << 30):
    return lib.aecf_sig_stream_fwd_bwd(rows, cols, off, d, t, min_t, bias, 1.0 / max(cols, 1), a, b, lr, dbias, dt, da, db, ws, wsb,
                                       None)


def test_fwd_bwd_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too)
    for bad in (dict(rows=0), dict(cols=0), dict(d=0), dict(min_t=0.0), dict(min_t=-1.0), dict(off=-1), dict(off=1),
                dict(rows=257)):
        kw = dict(d=100, t=None, wsb=0)
        kw.update(bad)
        assert _call(lib, **kw) == BAD_DIMS, bad
    # 2. the width, before any pointer is looked at
    for d in (64, 100, 192, 2048):
        assert _call(lib, d=d, t=None, wsb=0) == UNSUPPORTED, d
    # 3. NULL pointers, each of the required ones, and exactly one of da / db
    for name in ("t", "bias", "a", "b", "lr", "ws", "da", "db"):
        assert _call(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    # 4. then the workspace size: with gradients, in the loss-only mode, and with the optional scalars left out
    assert _call(lib, wsb=16) == WORKSPACE
    assert _call(lib, wsb=16, da=None, db=None, dbias=None, dt=None) == WORKSPACE
    assert _call(lib, wsb=16, dbias=None, dt=None) == WORKSPACE
    assert _call(lib, wsb=lib.aecf_sig_stream_workspace_bytes(256, 256, 256) - 1) == WORKSPACE
