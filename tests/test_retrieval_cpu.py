"""CPU-only tests of the retrieval-rank entry points: aecf_retrieval_workspace_bytes / aecf_retrieval_positive /
aecf_retrieval_ranks are declared, bound and exported with the ABI version still 10; their refusals come back in the documented
order (sizes, support, NULL pointers, workspace) before any pointer is read or any kernel is launched -- the pointers handed
over here are deliberately bogus; and the Python functions validate their arguments without touching a device."""
import os
import re

import pytest

from aecf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_retrieval_workspace_bytes", "aecf_retrieval_positive", "aecf_retrieval_ranks"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_retrieval_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def test_workspace_bytes_names_the_shapes_served(lib):
    assert lib.aecf_retrieval_workspace_bytes(257, 513, 96) == 0         # d % 64 != 0
    assert lib.aecf_retrieval_workspace_bytes(257, 513, 8192) == 0       # d > 4096
    assert lib.aecf_retrieval_workspace_bytes(0, 513, 64) == 0
    assert lib.aecf_retrieval_workspace_bytes(257, 513, 64) > 0
    # (rows + cols) x tiles integers, never rows x cols: configs[2] size stays far below its 2 GiB float32 block
    big = lib.aecf_retrieval_workspace_bytes(8192, 65536, 768)
    assert 0 < big <= 4 * (8192 * (65536 // 256) + 65536 * (8192 // 256)) + 4096


def _positive(lib, rows=256, cols=512, off=0, d=128, a=BAD, b=BAD, pos=BAD):
    return lib.aecf_retrieval_positive(rows, cols, off, d, a, b, pos, None)


def _ranks(lib, rows=256, cols=512, off=0, d=128, a=BAD, b=BAD, pr=BAD, pc=BAD, rg=BAD, re_=BAD, cg=BAD, ce=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_retrieval_ranks(rows, cols, off, d, a, b, pr, pc, rg, re_, cg, ce, ws, wsb, None)


def test_positive_refuses_in_the_documented_order(lib):
    assert _positive(lib, rows=0, d=96, a=None) == BAD_DIMS
    assert _positive(lib, off=257, d=96, a=None) == BAD_DIMS             # row_offset + rows > cols
    assert _positive(lib, off=-1, d=96, a=None) == BAD_DIMS
    assert _positive(lib, d=96, a=None) == UNSUPPORTED
    assert _positive(lib, d=8192, a=None) == UNSUPPORTED
    for name in ("a", "b", "pos"):
        assert _positive(lib, **{name: None}) == NULL_POINTER, name


def test_ranks_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too)
    assert _ranks(lib, rows=0, d=96, a=None, wsb=0) == BAD_DIMS
    assert _ranks(lib, cols=0, d=96, a=None, wsb=0) == BAD_DIMS
    assert _ranks(lib, off=257, d=96, a=None, wsb=0) == BAD_DIMS         # row_offset + rows > cols
    # 2. support, before any pointer is looked at
    assert _ranks(lib, d=96, a=None, wsb=0) == UNSUPPORTED
    assert _ranks(lib, d=8192, a=None, wsb=0) == UNSUPPORTED
    # 3. NULL pointers, each of them; the column outputs only where the column direction is on
    for name in ("a", "b", "pr", "rg", "re_", "ws", "cg", "ce"):
        assert _ranks(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    # 4. the workspace size (a NULL pos_col with NULL column outputs is a legal call: it gets this far)
    assert _ranks(lib, wsb=16) == WORKSPACE
    assert _ranks(lib, pc=None, cg=None, ce=None, wsb=16) == WORKSPACE


def test_python_refuses_cpu_tensors_and_malformed_arguments():
    torch = pytest.importorskip("torch")
    from aecf_amd import losses
    z = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.retrieval_ranks(z, z)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.retrieval_metrics(z, z)
    with pytest.raises(ValueError, match="ties"):
        losses.retrieval_metrics(z, z, ties="x")
    with pytest.raises(ValueError, match="ks"):
        losses.retrieval_metrics(z, z, ks=(0,))
    with pytest.raises(ValueError, match="ks"):
        losses.retrieval_metrics(z, z, ks=(1, 2.5))
    assert losses.RetrievalRanks._fields == ("a2b_greater", "a2b_equal", "b2a_greater", "b2a_equal")
