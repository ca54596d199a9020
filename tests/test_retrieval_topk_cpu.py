"""CPU-only tests of the top-k retrieval entry points: aecf_retrieval_topk_workspace_bytes / aecf_retrieval_topk are declared,
bound and exported with the ABI version still 10; the workspace query names the shapes served and stays far below rows x cols;
the refusals come back in the documented order (sizes, support, NULL pointers, workspace) before any pointer is read or any
kernel is launched -- the pointers handed over here are deliberately bogus; and losses.retrieval_topk validates its arguments
without touching a device."""
import os
import re

import pytest

from aecf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_retrieval_topk_workspace_bytes", "aecf_retrieval_topk"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_topk_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def test_workspace_bytes_names_the_shapes_served(lib):
    wsb = lib.aecf_retrieval_topk_workspace_bytes
    assert wsb(257, 513, 96, 10) == 0            # d % 64 != 0
    assert wsb(257, 513, 8192, 10) == 0          # d > 4096
    assert wsb(257, 513, 64, 0) == 0             # k < 1
    assert wsb(257, 513, 64, 17) == 0            # k > 16
    assert wsb(0, 513, 64, 10) == 0
    assert wsb(257, 513, 64, 16) > 0
    # 8 KP bytes per row and column tile, never rows x cols: the configs[2] size stays far below its 2 GiB float32 block
    big = wsb(8192, 65536, 768, 10)
    assert 0 < big <= 8 * 16 * 8192 * 256 + 4096
    # the formula of the header, for every k: KP = k rounded up to a power of two, Rp = rows rounded up to 256
    for k in range(1, 17):
        kp = 1 << (k - 1).bit_length()
        assert 8 * kp * 512 * 3 <= wsb(257, 513, 64, k) <= 8 * kp * 512 * 3 + 4096, k


def _topk(lib, rows=256, cols=512, off=0, d=128, k=10, excl=0, a=BAD, b=BAD, values=BAD, indices=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_retrieval_topk(rows, cols, off, d, k, excl, a, b, values, indices, ws, wsb, None)


def test_topk_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too)
    assert _topk(lib, rows=0, d=96, a=None, wsb=0) == BAD_DIMS
    assert _topk(lib, cols=0, d=96, a=None, wsb=0) == BAD_DIMS
    assert _topk(lib, k=0, d=96, a=None, wsb=0) == BAD_DIMS
    assert _topk(lib, k=-3, d=96, a=None, wsb=0) == BAD_DIMS
    assert _topk(lib, cols=9, k=10, d=96, a=None, wsb=0) == BAD_DIMS                     # k beyond the columns
    assert _topk(lib, rows=10, cols=10, k=10, excl=1, d=96, a=None, wsb=0) == BAD_DIMS    # ... beyond those left after exclusion
    assert _topk(lib, cols=8, rows=8, k=17, a=None, wsb=0) == BAD_DIMS                   # (sizes come before k > 16)
    assert _topk(lib, off=257, excl=1, d=96, a=None, wsb=0) == BAD_DIMS                  # row_offset + rows > cols
    assert _topk(lib, off=-1, excl=1, d=96, a=None, wsb=0) == BAD_DIMS
    # 2. support, before any pointer is looked at; without exclude_partner row_offset is ignored
    assert _topk(lib, d=96, a=None, wsb=0) == UNSUPPORTED
    assert _topk(lib, d=8192, a=None, wsb=0) == UNSUPPORTED
    assert _topk(lib, k=17, a=None, wsb=0) == UNSUPPORTED
    assert _topk(lib, off=257, d=96, a=None, wsb=0) == UNSUPPORTED
    assert _topk(lib, off=-1, k=17, a=None, wsb=0) == UNSUPPORTED
    # 3. NULL pointers, each of them
    for name in ("a", "b", "values", "indices", "ws"):
        assert _topk(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    # 4. the workspace size: one byte short is refused (exactly enough would launch, so it is not tried here)
    need = lib.aecf_retrieval_topk_workspace_bytes(256, 512, 128, 10)
    assert need > 0
    assert _topk(lib, wsb=16) == WORKSPACE
    assert _topk(lib, wsb=need - 1) == WORKSPACE
    assert _topk(lib, off=-1, wsb=need - 1) == WORKSPACE
    assert _topk(lib, rows=512, cols=512, k=16, excl=1, wsb=16) == WORKSPACE


def test_python_refuses_cpu_tensors_and_malformed_arguments(monkeypatch):
    torch = pytest.importorskip("torch")
    from aecf_amd import losses
    z = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.retrieval_topk(z, z, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):        # the device check comes first
        losses.retrieval_topk(z.float(), z, 0)
    assert losses.RetrievalTopK._fields == ("values", "indices")
    # the argument checks behind it read no data and load no library: let CPU tensors past the device check to reach them
    monkeypatch.setattr(losses, "_require_device", lambda t, what: None)
    monkeypatch.setattr(losses._lib, "load", lambda: pytest.fail("an argument check must refuse before the library is loaded"))
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.retrieval_topk(z.float(), z.float(), 4)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.retrieval_topk(z, z.to(torch.float16), 4)
    for k in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="positive integer k"):
            losses.retrieval_topk(z, z, k)
    with pytest.raises(NotImplementedError, match="k <= 16"):
        losses.retrieval_topk(torch.zeros(32, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16), 17)
    with pytest.raises(ValueError, match="keys to choose from"):
        losses.retrieval_topk(z, z, 10)                             # k > cols
    with pytest.raises(ValueError, match="keys to choose from"):
        losses.retrieval_topk(z, z, 8, exclude_partner=True)        # k > cols - 1
    with pytest.raises(ValueError, match="equal shape"):
        losses.retrieval_topk(z, torch.zeros(16, 64, dtype=torch.bfloat16), 4, exclude_partner=True)
    with pytest.raises(ValueError, match=r"\[b_q, d\]"):
        losses.retrieval_topk(z, torch.zeros(16, 128, dtype=torch.bfloat16), 4)
    with pytest.raises(NotImplementedError, match="d % 64"):
        losses.retrieval_topk(torch.zeros(8, 96, dtype=torch.bfloat16), torch.zeros(8, 96, dtype=torch.bfloat16), 4)
