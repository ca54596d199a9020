"""CPU-only tests of the sigmoid (SigLIP) contrastive entry points: aecf_sig_workspace_bytes / aecf_sig_pass1 / aecf_sig_grads are
declared, bound and exported with the ABI version still 10; their refusals come back in the documented order (sizes, dtype /
shape support, NULL pointers) before any pointer is read or any kernel is launched -- the pointers handed over here are
deliberately bogus; and the Python wrapper validates its scalar arguments without touching a device."""
import os
import re

import pytest

from aecf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG_SYMBOLS = ["aecf_sig_workspace_bytes", "aecf_sig_pass1", "aecf_sig_grads"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_sig_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SIG_SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def test_workspace_bytes_names_the_shapes_served(lib):
    assert lib.aecf_sig_workspace_bytes(333, 333, 100) == 0          # d % 64 != 0
    assert lib.aecf_sig_workspace_bytes(0, 333, 256) == 0
    need = lib.aecf_sig_workspace_bytes(333, 333, 256)
    assert need >= 512 * 512 * 2                                      # the padded bf16 g is in it
    assert lib.aecf_sig_workspace_bytes(8192, 65536, 768) > 8192 * 65536 * 2


def _pass1(lib, rows=256, cols=256, off=0, d=256, t=BAD, min_t=1e-3, bias=BAD, a=BAD, b=BAD, ws=BAD, wsb=1 << 30, lr=BAD, db=BAD):
    return lib.aecf_sig_pass1(rows, cols, off, d, t, min_t, bias, a, b, ws, wsb, lr, db, None)


def _grads(lib, rows=256, cols=256, off=0, d=256, t=BAD, min_t=1e-3, a=BAD, b=BAD, ws=BAD, wsb=1 << 30, gd=_lib.AECF_BF16, da=BAD,
           db=BAD):
    return lib.aecf_sig_grads(rows, cols, off, d, t, min_t, 1.0 / cols, a, b, ws, wsb, None, gd, da, db, None, None)


def test_pass1_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too)
    assert _pass1(lib, rows=0, d=100, t=None) == BAD_DIMS
    assert _pass1(lib, min_t=0.0, d=100, t=None) == BAD_DIMS
    assert _pass1(lib, off=1, d=100, t=None) == BAD_DIMS             # row_offset + rows > cols
    # 2. shape support, before any pointer is looked at
    assert _pass1(lib, d=100, t=None) == UNSUPPORTED
    # 3. NULL pointers, each of them
    for name in ("t", "bias", "a", "b", "ws", "lr", "db"):
        assert _pass1(lib, **{name: None}) == NULL_POINTER, name
    # then the workspace size
    assert _pass1(lib, wsb=16) == -4


def test_grads_refuses_in_the_documented_order(lib):
    assert _grads(lib, rows=0, d=100, t=None) == BAD_DIMS
    assert _grads(lib, min_t=-1.0, d=100, t=None) == BAD_DIMS
    assert _grads(lib, d=100, t=None) == UNSUPPORTED
    assert _grads(lib, gd=_lib.AECF_F16, t=None) == UNSUPPORTED
    for name in ("t", "a", "b", "ws", "da", "db"):
        assert _grads(lib, **{name: None}) == NULL_POINTER, name
    assert _grads(lib, wsb=16) == -4


def test_python_rejects_malformed_temperature_and_bias():
    torch = pytest.importorskip("torch")
    from aecf_amd.losses import _sig_args
    z = torch.zeros(4, 64)
    assert _sig_args(0.1, -10, z, 1e-3) == (0.1, -10.0)
    for which in ("temperature", "bias"):
        def call(v, min_t=1e-3):
            return _sig_args(v, -10.0, z, min_t) if which == "temperature" else _sig_args(0.1, v, z, min_t)
        with pytest.raises(TypeError, match=which):
            call(torch.tensor(0.1, dtype=torch.float64))
        with pytest.raises(ValueError, match=which):
            call(torch.tensor([0.1, 0.2]))
        with pytest.raises(ValueError, match=which):
            call(torch.tensor(0.1, device="meta"))                     # not where the embeddings live
        with pytest.raises(ValueError, match="min_temperature"):
            call(torch.tensor(0.1), 0.0)
        with pytest.raises(ValueError, match="min_temperature"):
            call(0.1, -1.0)
        v = torch.tensor(0.1)
        assert call(v)[0 if which == "temperature" else 1] is v


def test_cpu_tensors_are_refused():
    torch = pytest.importorskip("torch")
    from aecf_amd import losses
    z = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.sigmoid_contrastive(z, z)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="sigmoid")
    with pytest.raises(ValueError, match="contrastive"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="softmax")
