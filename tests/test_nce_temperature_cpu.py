"""CPU-only tests of the device-temperature InfoNCE entry points (aecf_*_dt): they are exported and bound, the ABI version stays
10, and their refusals (float16, a tile form below the 0.025 bound, a NULL temperature) come back before any pointer is read
or any kernel is launched -- the pointers handed over here are deliberately bogus."""
import os
import re

import pytest

from aecf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_SYMBOLS = ["aecf_nce_fwd_bwd_dt", "aecf_loss_fwd_bwd_dt", "aecf_nce_sym_pass1_dt", "aecf_nce_sym_loss_dt",
              "aecf_nce_sym_grads_dt"]
BAD = 0x10          # never dereferenced: every call below must refuse first
UNSUPPORTED, NULL_POINTER = -2, -3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_dt_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in DT_SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def test_fwd_bwd_dt_refuses_f16_before_pointers(lib):
    assert lib.aecf_nce_fwd_bwd_dt(256, 256, 0, 256, _lib.AECF_F16, BAD, 0.025, 0.5 / 256, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
                                   1 << 30, None) == UNSUPPORTED
    # a NULL temperature (the only other change against aecf_nce_fwd_bwd)
    assert lib.aecf_nce_fwd_bwd_dt(256, 256, 0, 256, _lib.AECF_BF16, None, 0.025, 0.5 / 256, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
                                   1 << 30, None) == NULL_POINTER
    # min_temperature must be positive (checked with the sizes)
    assert lib.aecf_nce_fwd_bwd_dt(256, 256, 0, 256, _lib.AECF_BF16, BAD, 0.0, 0.5 / 256, BAD, BAD, BAD, BAD, BAD, BAD, BAD,
                                   1 << 30, None) == -1


def test_loss_fwd_bwd_dt_refuses_null_temperature(lib):
    assert lib.aecf_loss_fwd_bwd_dt(256, 256, 0, 256, None, 0.025, 0.5 / 256, BAD, BAD, BAD, BAD, BAD, BAD, 0, 2, 0.7, None,
                                    1.0, None, None, BAD, 1 << 30, None) == NULL_POINTER


def test_sym_dt_refuses_low_min_temperature_and_null_temperature(lib):
    # the tile forms' constant shift 1/T needs T >= 0.025: a min_temperature below it is refused by all three calls
    assert lib.aecf_nce_sym_pass1_dt(256, 256, 256, BAD, 0.02, BAD, BAD, BAD, 1 << 30, BAD, None) == UNSUPPORTED
    assert lib.aecf_nce_sym_loss_dt(256, 256, 0, 256, BAD, 0.02, BAD, BAD, BAD, BAD, 1 << 30, BAD, 0, 2, 0.7, None, 1.0, None,
                                    None, None) == UNSUPPORTED
    assert lib.aecf_nce_sym_grads_dt(256, 256, 0, 256, BAD, 0.02, 0.5 / 256, BAD, BAD, BAD, 1 << 30, None, _lib.AECF_BF16, BAD,
                                     BAD, BAD, None) == UNSUPPORTED
    # gradients in float16: refused, as by aecf_nce_sym_grads
    assert lib.aecf_nce_sym_grads_dt(256, 256, 0, 256, BAD, 0.025, 0.5 / 256, BAD, BAD, BAD, 1 << 30, None, _lib.AECF_F16, BAD,
                                     BAD, BAD, None) == UNSUPPORTED
    # a NULL temperature at the bound
    assert lib.aecf_nce_sym_pass1_dt(256, 256, 256, None, 0.025, BAD, BAD, BAD, 1 << 30, BAD, None) == NULL_POINTER
    assert lib.aecf_nce_sym_loss_dt(256, 256, 0, 256, None, 0.025, BAD, BAD, BAD, BAD, 1 << 30, BAD, 0, 2, 0.7, None, 1.0, None,
                                    None, None) == NULL_POINTER
    assert lib.aecf_nce_sym_grads_dt(256, 256, 0, 256, None, 0.025, 0.5 / 256, BAD, BAD, BAD, 1 << 30, None, _lib.AECF_BF16, BAD,
                                     BAD, BAD, None) == NULL_POINTER


def test_python_rejects_malformed_temperatures():
    torch = pytest.importorskip("torch")
    from aecf_amd.losses import _temperature_arg
    z = torch.zeros(4, 64)
    assert _temperature_arg(0.07, z, 0.025) == 0.07
    with pytest.raises(TypeError):
        _temperature_arg(torch.tensor(0.07, dtype=torch.float64), z, 0.025)
    with pytest.raises(ValueError):
        _temperature_arg(torch.tensor([0.07, 0.08]), z, 0.025)
    with pytest.raises(ValueError):
        _temperature_arg(torch.tensor(0.07), z, 0.0)
    t = torch.tensor(0.07)
    assert _temperature_arg(t, z, 0.025) is t
