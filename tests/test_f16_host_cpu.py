"""CPU-only tests of the float16 element type on the host side of the C ABI (ABI v10): the version, where the shape checks
take AECF_F16 (exactly where they take AECF_BF16), the workspace queries that must stay closed for it, and an entry point that
must refuse it before it looks at any pointer."""
import ctypes
import os

import pytest

from aecf_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _pool(B=4096, M=3, E=512, H=8, dtype=_lib.AECF_F16, mode=1):
    return _lib.PoolDesc(B, M, E, H, dtype, mode, 1, 0.15, 0.7, 1e-8)


def test_abi_version_10(lib):
    assert _lib.AECF_ABI_VERSION == 10 and lib.aecf_abi_version() == 10
    assert _lib.AECF_F16 == 2


POOL_SHAPES = [(M, E, H) for M in (1, 3, 8, 9) for E in (64, 96, 128, 512, 768, 1024, 1088) for H in (1, 2, 4, 8, 16, 17)]


def test_pool_check_takes_f16_where_it_takes_bf16(lib):
    for M, E, H in POOL_SHAPES:
        got = lib.aecf_pool_check(ctypes.byref(_pool(M=M, E=E, H=H)))
        want = lib.aecf_pool_check(ctypes.byref(_pool(M=M, E=E, H=H, dtype=_lib.AECF_BF16)))
        assert got == want, (M, E, H, got, want)
    assert lib.aecf_pool_check(ctypes.byref(_pool(E=64, H=4))) == -2            # head_dim 16: float32 only
    assert lib.aecf_pool_check(ctypes.byref(_pool(E=64, H=4, dtype=_lib.AECF_F32))) == 0
    assert lib.aecf_pool_check(ctypes.byref(_pool(dtype=3))) == -2              # no other element type


def test_mha_check_takes_f16_where_it_takes_bf16(lib):
    for E in (32, 64, 96, 128, 192, 512, 1024, 1088):
        for H in (1, 2, 3, 4, 8):
            if E % H:
                continue
            f16 = lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(8, 2, 5, E, H, _lib.AECF_F16, 0.0)))
            bf16 = lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(8, 2, 5, E, H, _lib.AECF_BF16, 0.0)))
            assert f16 == bf16, (E, H, f16, bf16)
    assert lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(8, 2, 5, 96, 3, _lib.AECF_F16, 0.0))) == -2     # E % 64
    assert lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(8, 2, 5, 96, 3, _lib.AECF_F32, 0.0))) == 0


def test_f16_workspaces_and_closed_paths(lib):
    d16, dbf = _pool(), _pool(dtype=_lib.AECF_BF16)
    r16, rbf = ctypes.byref(d16), ctypes.byref(dbf)
    assert lib.aecf_pool_hilo_bwd_workspace_bytes(r16) == 0                     # the hi/lo products are bf16 only
    assert lib.aecf_pool_hilo_bwd_workspace_bytes(rbf) > 0
    assert lib.aecf_pool_precise_workspace_bytes(r16, 0) == 0 and lib.aecf_pool_precise_workspace_bytes(r16, 1) == 0
    assert lib.aecf_pool_wants_saved_v(r16) == 1                                # no dsu_ws for float16: V is saved
    assert lib.aecf_pool_wants_saved_v(rbf) == 0
    # 2-byte elements: the activation-sized parts of the workspaces are those of bf16, not of float32
    d32 = _pool(dtype=_lib.AECF_F32)
    f16, f32 = lib.aecf_pool_fwd_workspace_bytes(r16), lib.aecf_pool_fwd_workspace_bytes(ctypes.byref(d32))
    assert f16 == lib.aecf_pool_fwd_workspace_bytes(rbf) and f16 < f32
    assert lib.aecf_pool_bwd_workspace_bytes(r16) < lib.aecf_pool_bwd_workspace_bytes(ctypes.byref(d32))
    assert lib.aecf_pool_prep_bytes(r16) == lib.aecf_pool_prep_bytes(rbf)
    md = _lib.MhaDesc(64, 2, 5, 256, 4, _lib.AECF_F16, 0.0)
    md32 = _lib.MhaDesc(64, 2, 5, 256, 4, _lib.AECF_F32, 0.0)
    assert 0 < lib.aecf_mha_bwd_workspace_bytes(ctypes.byref(md)) < lib.aecf_mha_bwd_workspace_bytes(ctypes.byref(md32))
    assert lib.aecf_nce_workspace_bytes(256, 256, 128, _lib.AECF_F16) == 0      # no float16 InfoNCE
    assert lib.aecf_nce_stream_workspace_bytes(256, 256, 128, _lib.AECF_F16) == 0


def test_f16_refused_before_pointers(lib):
    # valid dimensions, null pointers everywhere: the dtype is checked first, so nothing is launched
    assert lib.aecf_modality_frontend(16, 64, _lib.AECF_F16, None, None, None, None, None) == -2
    assert lib.aecf_front_pair(16, 64, 64, _lib.AECF_F16, None, None, None, 0.3, None, None, None, None, None, None, None,
                               None) == -2
    assert lib.aecf_l2norm_forward(16, 64, _lib.AECF_F16, 1e-12, None, None, None, None) == -2
    assert lib.aecf_nce_fwd_bwd(16, 16, 0, 64, _lib.AECF_F16, 0.07, 1.0, None, None, None, None, None, None, 0, None) == -2
    # ... while the entry points opened for float16 get past the dtype and stop at the pointers
    assert lib.aecf_modality_frontend(16, 64, _lib.AECF_BF16, None, None, None, None, None) == -3
    assert lib.aecf_entropy_loss_fwd_bwd(16, _lib.AECF_F16, 3, 0.7, None, 1.0, None, None, None, None) == -3
    assert lib.aecf_sdpa_forward(2, 3, 3, 64, _lib.AECF_F16, 0.125, None, None, None, None, None, None) == -3
    assert lib.aecf_cast_f32_to_f16(1, None, None, None, None) == -3
    assert lib.aecf_cast_f32_to_f16(0, None, None, None, None) == 0
    assert lib.aecf_cast_f32_to_f16(9, None, None, None, None) == -1
    # the pool entry points: AECF_PRECISE stays bf16 only (checked before the arguments' pointers)
    args = _lib.PoolFwdArgs()
    args.flags = _lib.AECF_PRECISE
    assert lib.aecf_pool_forward(ctypes.byref(_pool()), ctypes.byref(args), None) == -2
