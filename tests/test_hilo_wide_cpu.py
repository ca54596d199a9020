"""CPU-only: which descriptions the hi/lo weight-gradient products (AECF_HILO_GRADS) are built for.  Every bf16 shape whose value
projection runs on the weight-stationary engine -- d = 256, 512, 768, 1024 with M <= 4 and head_dim % 32 == 0 -- including the
per-rank shards of the d = 768 and d = 1024 benchmark configurations and any four-modality pool; nothing else."""
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


def _desc(B, M, E, H, dtype=_lib.AECF_BF16):
    return _lib.PoolDesc(B, M, E, H, dtype, 1, 1, 0.15, 0.7, 1e-8)


def _hilo_bytes(lib, *shape, **kw):
    return lib.aecf_pool_hilo_bwd_workspace_bytes(ctypes.byref(_desc(*shape, **kw)))


# (B, M, E, H): the two benchmark shards, the test batches of the full-size suite and every M of the new widths
BUILT = [
    (8192, 2, 768, 8), (16384, 4, 1024, 8), (1024, 2, 768, 8), (512, 4, 1024, 8),
    (700, 4, 512, 8), (4133, 4, 512, 8), (1100, 4, 256, 8),
    (700, 1, 768, 8), (1100, 3, 768, 8), (4133, 4, 768, 8), (700, 4, 768, 4),
    (700, 1, 1024, 8), (1100, 2, 1024, 8), (4133, 4, 1024, 8), (1100, 2, 1024, 4),
]


@pytest.mark.parametrize("B,M,E,H", BUILT)
def test_hilo_built_for_wide_and_four_modality_shapes(lib, B, M, E, H):
    got = _hilo_bytes(lib, B, M, E, H)
    base = lib.aecf_pool_bwd_workspace_bytes(ctypes.byref(_desc(B, M, E, H)))
    # the hi/lo workspace is the default one plus the low part of do (B x E bf16)
    assert got >= base + B * E * 2, (B, M, E, H, got, base)


@pytest.mark.parametrize("B,M,E,H,dtype", [
    (8192, 2, 768, 8, _lib.AECF_F16), (8192, 2, 768, 8, _lib.AECF_F32),    # bf16 only (float16 refusal stays)
    (16384, 4, 1024, 8, _lib.AECF_F16), (512, 4, 512, 8, _lib.AECF_F32),
    (1024, 5, 512, 8, _lib.AECF_BF16), (1024, 8, 768, 8, _lib.AECF_BF16),  # M > 4: the LDS-tile route keeps the default products
    (1024, 3, 1024, 8, _lib.AECF_BF16),                                    # no weight-stationary value projection at d = 1024, M = 3
    (1024, 2, 384, 4, _lib.AECF_BF16), (1024, 2, 128, 2, _lib.AECF_BF16),  # E outside the engine's set
    (1024, 2, 640, 4, _lib.AECF_BF16), (1024, 2, 768, 16, _lib.AECF_BF16),  # (and descriptions the pool refuses altogether)
])
def test_hilo_refused_elsewhere(lib, B, M, E, H, dtype):
    assert _hilo_bytes(lib, B, M, E, H, dtype=dtype) == 0


def test_hilo_unchanged_where_it_was_built(lib):
    # d = 256 / 512 with M <= 3: built before, still built
    for shape in [(65536, 3, 512, 8), (200, 3, 512, 8), (4096, 2, 256, 4), (1000, 1, 512, 16)]:
        assert _hilo_bytes(lib, *shape) > 0, shape
