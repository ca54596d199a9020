"""CPU side of the general attention route's edge tests (tests/test_mha_edges_gpu.py): the judge is right on what it is about
to judge, the case table tests the chunking its comments claim, and the backward's workspace holds the float32 dk / dv carries
exactly when there is a second query chunk."""
import ctypes
import os

import pytest
import torch

from aecf_amd import _lib
from tests import mha_edges_cases as C


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


PINS = ["bool3d+bool_kpm", "float2d+bool_kpm", "nobias", "key_is_value", "float_kpm+bool2d"]


@pytest.mark.parametrize("name", PINS)
def test_oracle_matches_torch_module_in_float64_on_option_combinations(name):
    """oracle/ is pinned against the reference for the four g11 option sets only.  Here it meets torch.nn.MultiheadAttention
    in float64 -- the module the reference itself calls -- on the combinations the GPU tests judge with it: all outputs and
    gradients to 1e-12.  A float key_padding_mask reaches the oracle merged into the [B*H,T,S] additive mask, as the layer
    merges it before the C call; torch is given the float key_padding_mask itself."""
    B, T, S, E, H = 3, 7, 6, 32, 4
    d = C.make_inputs(500 + PINS.index(name), B, T, S, E, H, torch.float32, bias=name != "nobias")
    if name == "key_is_value":
        d["v"] = d["k"]
    opt = C.make_option(name if "+" in name else "none", d)
    if "float2d" in name:
        assert bool(torch.isinf(opt["oracle"]["attn_mask"]).any())                 # some -inf among the finite values
    _, want = C.oracle_nine(d, opt["oracle"])
    got = C.torch_mha_nine(d, opt["torch"], torch.float64)
    assert set(got) == set(want) and len(want) == (7 if name == "nobias" else 9)
    for n, w in want.items():
        assert bool(torch.isfinite(w).all()), n
    for n, e in C.errors(got, want).items():
        assert e < 1e-12, (name, n, e)
    if name == "key_is_value":
        # one leaf for both: the gradient the caller sees is the sum
        k = d["k"].double().requires_grad_(True)
        mha = torch.nn.MultiheadAttention(E, H, batch_first=True).double()
        with torch.no_grad():
            mha.in_proj_weight.copy_(d["w_in"]); mha.in_proj_bias.copy_(d["b_in"])
            mha.out_proj.weight.copy_(d["w_out"]); mha.out_proj.bias.copy_(d["b_out"])
        y, w = mha(d["q"].double(), k, k, need_weights=True)
        ((y * d["dy"].double()).sum() + (w * d["dwbar"].double()).sum()).backward()
        assert C.errors(dict(dx=k.grad), dict(dx=want["dkey"] + want["dvalue"]))["dx"] < 1e-12


@pytest.mark.parametrize("name", list(C.GEOMETRIES) + list(C.LIMITS))
def test_case_table_has_the_chunking_it_claims(name):
    """A later change of CORE_LDS (or of core_rows) makes the table fail here instead of silently testing one chunk again."""
    B, T, S, E, H, claim = (C.GEOMETRIES.get(name) or C.LIMITS[name])
    assert C.chunking(T, S) == claim, (name, C.chunking(T, S), claim)
    assert E % H == 0 and T <= 4096 and S <= 4096


def test_chunk_height_steps_where_the_table_says():
    assert C.core_rows(4096, 191) == 64 and C.core_rows(4096, 192) == 63
    assert C.core_rows(4096, 4096) == 2 and C.core_lds_bytes(4096, 4096) == 65552      # the largest LDS request
    assert C.core_rows(4096, 4095) == 3 and C.core_rows(4096, 2047) == 6
    assert max(C.core_lds_bytes(4096, S) for S in range(1, 4097)) <= C.CORE_LDS
    multi = [n for n, g_ in C.GEOMETRIES.items() if g_[5][1] > 1]
    assert len(multi) >= 5                                                             # the point of the table


def test_case_table_is_accepted_by_the_library(lib):
    for name in list(C.GEOMETRIES) + list(C.LIMITS):
        B, T, S, E, H, _ = (C.GEOMETRIES.get(name) or C.LIMITS[name])
        for dt in (_lib.AECF_F32, _lib.AECF_BF16, _lib.AECF_F16):
            assert lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(B, T, S, E, H, dt, 0.25))) == 0, (name, dt)
    for T, S in ((4097, 3), (3, 4097)):
        assert lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(2, T, S, 64, 4, _lib.AECF_F32, 0.0))) == -2      # AECF_ERR_UNSUPPORTED
        assert lib.aecf_mha_bwd_workspace_bytes(ctypes.byref(_lib.MhaDesc(2, T, S, 64, 4, _lib.AECF_F32, 0.0))) == 0


@pytest.mark.parametrize("dt", [_lib.AECF_F32, _lib.AECF_BF16, _lib.AECF_F16])
def test_backward_workspace_holds_the_carries_exactly_with_a_second_chunk(lib, dt):
    """T = 64 -> 65 at S = 5 opens the second chunk: the workspace grows by at least the two float32 [B*S, E] carries.
    T = 63 -> 64 stays in one chunk: no such step."""
    B, S, E, H = 6, 5, 64, 4
    ws = lambda T: lib.aecf_mha_bwd_workspace_bytes(ctypes.byref(_lib.MhaDesc(B, T, S, E, H, dt, 0.0)))
    carries = 2 * B * S * E * 4
    assert ws(63) > 0
    assert ws(65) - ws(64) >= carries
    assert 0 <= ws(64) - ws(63) < carries
