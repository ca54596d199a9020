"""The mixed-precision optimiser entry points (aecf_adamw_mp_step, aecf_grad_norm) and FusedAdamW's host logic, without a
device: symbols, status codes with NULL buffers (argument checks come before anything touches the device), constructor
validation and the float32 state that load_state_dict must not cast."""
import copy
import ctypes

import pytest
import torch

from aecf_amd import _lib

OK, BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = 0, -1, -2, -3, -4
I64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
I32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
PTRS = lambda *v: (ctypes.c_void_p * len(v))(*v)


def _mp_step(lib, n, numel, pdt, gdt, *, bufs=None, ticket=None):
    return lib.aecf_adamw_mp_step(n, bufs, bufs, None, bufs, bufs, bufs, numel, pdt, gdt, ticket, 1e-3, 0.9, 0.999, 1e-8, 0.01,
                                  None, None, None, None, None, None)


def _norm(lib, n, numel, gdt, *, grads=None, workspace=None, workspace_bytes=0, out=None):
    return lib.aecf_grad_norm(n, grads, gdt, numel, 1.0, None, workspace, workspace_bytes, out, None)


def test_new_symbols_load_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("aecf_adamw_mp_step", "aecf_grad_norm_workspace_bytes", "aecf_grad_norm"):
        assert name in _lib.SYMBOL_NAMES
        assert getattr(lib, name) is not None
    assert lib.aecf_abi_version() == 10 == _lib.AECF_ABI_VERSION


def test_adamw_mp_step_status_codes():
    lib = _lib.load()
    assert _mp_step(lib, -1, I64(4), I32(0), I32(0)) == BAD_DIMS
    assert _mp_step(lib, 2, I64(4, -1), I32(0, 0), I32(0, 0)) == BAD_DIMS
    assert _mp_step(lib, 1, I64(4), I32(3), I32(0)) == UNSUPPORTED
    assert _mp_step(lib, 1, I64(4), I32(1), I32(-1)) == UNSUPPORTED
    assert _mp_step(lib, 1, I64(4), I32(2), I32(1)) == NULL_POINTER                    # arrays NULL
    assert _mp_step(lib, 1, I64(4), I32(2), I32(1), bufs=PTRS(None)) == NULL_POINTER  # an entry NULL
    assert _mp_step(lib, 1, None, I32(0), I32(0)) == NULL_POINTER
    assert _mp_step(lib, 0, None, None, None) == OK
    assert _mp_step(lib, 3, I64(0, 0, 0), I32(0, 1, 2), I32(1, 1, 0)) == OK            # all empty: no launch, no pointer read


def test_grad_norm_status_codes():
    lib = _lib.load()
    assert _norm(lib, -1, I64(4), I32(0)) == BAD_DIMS
    assert _norm(lib, 1, I64(-4), I32(0)) == BAD_DIMS
    assert _norm(lib, 1, I64(4), I32(7)) == UNSUPPORTED
    assert _norm(lib, 1, I64(4), I32(1)) == NULL_POINTER
    assert _norm(lib, 1, I64(4), I32(1), grads=PTRS(None), out=ctypes.c_void_p(64)) == NULL_POINTER
    # (non-NULL addresses that are never dereferenced: the workspace check answers first)
    assert _norm(lib, 1, I64(10000), I32(1), grads=PTRS(64), workspace=ctypes.c_void_p(64), workspace_bytes=4,
                 out=ctypes.c_void_p(64)) == WORKSPACE
    assert _norm(lib, 0, None, None) == OK
    assert _norm(lib, 2, I64(0, 0), I32(0, 2)) == OK


def test_grad_norm_workspace_grows_with_the_block_count():
    lib = _lib.load()
    ws = lib.aecf_grad_norm_workspace_bytes
    assert ws(0, None) == 0
    assert ws(1, I64(1)) > 0
    assert ws(1, I64(1)) % 4 == 0
    small, large = ws(1, I64(1 << 12)), ws(1, I64(1 << 24))
    assert 0 < small < large
    assert ws(2, I64(1 << 24, 1 << 24)) == 2 * large
    assert ws(3, I64(1, 1, 1)) == 3 * ws(1, I64(1))                # one partial per block, a block never spans tensors


def test_constructor_validation():
    from aecf_amd.optim import FusedAdamW
    p = [torch.zeros(4, requires_grad=True)]
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError):
            FusedAdamW(p, max_grad_norm=bad)
    with pytest.raises(ValueError):
        FusedAdamW(p, lr=torch.tensor(1e-3, dtype=torch.float64))
    with pytest.raises(ValueError):
        FusedAdamW(p, lr=torch.tensor([1e-3, 1e-3]))
    with pytest.raises(ValueError):
        FusedAdamW(p, lr=-1.0)
    opt = FusedAdamW(p, lr=torch.tensor(1e-3), master_weights=True, max_grad_norm=2)
    assert opt.master_weights and opt.max_grad_norm == 2.0 and opt._step_supports_amp_scaling


def test_load_state_dict_keeps_float32_state_of_a_bf16_parameter():
    from aecf_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(11)
    p = torch.randn(33, 5, generator=g).bfloat16().requires_grad_()
    q = torch.randn(7, generator=g).requires_grad_()                               # a float32 parameter beside it
    opt = FusedAdamW([p, q], lr=1e-3, master_weights=True)
    # float32 values that bf16 cannot hold
    state = {0: dict(step=torch.tensor(3.0), master=torch.randn(33, 5, generator=g) * (1 + 2.0 ** -12),
                     exp_avg=torch.randn(33, 5, generator=g), exp_avg_sq=torch.rand(33, 5, generator=g)),
             1: dict(step=torch.tensor(3.0), exp_avg=torch.randn(7, generator=g), exp_avg_sq=torch.rand(7, generator=g))}
    assert not torch.equal(state[0]["master"], state[0]["master"].bfloat16().float())
    sd = dict(state=state, param_groups=copy.deepcopy(opt.state_dict()["param_groups"]))
    keep = copy.deepcopy(sd)
    opt.load_state_dict(sd)
    for key in ("master", "exp_avg", "exp_avg_sq"):
        got = opt.state[p][key]
        assert got.dtype == torch.float32 and torch.equal(got, keep["state"][0][key]), key
        assert got.data_ptr() != sd["state"][0][key].data_ptr()                    # a copy, as load_state_dict makes
    assert float(opt.state[p]["step"]) == 3.0
    assert torch.equal(opt.state[q]["exp_avg"], keep["state"][1]["exp_avg"]) and "master" not in opt.state[q]
    # and back out: the round trip through state_dict() is bit-identical
    again = FusedAdamW([p, q], lr=1e-3, master_weights=True)
    again.load_state_dict(copy.deepcopy(opt.state_dict()))
    for key in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(again.state[p][key], keep["state"][0][key])
    # the step itself still refuses CPU tensors
    p.grad = torch.zeros_like(p)
    q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError):
        opt.step()
