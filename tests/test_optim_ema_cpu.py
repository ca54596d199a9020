"""The moving-average entry points (aecf_adamw_mp_ema_step, aecf_ema_update) and FusedAdamW(ema_decay=...)'s host logic,
without a device: symbols, status codes with NULL buffers (argument checks come before anything touches the device),
constructor validation, the state-dict round trip of ``ema``, and an emulation in numpy showing that the bound and the
exact-equality demands of tests/test_optim_ema_gpu.py tell the kernel's rules from each broken one.

Factors measured by the emulation (max |error| / bound; 1 is the bound):
    the kernel's fused form                                   0.99
    e + fl(om fl(w' - e))                                     1.15
    fl(beta e) + fl(om w')                                    1.96
    average taken from the bf16 parameter beside a master     3.5e4   (a weight near 1 whose master moves below half an ulp)
    gradient-less parameter not moved (beta = 0.9)            1.7e7
    average moved on a skipped step / ema_out rounded from w'  exact equality fails in 100 % / 99.9 % of the elements"""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from aecf_amd import _lib
from tests import ema_cases as E

OK, BAD_DIMS, UNSUPPORTED, NULL_POINTER = 0, -1, -2, -3
I64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
I32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
PTRS = lambda *v: (ctypes.c_void_p * len(v))(*v)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ema_step(lib, n, numel, pdt, gdt, *, bufs=None, ticket=None, ema=None, ema_out=None):
    return lib.aecf_adamw_mp_ema_step(n, bufs, bufs, None, bufs, bufs, bufs, numel, pdt, gdt, ticket, 1e-3, 0.9, 0.999, 1e-8, 0.01,
                                      None, None, None, None, None, ema, ema_out, 0.99, None, None)


def _ema_update(lib, n, numel, sdt, odt, *, src=None, ema=None, ema_out=None):
    return lib.aecf_ema_update(n, src, sdt, ema, ema_out, odt, numel, 0.99, None, None, None, None)


def test_new_symbols_in_the_header_and_the_binding():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "aecf_hip.h")) as f:
        header = f.read()
    for name in ("aecf_adamw_mp_ema_step", "aecf_ema_update"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOL_NAMES
        assert getattr(lib, name) is not None
    assert lib.aecf_abi_version() == 10 == _lib.AECF_ABI_VERSION          # entry points only: no bump


def test_adamw_mp_ema_step_status_codes():
    lib = _lib.load()
    assert _ema_step(lib, -1, I64(4), I32(0), I32(0)) == BAD_DIMS
    assert _ema_step(lib, 2, I64(4, -1), I32(0, 0), I32(0, 0)) == BAD_DIMS
    assert _ema_step(lib, 1, I64(4), I32(3), I32(0)) == UNSUPPORTED
    assert _ema_step(lib, 1, I64(4), I32(1), I32(-1)) == UNSUPPORTED
    assert _ema_step(lib, 1, I64(4), I32(2), I32(1)) == NULL_POINTER                                    # arrays NULL
    assert _ema_step(lib, 1, I64(4), I32(2), I32(1), bufs=PTRS(None), ema=PTRS(None)) == NULL_POINTER  # an entry NULL
    # (non-NULL addresses that are never dereferenced: the missing `ema` ARRAY answers first; an ema ENTRY may be NULL)
    assert _ema_step(lib, 1, I64(4), I32(2), I32(1), bufs=PTRS(64), ticket=ctypes.c_void_p(64)) == NULL_POINTER
    assert _ema_step(lib, 1, None, I32(0), I32(0)) == NULL_POINTER
    assert _ema_step(lib, 0, None, None, None) == OK
    assert _ema_step(lib, 3, I64(0, 0, 0), I32(0, 1, 2), I32(1, 1, 0)) == OK        # all empty: no launch, no pointer read


def test_ema_update_status_codes():
    lib = _lib.load()
    assert _ema_update(lib, -1, I64(4), I32(0), I32(0)) == BAD_DIMS
    assert _ema_update(lib, 2, I64(4, -1), I32(0, 0), None) == BAD_DIMS
    assert _ema_update(lib, 1, I64(4), I32(3), None) == UNSUPPORTED
    assert _ema_update(lib, 1, I64(4), I32(1), I32(5), ema_out=PTRS(64)) == UNSUPPORTED
    assert _ema_update(lib, 1, I64(4), I32(1), None, ema_out=PTRS(64)) == NULL_POINTER      # an output without its dtype
    assert _ema_update(lib, 1, I64(4), None, None) == NULL_POINTER
    assert _ema_update(lib, 1, None, I32(1), None) == NULL_POINTER
    assert _ema_update(lib, 1, I64(4), I32(1), None) == NULL_POINTER                        # arrays NULL
    assert _ema_update(lib, 1, I64(4), I32(1), None, src=PTRS(64), ema=PTRS(None)) == NULL_POINTER
    assert _ema_update(lib, 1, I64(4), I32(1), None, src=PTRS(None), ema=PTRS(64)) == NULL_POINTER
    assert _ema_update(lib, 0, None, None, None) == OK
    assert _ema_update(lib, 2, I64(0, 0), I32(0, 2), None) == OK


def test_constructor_validation_of_ema_decay():
    from aecf_amd.optim import EmaModel, FusedAdamW
    p = [torch.zeros(4, requires_grad=True)]
    for bad in (-0.1, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError):
            FusedAdamW(p, ema_decay=bad)
    with pytest.raises(ValueError):
        FusedAdamW(p, ema_decay=torch.tensor(0.9, dtype=torch.float64))
    with pytest.raises(ValueError):
        FusedAdamW(p, ema_decay=torch.tensor([0.9, 0.9]))
    with pytest.raises(TypeError):
        FusedAdamW(p, 1e-3, (0.9, 0.999), 1e-8, 1e-2, False, None, 0.9)            # keyword-only
    assert FusedAdamW(p).ema_decay is None
    for good in (0, 0.0, 1, 0.999):
        assert FusedAdamW(p, ema_decay=good).ema_decay == float(good)
    t = torch.tensor(0.99)
    assert FusedAdamW(p, ema_decay=t).ema_decay is t
    model = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError):
        EmaModel(model, FusedAdamW(model.parameters()))                            # an optimiser without ema_decay
    with pytest.raises(RuntimeError):
        with FusedAdamW(p).ema_weights():
            pass


def test_ema_model_and_the_state_dict_round_trip_on_the_host():
    from aecf_amd.optim import EmaModel, FusedAdamW
    g = torch.Generator().manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3), torch.nn.Linear(3, 2))
    model[2] = model[2].bfloat16()
    frozen = model[0].bias                                                          # not held by the optimiser
    held = [p for p in model.parameters() if p is not frozen]
    opt = FusedAdamW(held, lr=1e-3, master_weights=True, ema_decay=0.99)
    ema = EmaModel(model, opt)
    assert not any(q.requires_grad for q in ema.module.parameters())
    w32, w16 = model[0].weight, model[2].weight
    # float32: the copy's parameter IS the state (same storage, same version counter); 16-bit: an output beside a float32 state
    assert opt.state[w32]["ema"].data_ptr() == ema.module[0].weight.data_ptr()
    assert opt.state[w16]["ema"].dtype == torch.float32 and ema.module[2].weight.dtype == torch.bfloat16
    assert torch.equal(opt.state[w16]["ema"], w16.detach().float()) and opt._ema_out[w16] is ema.module[2].weight
    v = ema.module[0].weight._version
    torch.autograd.graph.increment_version([opt.state[w32]["ema"]])
    assert ema.module[0].weight._version == v + 1
    # what the optimiser does not hold, and the buffers, follow sync()
    with torch.no_grad():
        frozen.add_(1.0)
        model[1].running_mean.add_(2.0)
    assert not torch.equal(ema.module[0].bias, frozen)
    ema.sync()
    assert torch.equal(ema.module[0].bias, frozen) and torch.equal(ema.module[1].running_mean, model[1].running_mean)
    # float32 averages that bf16 cannot hold survive state_dict() -> load_state_dict(), also beside a bf16 parameter
    with torch.no_grad():
        for p in held:
            opt.state[p]["ema"].copy_(torch.randn(p.shape, generator=g) * (1 + 2.0 ** -12))
    keep = copy.deepcopy(opt.state_dict())
    assert not torch.equal(opt.state[w16]["ema"], opt.state[w16]["ema"].bfloat16().float())
    other = FusedAdamW(held, lr=1e-3, master_weights=True, ema_decay=0.99)
    other.load_state_dict(copy.deepcopy(keep))
    for i, p in enumerate(held):
        got = other.state[p]["ema"]
        assert got.dtype == torch.float32 and torch.equal(got, keep["state"][i]["ema"]), i
    # into the optimiser an EmaModel is bound to: the values land IN the bound tensors, outputs included
    with torch.no_grad():
        for p in held:
            opt.state[p]["ema"].zero_()
    opt.load_state_dict(copy.deepcopy(keep))
    assert opt.state[w32]["ema"].data_ptr() == ema.module[0].weight.data_ptr()
    assert torch.equal(ema.module[0].weight, keep["state"][0]["ema"])
    assert torch.equal(ema.module[2].weight, keep["state"][[p is w16 for p in held].index(True)]["ema"].bfloat16())
    # a state without "ema" gets one from the weights at the next step: here only the host part, the state is simply absent
    bare = copy.deepcopy(keep)
    for st in bare["state"].values():
        del st["ema"]
    third = FusedAdamW(held, lr=1e-3, master_weights=True, ema_decay=0.99)
    third.load_state_dict(bare)
    assert all("ema" not in third.state[p] for p in held)
    assert torch.equal(third._ema_state(w16, third.state[w16]), w16.detach().float())
    # ema_weights(): the SAME module on the averages, restored bit for bit
    before = [p.detach().clone() for p in held]
    with opt.ema_weights():
        assert torch.equal(w32, opt.state[w32]["ema"]) and torch.equal(w16, opt.state[w16]["ema"].bfloat16())
    assert all(torch.equal(p, b) for p, b in zip(held, before))
    # several devices are refused
    meta = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2).to("meta"))
    with pytest.raises(ValueError):
        EmaModel(meta, FusedAdamW(meta[0].parameters(), ema_decay=0.5))


def _sweep():
    """beta x magnitude x element: weights around the average at three scales, the differences of a slowly trained model."""
    rng = np.random.default_rng(0)
    for beta in (0.0, 0.3, 0.9, 0.99, 0.999, 0.9999, 0.99999):
        for scale in (1e-3, 1.0, 1e3):
            e = (rng.standard_normal(20000) * scale).astype(np.float32)
            w = (e + rng.standard_normal(20000).astype(np.float32) * np.float32(scale * 10.0 ** rng.integers(-4, 1))).astype(np.float32)
            yield beta, w, e


def test_the_bound_tells_the_fused_form_from_the_others():
    worst = dict(fused=0.0, unfused=0.0, beta_form=0.0)
    for beta, w, e in _sweep():
        for name in worst:
            worst[name] = max(worst[name], E.excess(getattr(E, name)(w, e, beta), w, e, beta))
    print("max |error| / bound:", worst)
    assert worst["fused"] <= 1.0
    assert worst["unfused"] > 1.0 and worst["beta_form"] > 1.0


def test_each_broken_rule_leaves_the_bound_or_the_equality():
    rng = np.random.default_rng(1)
    beta, n = 0.9, 4096
    factors = {}
    # (a) bf16 parameter + master near 1, 50 updates of at most 0.7e-4 (lr = 1e-4) stay below half a bf16 ulp above 1: the parameter's bits stand still
    master = np.ones(n, np.float32)
    e_good = master.copy()
    e_bad = master.copy()
    for _ in range(50):
        master = (master + np.float32(1e-4) * rng.uniform(0.2, 0.7, n).astype(np.float32)).astype(np.float32)
        prev = e_good.copy()
        e_good = E.fused(master, prev, beta)
        assert E.excess(e_good, master, prev, beta) <= 1.0
        e_bad = E.fused(E.bf16_round(master), e_bad, beta)
    assert np.all(E.bf16_round(master) == 1.0) and np.all(e_bad == 1.0) and np.all(e_good > 1.0)
    factors["from_bf16_param"] = E.excess(e_bad, master, prev, beta)
    # (b) a skipped step writes nothing: exact equality with the average before it
    w = rng.standard_normal(n).astype(np.float32)
    e = rng.standard_normal(n).astype(np.float32)
    factors["moved_on_skip_fraction"] = float(np.mean(E.fused(w, e, beta) != e))
    # (c) a parameter without a gradient still moves its average (towards the unchanged weight)
    factors["gradless_not_moved"] = E.excess(e, w, e, beta)
    # (d) the beta form
    factors["beta_form"] = max(E.excess(E.beta_form(w_, e_, b_), w_, e_, b_) for b_, w_, e_ in _sweep())
    # (e) ema_out is the rounding of e', not of w'
    out_good, out_bad = E.bf16_round(E.fused(w, e, beta)), E.bf16_round(w)
    factors["ema_out_from_w_fraction"] = float(np.mean(out_good != out_bad))
    print("broken rules:", factors)
    assert factors["from_bf16_param"] > 100.0
    assert factors["moved_on_skip_fraction"] > 0.9
    assert factors["gradless_not_moved"] > 100.0
    assert factors["beta_form"] > 1.0
    assert factors["ema_out_from_w_fraction"] > 0.9
