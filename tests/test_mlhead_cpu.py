"""CPU-only tests of the fused classifier head: the float64 reference of tests/mlhead_cases.py against autograd through
F.linear + binary_cross_entropy_with_logits in float64; a numpy emulation of the design (float32 z, bfloat16 g in the products,
split-order sums) inside the derived bounds on every case, and outside them -- or breaking an equality -- for every broken rule;
the split counts the table of cases relies on; the aecf_mlhead_* entry points declared, bound and exported with the ABI version
still 10, their workspace answers and their refusals in the documented order before any pointer is read (the pointers handed
over here are bogus)."""
import os
import re

import numpy as np
import pytest

from aecf_amd import _lib
from tests import mlhead_cases as H
from tests import mlloss_cases as M

torch = pytest.importorskip("torch")
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_mlhead_workspace_bytes", "aecf_mlhead_forward", "aecf_mlhead_backward"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
f64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the cases and the reference

def test_the_cases_exercise_the_splits_they_name():
    """flash_split restated: H6 runs 3 CLS splits over the rows, H7 3 ROW splits over the classes and 18 class blocks"""
    for name, (kc, kr, blocks) in H.EXPECTED_SPLITS.items():
        n, C, K = H.CASES[name][:3]
        assert (H.split(C, n).live, H.split(n, C).live, (C + 63) // 64) == (kc, kr, blocks), name
        assert K in H.WIDTHS
    assert H.split(15, 1100) == H.Split(3, 3, 384) and H.split(33, 1100) == H.Split(3, 3, 384)
    assert H.split(4096, 65536) == H.Split(4, 4, 16384) and H.split(65536, 4096).live == 1 and H.split(80, 65536).live == 64
    assert {H.CASES[n][2] for n in H.CASE_IDS} == set(H.WIDTHS)
    assert {H.CASES[n][4] for n in H.CASE_IDS} == {"float32", "bfloat16", "int8", "uint8", "bool"}
    assert {H.CASES[n][5] for n in H.CASE_IDS} == {"none", "some", "row", "class", "all", "specials"}
    assert {H.CASES[n][3] for n in H.CASE_IDS} == {"bce", "bce_w", "bce_soft", "focal", "asl"}


def test_specials_hold_the_named_logits():
    c = H.case("H10")
    z = H.reference(c).z
    for k, want in ((0, "positive"), (1, "negative"), (2, "unknown")):
        seen = {float(v) for v in z[:, k::3].reshape(-1)}
        assert seen == {0.0, 20.0, -20.0, 88.5, -88.5, 104.0, -104.0, 9984.0, -9984.0}, want
    assert not c.valid[:, 2::3].any() and c.valid[:, 0::3].all() and (c.t[:, 0::3] == 1).all() and (c.t[:, 1::3] == 0).all()
    ref = H.reference(c)
    assert np.isfinite(ref.loss) and np.isfinite(ref.dh).all() and np.isfinite(ref.dw).all()


@pytest.mark.parametrize("name", [n for n in H.CASE_IDS if H.CASES[n][3] in ("bce", "bce_w", "bce_soft") and not n.startswith("H10")])
def test_reference_against_torch_autograd(name):
    """z = F.linear in float64, F.binary_cross_entropy_with_logits with weight and pos_weight over the valid elements, autograd
    for all three gradients: within 1e-12.  The scales are formed in float64 here (the float32 fold rounds a = w p once, which
    is no part of the definition)."""
    c = H.case(name)
    if c.pos_weight is not None:
        b64 = c.class_weight.astype(np.float64)
        c = c._replace(a=b64 * c.pos_weight.astype(np.float64), b=b64)
    ref = H.reference(c)
    h = torch.tensor(c.h, dtype=f64, requires_grad=True)
    w = torch.tensor(c.w, dtype=f64, requires_grad=True)
    b = None if c.bias is None else torch.tensor(c.bias, dtype=f64, requires_grad=True)
    valid = torch.tensor(c.valid)
    t = torch.where(valid, torch.tensor(c.t, dtype=f64), torch.zeros((), dtype=f64))
    tp = t * (1.0 - c.form.eps) + c.form.eps / 2
    cw = None if c.class_weight is None else torch.tensor(c.class_weight, dtype=f64)
    pw = None if c.pos_weight is None else torch.tensor(c.pos_weight, dtype=f64)
    el = F.binary_cross_entropy_with_logits(F.linear(h, w, b), tp, weight=cw, pos_weight=pw, reduction="none")
    loss = torch.where(valid, el, torch.zeros((), dtype=f64)).sum() / valid.sum()
    loss.backward()
    assert abs(ref.loss - float(loss.detach())) <= 1e-12
    assert np.abs(ref.dh - h.grad.numpy()).max() <= 1e-12 and np.abs(ref.dw - w.grad.numpy()).max() <= 1e-12
    if b is not None:
        assert np.abs(ref.db - b.grad.numpy()).max() <= 1e-12


def test_reference_of_the_other_forms_against_the_restatement():
    """focal and asymmetric: autograd through mlloss_cases.restate_elements of z = F.linear in float64"""
    for name in ("H2_i8", "H3", "H5"):
        c = H.case(name)
        ref = H.reference(c, "sum")
        h = torch.tensor(c.h, dtype=f64, requires_grad=True)
        w = torch.tensor(c.w, dtype=f64, requires_grad=True)
        b = None if c.bias is None else torch.tensor(c.bias, dtype=f64)
        el = M.restate_elements(F.linear(h, w, b), torch.tensor(c.t, dtype=f64), torch.tensor(c.valid), torch.tensor(c.a, dtype=f64),
                                torch.tensor(c.b, dtype=f64), c.form)
        el.sum().backward()
        assert abs(ref.loss - float(el.sum().detach())) <= 1e-12 * max(1.0, abs(ref.loss))
        assert np.abs(ref.dh - h.grad.numpy()).max() <= 1e-11 and np.abs(ref.dw - w.grad.numpy()).max() <= 1e-11


# ---------------------------------------------------------------------------------------------- emulation and the bounds

def _factor(got, want, bound):
    """largest error over bound; inf where a NaN or an infinity stands at another place than the reference's, or where a
    demanded zero (bound 0) is none"""
    got, want, bound = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (got, want, bound)))
    if not np.array_equal(np.isnan(got), np.isnan(want)) or not np.array_equal(np.isinf(got), np.isinf(want)):
        return float("inf")
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - want[fin])
    if (err[bound[fin] == 0] > 0).any():
        return float("inf")
    return float((err / np.maximum(bound[fin], 1e-300)).max())


def _factors(em, ref):
    return dict(loss=_factor(em["loss"], ref.loss, ref.loss_bound), stats=_factor(em["stats"][0], ref.stats[0], ref.stats_bound),
                dh=_factor(em["dh"], ref.dh, ref.dh_bound), dw=_factor(em["dw"], ref.dw, ref.dw_bound),
                db=_factor(em["db"], ref.db, ref.db_bound),
                counts=0.0 if np.array_equal(em["stats"][1], ref.stats[1]) else float("inf"),
                n_valid=0.0 if em["n_valid"] == ref.n_valid else float("inf"))


@pytest.mark.parametrize("name", H.CASE_IDS)
def test_emulation_is_inside_the_bounds(name):
    c = H.case(name)
    for reduction, upstream in (("mean", 1.0), ("sum", -0.75)):
        ref, em = H.reference(c, reduction, upstream), H.emulate(c, reduction, upstream)
        fs = _factors(em, ref)
        assert max(fs.values()) <= 1.0, (name, reduction, fs)
        H.check_zero(em["dh"], ref.zero_rows, f"{name} dh")
        H.check_zero(em["dw"], ref.zero_classes, f"{name} dW")
        H.check_zero(em["db"], ref.zero_classes, f"{name} dbias")
        if ref.n_valid == 0:
            assert em["loss"] == 0 and not em["dh"].any() and not em["dw"].any() and not em["db"].any() and not em["stats"].any()
    print(f"mlhead emulation {name}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in fs.items()))


def test_broken_rules_leave_the_bounds():
    """Each broken rule, emulated, moves the output RULE_OUTPUT names out of its derived bound or breaks its equality, on the
    case chosen for it here; the unbroken emulation of the same case and upstream stays inside.  The factors (error over
    bound) are printed."""
    tiny = 2.0 ** -126
    plans = {"bias_dropped": ("H2", {}), "bias_per_row": ("H2", {}), "z_bf16": ("H1", {}), "count_ignored": ("H3", {}),
             "ignore_by_product": ("H3", {"nan_at": "unknown"}), "padded_rows_counted": ("H2", {}),
             "scale_before_rounding": ("H2", {"upstream": tiny}), "db_from_rounded_g": ("H1", {}), "targets_transposed": ("H3", {})}
    assert set(plans) == set(H.RULES) == set(H.RULE_OUTPUT)
    factors = {}
    for rule, (name, kw) in plans.items():
        c = H.case(name)
        kw = dict(kw)
        if kw.get("nan_at") == "unknown":
            i, k = np.argwhere(~c.valid & c.valid.any(1)[:, None] & c.valid.any(0)[None, :])[0]
            kw["nan_at"] = (int(i), int(k))
        ref = H.reference(c, "mean", kw.get("upstream", 1.0))
        control = _factors(H.emulate(c, "mean", **kw), ref)
        assert max(control.values()) <= 1.0, (rule, control)
        factors[rule] = _factors(H.emulate(c, "mean", rule=rule, **kw), ref)[H.RULE_OUTPUT[rule]]
    print("mlhead broken-rule factors: " + " ".join(f"{k}={v:.3g}" for k, v in factors.items()))
    for rule, f in factors.items():
        assert f > 1.0, (rule, f)


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU

def test_mlhead_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    assert "#define AECF_ABI_VERSION 10" in header
    make = open(os.path.join(ROOT, "aecf_amd", "csrc", "Makefile")).read()
    assert "aecf_mlhead_flash.hip" in make and "aecf_mlloss_elem.h" in make
    assert '#include "aecf_mlloss_elem.h"' in open(os.path.join(ROOT, "aecf_amd", "csrc", "aecf_mlloss.hip")).read()


def test_workspace_bytes_match_the_documented_layout(lib):
    shapes = sorted({H.CASES[n][:3] for n in H.CASE_IDS} | {(65536, 4096, 512), (65536, 4096, 1024), (65536, 80, 256), (64, 15, 256),
                                                           (64, 65536, 128), ((1 << 31) - 1, 1, 128)})
    for n, C, K in shapes:
        assert lib.aecf_mlhead_workspace_bytes(n, C, K) == H.workspace_layout(n, C, K) > 0, (n, C, K)
    for n, C, K in ((0, 3, 128), (5, 0, 128), (5, 3, 0), (-1, 3, 128), (5, 65537, 128), (1 << 31, 1, 128), (5, 3, 64), (5, 3, 640),
                    (5, 3, 130), (5, 3, 2048)):
        assert lib.aecf_mlhead_workspace_bytes(n, C, K) == 0, (n, C, K)


def _forward(lib, n=64, C=15, K=128, dtype=0, ldtype=1, h=BAD, w=BAD, bias=None, y=BAD, ps=None, ns=None, gp=0.0, gn=0.0, m=0.0,
             eps=0.0, red=0, want=1, st=BAD, tot=BAD, dwu=BAD, dbu=BAD, ws=BAD, wsb=1 << 40):
    return lib.aecf_mlhead_forward(n, C, K, dtype, ldtype, h, w, bias, y, ps, ns, gp, gn, m, eps, red, want, st, tot, dwu, dbu, ws,
                                   wsb, None)


def _backward(lib, n=64, C=15, K=128, dtype=0, ldtype=1, h=BAD, w=BAD, bias=None, y=BAD, ps=None, ns=None, gp=0.0, gn=0.0, m=0.0,
              eps=0.0, red=0, tot=BAD, up=None, factor=1.0, dwu=BAD, dbu=BAD, dhd=0, dh=BAD, dw=BAD, db=BAD, ws=BAD, wsb=1 << 40):
    return lib.aecf_mlhead_backward(n, C, K, dtype, ldtype, h, w, bias, y, ps, ns, gp, gn, m, eps, red, tot, up, factor, dwu, dbu,
                                    dhd, dh, dw, db, ws, wsb, None)


def test_forward_refuses_in_the_documented_order(lib):
    bad = dict(C=70000, dtype=1, h=None, wsb=0)                     # everything after the sizes is wrong too
    assert _forward(lib, n=0, **bad) == BAD_DIMS
    assert _forward(lib, **{**bad, "C": 0}) == BAD_DIMS
    assert _forward(lib, K=0, **bad) == BAD_DIMS
    for opt in (dict(gp=-1.0), dict(gn=float("nan")), dict(gp=float("inf")), dict(m=1.0), dict(m=-0.1), dict(eps=1.0), dict(red=2),
                dict(want=2), dict(want=-1)):
        assert _forward(lib, **bad, **opt) == BAD_DIMS, opt
    assert _forward(lib, C=65537, h=None, wsb=0) == UNSUPPORTED
    assert _forward(lib, n=1 << 31, h=None, wsb=0) == UNSUPPORTED
    for K in (64, 192, 640, 2048):
        assert _forward(lib, K=K, h=None, wsb=0) == UNSUPPORTED, K
    assert _forward(lib, dtype=1, h=None, wsb=0) == UNSUPPORTED      # float32 features
    assert _forward(lib, dtype=2, h=None, wsb=0) == UNSUPPORTED      # float16 features
    assert _forward(lib, ldtype=5, h=None, wsb=0) == UNSUPPORTED
    assert _forward(lib, ldtype=-1, h=None, wsb=0) == UNSUPPORTED
    for name in ("h", "w", "y", "st", "tot", "ws", "dwu", "dbu"):
        assert _forward(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _forward(lib, want=0, dwu=None, dbu=None, wsb=0) == WORKSPACE         # the loss-only pass needs neither
    assert _forward(lib, wsb=H.workspace_layout(64, 15, 128) - 1) == WORKSPACE
    assert _forward(lib, bias=BAD, ps=BAD, ns=BAD, wsb=0) == WORKSPACE           # optional vectors: never read before this


def test_backward_refuses_in_the_documented_order(lib):
    bad = dict(C=70000, dtype=1, tot=None, wsb=0)
    assert _backward(lib, n=-3, **bad) == BAD_DIMS
    for opt in (dict(gn=-0.5), dict(m=float("nan")), dict(eps=-0.1), dict(red=-1), dict(factor=float("nan")), dict(factor=float("inf")),
                dict(K=-128)):
        assert _backward(lib, **bad, **opt) == BAD_DIMS, opt
    assert _backward(lib, C=65537, tot=None, wsb=0) == UNSUPPORTED
    assert _backward(lib, K=320, tot=None, wsb=0) == UNSUPPORTED
    assert _backward(lib, dtype=2, tot=None, wsb=0) == UNSUPPORTED
    assert _backward(lib, dhd=2, tot=None, wsb=0) == UNSUPPORTED     # dh as float16
    assert _backward(lib, ldtype=9, tot=None, wsb=0) == UNSUPPORTED
    for name in ("tot", "h", "w", "y", "ws", "dwu", "dbu"):
        assert _backward(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _backward(lib, wsb=H.workspace_layout(64, 15, 128) - 1) == WORKSPACE
    assert _backward(lib, dh=None, dw=None, db=None, h=None, w=None, y=None, ws=None, dwu=None, dbu=None, wsb=0) == 0   # nothing wanted


def test_python_refuses_cpu_tensors_and_malformed_arguments():
    from aecf_amd import losses
    h, w, y = torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(3, 128, dtype=torch.bfloat16), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.linear_multilabel_loss(h, w, None, y)
    with pytest.raises(ValueError, match="'mean' or 'sum'"):
        losses.MultilabelHead(128, 3, reduction="none")
    with pytest.raises(ValueError, match=r"margin must lie in \[0, 1\)"):
        losses.MultilabelHead(128, 3, margin=1.0)
    with pytest.raises(TypeError, match="takes an nn.Linear"):
        losses.MultilabelHead.from_linear(torch.nn.Conv1d(2, 2, 1))
    torch.manual_seed(3)
    head = losses.MultilabelHead(128, 5, pos_weight=[1.0, 2.0, 3.0, 4.0, 5.0])
    torch.manual_seed(3)
    lin = torch.nn.Linear(128, 5)
    assert set(head.state_dict()) == set(lin.state_dict()) == {"weight", "bias"}
    assert torch.equal(head.weight, lin.weight) and torch.equal(head.bias, lin.bias)          # nn.Linear's initialisation
    shared = losses.MultilabelHead.from_linear(lin, gamma_neg=4.0, margin=0.05)
    assert shared.weight is lin.weight and shared.bias is lin.bias and shared.margin == 0.05
    x = torch.randn(7, 128)
    assert torch.equal(shared(x), lin(x))
    lin.load_state_dict(head.state_dict())
    assert losses.MultilabelHead(128, 5, bias=False).bias is None
