"""CPU-only: that the per-block, per-upstream checks of tests/test_pool_score_gpu.py can see what they are there to see.

tests/pool_score_cases.py restates the shared-query backward in float64 as the kernels arrange it, with a switch per broken rule
(``RULES``).  Here, with no kernel involved:
  * every switch off, the restatement is oracle.mha_backward to 1e-12 on every block and upstream;
  * every broken rule leaves the new bound (error / bound > 1) in at least one block, on every case -- except rule 6, which is
    no error at all: -(log w + 1) de and -(log w) de differ by de, the same for every key of a row, and the softmax backward
    p (dp - sum_m p dp) removes whatever is the same for every key.  The test asserts exactly that (the gradients agree to
    1e-12), so nobody hunts for a lost ``+ 1`` through these tests;
  * rule 7 (``live`` ignored) needs a row on a clamp; a softmax row is never there by more than float32 rounding, so the rule
    runs on weights built for it (``clamped_weights``), on every case with more than one row;
  * which broken rules the whole-tensor BF16_BOUNDS under the combined loss y . dy + wbar . dwbar -- what every other parity
    test of the fused backward asserts -- would have let pass, printed and recorded (``pool_score_old_metric_*``).  Measured,
    at d >= 512: rules 1 and 3 (the whole term missing) pass the old dx and dw_in bounds on every bf16 case, rule 4 passes
    everything, rule 5 passes everything at B >= 37; at d = 128 and d = 256 the term is large enough for the old bounds.  Rule 8
    (5 % of the key term of dx) does NOT pass the old dx bound (6.9e-3 .. 8.6e-3 against 4.5e-3 at d = 512, M = 3) while 2 x
    torch's bf16 error alone (7e-3 .. 9e-3 on dx under dy) would let it through: that is why ``bounds`` keeps the table's entry
    on the whole of dx wherever dy flows;
  * the conditions on the inputs, the route of every case and the ragged last chunk of the kernel it reaches, restated from
    the launchers."""
import ctypes
import os

import pytest
import torch

from tests import pool_score_cases as C
from tests.helpers import record_errors, rel_err

CASE_IDS = list(C.CASES)
BF16_CASES = [c for c in CASE_IDS if C.CASES[c][0] == C.bf16 and C.CASES[c][1] == C.bf16]


@pytest.fixture(scope="module")
def lib():
    from aecf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@pytest.mark.parametrize("case", CASE_IDS)
def test_restatement_is_the_oracle(case):
    M = C.shape(case)[1]
    for up in ("dy", "dwbar", "dent", "both"):
        want = C.reference(case, up)[0]
        got = C.restated_blocks(case, up)
        for n in C.checked_blocks(up, M):
            assert rel_err(got[n], want[n]) < 1e-12, (case, up, n)
        scale = max(float(want[n].abs().max()) for n in ("dw_in.q", "db_in.q"))
        assert float(got["db_in.k"].abs().max()) < 1e-12 * scale and float(want["db_in.k"].abs().max()) < 1e-12 * scale
        if up in ("dwbar", "dent"):
            for n in C.ZERO_WITHOUT_DY:
                assert float(want[n].abs().max()) == 0.0 and float(got[n].abs().max()) == 0.0, (case, up, n)


@pytest.mark.parametrize("case", CASE_IDS)
def test_route_and_ragged_last_chunk(lib, case):
    from aecf_amd import _lib
    adt, pdt, B, M, E, H, route = C.CASES[case]
    assert C.expected_route(case) == route
    code = {C.bf16: _lib.AECF_BF16, C.f16: _lib.AECF_F16, C.f32: _lib.AECF_F32}[adt]
    desc = _lib.PoolDesc(B, M, E, H, code, 0, 1, 0.15, 0.7, 1e-8)
    assert lib.aecf_pool_check(ctypes.byref(desc)) == 0
    # the forward saves no V exactly where dsu_ws_kernel takes the shape.  One hi / lo case shares that answer and still runs
    # bwd_g: d = 512 with M = 4, where the kernel has no room for the low tiles (160 256 of 163 840 bytes without them)
    takes = adt == C.bf16 and C.dsu_ws_takes(M, E, H)
    assert (lib.aecf_pool_wants_saved_v(ctypes.byref(desc)) == 0) == takes
    assert takes == (route.startswith("dsu_ws") or case == "bwdg_master_B37_M4_E512_H8")
    if case == "bwdg_master_B37_M4_E512_H8":
        assert not C.dsu_ws_takes(M, E, H, lo=True) and C.dsu_ws_smem(E, M, E // H, False) == 160256
    hilo = lib.aecf_pool_hilo_bwd_workspace_bytes(ctypes.byref(desc)) > 0 and adt == C.bf16
    assert (hilo and C.is_master(case)) == (route in ("dsu_ws_lo", "bwd_g"))
    if C.is_master(case):
        assert hilo                                        # the tight table is the one that applies (helpers.f32grad_bounds)
    rows, n, last = C.score_chunking(case)
    if case in ("dsv_bf16_B300_M3_E128_H4", "dsv_f32_B300_M4_E128_H4"):
        # 300 = 75 blocks of 4 waves: dscore_v_kernel's last block is full.  The batch is ragged for the dx kernel of these
        # shapes (bwd_g_kernel, 128 samples per block: 128 + 128 + 44), which reads the ds written here
        assert last == rows == 4 and B % C.G_SAMPLES != 0
    else:
        assert 0 < last < rows, (case, rows, n, last)
    if route.startswith("dsu_ws"):
        assert rows % 16 == 0 and (last % 16 != 0 or B == 2100 and last == 20)      # a tail inside a 16-row step
    if case == "dsu_bf16_B2100_M3_E512_H8":
        assert (rows, n, last) == (32, 66, 20)              # two 16-row steps per block; 16 + 4 rows in the last


@pytest.mark.parametrize("case", CASE_IDS)
def test_input_conditions(case):
    adt, pdt, B, M, E, H, _ = C.CASES[case]
    for up in C.UPSTREAMS + ("both",):
        want, bnd, ref = C.reference(case, up)
        for n in bnd:
            assert float(want[n].abs().max()) > 0.0, (case, up, n)
        if ref is not None:
            for n, e in ref.items():
                assert e <= 2e-2, (case, up, n, e)          # torch's own error: no bound beyond 4e-2
        assert max(bnd.values()) <= 4e-2
    for kpm in (True,) if case in C.KPM_CASES else ():
        want, bnd, ref = C.reference(case, "dwbar", kpm)
        assert all(float(want[n].abs().max()) > 0.0 for n in bnd) and max(ref.values()) <= 2e-2
        frac = float(C.inputs(case)["kpm"].double().mean())
        assert 0.1 < frac < 0.4 and not bool(C.inputs(case)["kpm"][:, 0].any())
    qs = C.dent_scale(case)
    assert 8.0 <= qs <= 64.0
    w = C.forward(case, qs)["wbar"]
    lo, hi = C.DENT_SPREAD.get(case, (0.1, 0.5))
    assert float(w.min()) <= lo and float(w.max()) >= hi, (case, float(w.min()), float(w.max()))
    assert float(C.clamp_distance(w.float().double()).min()) > 1e-4       # no row near a clamp: ``live`` is true in any precision
    x = C.inputs(case, qs)["x"]
    assert float((x != C.inputs(case, 1.0)["x"]).any(-1).any(-1).double().mean()) <= 0.1      # rows replaced to get there: a few


def _ratios(got, want, bnd):
    return {n: rel_err(got[n], want[n]) / b for n, b in bnd.items()}


@pytest.mark.parametrize("case", CASE_IDS)
def test_broken_rules_leave_the_bounds(case):
    B, M = C.shape(case)[:2]
    worst = {}
    for rule, up in C.RULE_UPSTREAM.items():
        if rule == 7:
            if B == 1:
                continue                                    # its only row cannot be both clamped and the scale of the blocks
            w = C.forward(case, C.dent_scale(case))["wbar"].float().double().reshape(B, M)
            w_ent, rows = C.clamped_weights(w)
            assert float(C.clamp_distance(w_ent)[rows].max()) < 0.0 and len(rows) >= 1
            want = C.truth(case, "dent", w_kernel=w_ent)
            bnd, _ = C.bounds(case, "dent", want, w_kernel=w_ent)
            assert all(float(want[n].abs().max()) > 0.0 for n in bnd)
            assert max(_ratios(C.restated_blocks(case, "dent", None, w_ent), want, bnd).values()) < 1e-9
            r = _ratios(C.restated_blocks(case, "dent", 7, w_ent), want, bnd)
        else:
            want, bnd, _ = C.reference(case, up)
            r = _ratios(C.restated_blocks(case, up, rule), want, bnd)
        n = max(r, key=r.get)
        worst[rule] = r[n]
        print("%s rule %d (%s): largest error / bound %.3g in %s" % (case, rule, C.RULES[rule], r[n], n))
        if rule == 6:
            # the same for every key of a row: the softmax backward removes it (module docstring)
            want, _, _ = C.reference(case, "dent")
            got = C.restated_blocks(case, "dent", 6)
            assert max(rel_err(got[k], want[k]) for k in C.checked_blocks("dent", M)) < 1e-12
        else:
            assert r[n] > 1.0, (case, rule, C.RULES[rule], r)
    record_errors("pool_score_rules_" + case, **{"rule%d" % k: v for k, v in worst.items()})


def test_what_the_whole_tensor_bounds_let_pass():
    passed = {}
    for case in BF16_CASES:
        for rule in (1, 2, 3, 4, 5, 8):                    # (6 and 7 need the entropy upstream, which that loss does not have)
            e = C.old_metric_errors(case, rule)
            changed = {n: v for n, v in e.items() if v > 0.0}
            assert changed, (case, rule)
            ok = sorted(n for n, v in changed.items() if v < C.OLD_BOUNDS[n])
            print("%s rule %d: %s | passes the old bound: %s" % (
                case, rule, " ".join("%s %.2e/%.1e" % (n, v, C.OLD_BOUNDS[n]) for n, v in changed.items()), ", ".join(ok) or "-"))
            record_errors("pool_score_old_metric_%s_rule%d" % (case, rule), **{n: v / C.OLD_BOUNDS[n] for n, v in changed.items()})
            passed[case, rule] = (ok, sorted(changed))
    assert any(ok for ok, _ in passed.values())
    for case in BF16_CASES:
        B, M, E, H = C.shape(case)
        if E < 512:
            continue            # (d = 128 and d = 256: the term is 0.5 % .. 0.8 % of dx and the old bounds do see it go)
        assert passed[case, 4][0] == passed[case, 4][1] == ["dx"]           # nothing anywhere notices rule 4
        for rule in (1, 3):                                                 # the whole term missing from dx and from dw_in
            assert {"dx", "dw_in"} <= set(passed[case, rule][0]), (case, rule, passed[case, rule])
        if (M, E) == (3, 512):
            # ... and the one rule the old bound on dx is the tighter yardstick for
            assert "dx" not in passed[case, 8][0]
