"""Bit fingerprints of the contrastive kernels: a fixed list of cases with seeded inputs through the C ABI, one sha256 per output
tensor.  Two builds of the library compute the same bits where every line of their outputs is equal; run once per library,
each in a fresh process (AECF_LIB_PATH selects the build, tools/build_variant.sh):

    python tools/flash_bits.py > new.txt
    AECF_LIB_PATH=aecf_amd/lib/var/NAME/libaecf_hip.so python tools/flash_bits.py > other.txt

Cases (rows, cols, row_offset, d):
  InfoNCE streaming form (aecf_nce_fwd_bwd / _dt with d_t on the O(rows d) workspace; the tool checks that this workspace is
  smaller than the tile form's, so the streaming form is what runs): one block, ragged rows and columns, three key splits with
  a ragged last one, a split rule that leaves an empty split, the column-split widths 768 and 1024; aecf_loss_fwd_bwd / _dt once
  with the entropy regulariser riding (300 entries, a NaN, +inf and -inf among them, d_entropy requested).
  Sigmoid streaming form (aecf_sig_stream_fwd_bwd), full call and loss-only.
  Tile-GEMM forms: symmetric InfoNCE pass1 / loss (with the entropy rider) / grads, host and device temperature; sigmoid pass1 /
  grads with d_t; aecf_retrieval_positive / _ranks with column counts.
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib  # noqa: E402
from aecf_amd.layer import _ptr, _stream  # noqa: E402

NCE_STREAM = [(1, 1, 0, 128), (100, 333, 57, 256), (70, 1100, 37, 128), (512, 16385, 0, 128), (97, 1500, 3, 768),
              (64, 700, 600, 1024)]
ENTROPY_CASE = (70, 1100, 37, 128)
SIG_STREAM = [(1, 1, 0, 128), (70, 1100, 37, 128), (257, 300, 43, 128), (70, 130, 37, 768), (70, 130, 37, 1024)]
TILE = [(257, 300, 43, 128), (640, 2048, 1000, 512)]
RANKS = [(257, 300, 43, 128)]
T, MIN_T, BIAS = 0.07, 0.025, -10.0


def main():
    if not torch.cuda.is_available():
        raise SystemExit("flash_bits: no GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    bf16 = dict(dtype=torch.bfloat16, device=dev)

    def views(rows, cols, off, d):
        g = torch.Generator().manual_seed(1000 * rows + 10 * cols + d)
        nrm = lambda t: (t / t.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
        a, b = nrm(torch.randn(rows, d, generator=g)), nrm(torch.randn(cols, d, generator=g))
        b[off:off + rows] = nrm(0.8 * a.float() + 0.6 * b[off:off + rows].float())        # real positives
        return a.to(dev).contiguous(), b.to(dev).contiguous()

    def entropy():
        e = torch.rand(300, generator=torch.Generator().manual_seed(7)) * 1.2
        e[5], e[77], e[200] = float("nan"), float("inf"), float("-inf")
        return e.to(dev)

    def show(tag, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            print(f"{tag} {name} {hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()}", flush=True)

    def zeros_ws(n):
        return torch.zeros(n, dtype=torch.uint8, device=dev)

    t_dev, bias_dev, up = torch.full((1,), T, **f32), torch.full((1,), BIAS, **f32), torch.full((1,), 0.75, **f32)

    for case in NCE_STREAM:
        rows, cols, off, d = case
        q, k = views(*case)
        n = lib.aecf_nce_stream_workspace_bytes(rows, cols, d, _lib.AECF_BF16)
        assert 0 < n < lib.aecf_nce_sym_workspace_bytes(rows, cols, d), "the streaming workspace would select the tile form"
        coef = 0.5 / cols
        for dt in (False, True):
            loss, dq, dk, d_t = torch.zeros(rows, **f32), torch.zeros(rows, d, **f32), torch.zeros(cols, d, **f32), torch.zeros(1, **f32)
            ws = zeros_ws(n)
            if dt:
                _lib.check(lib.aecf_nce_fwd_bwd_dt(rows, cols, off, d, _lib.AECF_BF16, _ptr(t_dev), MIN_T, coef, _ptr(q), _ptr(k),
                                                   _ptr(loss), _ptr(dq), _ptr(dk), _ptr(d_t), _ptr(ws), n, _stream()), "nce_fwd_bwd_dt")
                show(f"nce_stream_dt {case}", loss_rows=loss, dq=dq, dk=dk, d_t=d_t)
            else:
                _lib.check(lib.aecf_nce_fwd_bwd(rows, cols, off, d, _lib.AECF_BF16, T, coef, _ptr(q), _ptr(k), _ptr(loss), _ptr(dq),
                                                _ptr(dk), _ptr(ws), n, _stream()), "nce_fwd_bwd")
                show(f"nce_stream {case}", loss_rows=loss, dq=dq, dk=dk)
            if case != ENTROPY_CASE:
                continue
            ent = entropy()
            loss, dq, dk, d_t = torch.zeros(rows, **f32), torch.zeros(rows, d, **f32), torch.zeros(cols, d, **f32), torch.zeros(1, **f32)
            el, de = torch.zeros(1, **f32), torch.zeros(300, **f32)
            ws = zeros_ws(n)
            if dt:
                _lib.check(lib.aecf_loss_fwd_bwd_dt(rows, cols, off, d, _ptr(t_dev), MIN_T, coef, _ptr(q), _ptr(k), _ptr(loss), _ptr(dq),
                                                    _ptr(dk), _ptr(d_t), 300, 3, 0.7, _ptr(ent), 1.0, _ptr(el), _ptr(de), _ptr(ws), n,
                                                    _stream()), "loss_fwd_bwd_dt")
                show(f"nce_stream_entropy_dt {case}", loss_rows=loss, dq=dq, dk=dk, d_t=d_t, ent_loss=el, d_ent=de)
            else:
                _lib.check(lib.aecf_loss_fwd_bwd(rows, cols, off, d, T, coef, _ptr(q), _ptr(k), _ptr(loss), _ptr(dq), _ptr(dk), 300, 3,
                                                 0.7, _ptr(ent), 1.0, _ptr(el), _ptr(de), _ptr(ws), n, _stream()), "loss_fwd_bwd")
                show(f"nce_stream_entropy {case}", loss_rows=loss, dq=dq, dk=dk, ent_loss=el, d_ent=de)

    for case in SIG_STREAM:
        rows, cols, off, d = case
        a, b = views(*case)
        n = lib.aecf_sig_stream_workspace_bytes(rows, cols, d)
        assert n > 0
        loss, d_bias, d_t = torch.zeros(rows, **f32), torch.zeros(1, **f32), torch.zeros(1, **f32)
        da, db = torch.zeros(rows, d, **f32), torch.zeros(cols, d, **f32)
        ws = zeros_ws(n)
        _lib.check(lib.aecf_sig_stream_fwd_bwd(rows, cols, off, d, _ptr(t_dev), MIN_T, _ptr(bias_dev), 1.0 / cols, _ptr(a), _ptr(b),
                                               _ptr(loss), _ptr(d_bias), _ptr(d_t), _ptr(da), _ptr(db), _ptr(ws), n, _stream()),
                   "sig_stream_fwd_bwd")
        show(f"sig_stream {case}", loss_rows=loss, d_bias=d_bias, d_t=d_t, da=da, db=db)
        loss, ws = torch.zeros(rows, **f32), zeros_ws(n)
        _lib.check(lib.aecf_sig_stream_fwd_bwd(rows, cols, off, d, _ptr(t_dev), MIN_T, _ptr(bias_dev), 1.0 / cols, _ptr(a), _ptr(b),
                                               _ptr(loss), None, None, None, None, _ptr(ws), n, _stream()), "sig_stream loss only")
        show(f"sig_stream_loss_only {case}", loss_rows=loss)

    for case in TILE:
        rows, cols, off, d = case
        a, b = views(*case)
        ent = entropy()
        n = lib.aecf_nce_sym_workspace_bytes(rows, cols, d)
        coef = 0.5 / cols
        for dt in (False, True):
            ws, cs, loss = zeros_ws(n), torch.zeros(cols, **f32), torch.zeros(rows, **f32)
            el, de, d_t = torch.zeros(1, **f32), torch.zeros(300, **f32), torch.zeros(1, **f32)
            if dt:
                da, db = torch.zeros(rows, d, **bf16), torch.zeros(cols, d, **bf16)
                _lib.check(lib.aecf_nce_sym_pass1_dt(rows, cols, d, _ptr(t_dev), MIN_T, _ptr(a), _ptr(b), _ptr(ws), n, _ptr(cs),
                                                     _stream()), "sym_pass1_dt")
                _lib.check(lib.aecf_nce_sym_loss_dt(rows, cols, off, d, _ptr(t_dev), MIN_T, _ptr(a), _ptr(b), _ptr(cs), _ptr(ws), n,
                                                    _ptr(loss), 300, 3, 0.7, _ptr(ent), 1.0, _ptr(el), _ptr(de), _stream()), "sym_loss_dt")
                _lib.check(lib.aecf_nce_sym_grads_dt(rows, cols, off, d, _ptr(t_dev), MIN_T, coef, _ptr(a), _ptr(b), _ptr(ws), n, _ptr(up),
                                                     _lib.AECF_BF16, _ptr(da), _ptr(db), _ptr(d_t), _stream()), "sym_grads_dt")
                show(f"nce_sym_dt {case}", col_sums=cs, loss_rows=loss, ent_loss=el, d_ent=de, da=da, db=db, d_t=d_t)
            else:
                da, db = torch.zeros(rows, d, **f32), torch.zeros(cols, d, **f32)
                _lib.check(lib.aecf_nce_sym_pass1(rows, cols, d, T, _ptr(a), _ptr(b), _ptr(ws), n, _ptr(cs), _stream()), "sym_pass1")
                _lib.check(lib.aecf_nce_sym_loss(rows, cols, off, d, T, _ptr(a), _ptr(b), _ptr(cs), _ptr(ws), n, _ptr(loss), 300, 3, 0.7,
                                                 _ptr(ent), 1.0, _ptr(el), _ptr(de), _stream()), "sym_loss")
                _lib.check(lib.aecf_nce_sym_grads(rows, cols, off, d, T, coef, _ptr(a), _ptr(b), _ptr(ws), n, None, _lib.AECF_F32,
                                                  _ptr(da), _ptr(db), _stream()), "sym_grads")
                show(f"nce_sym {case}", col_sums=cs, loss_rows=loss, ent_loss=el, d_ent=de, da=da, db=db)
        n = lib.aecf_sig_workspace_bytes(rows, cols, d)
        ws, loss, d_bias, d_t = zeros_ws(n), torch.zeros(rows, **f32), torch.zeros(1, **f32), torch.zeros(1, **f32)
        da, db = torch.zeros(rows, d, **f32), torch.zeros(cols, d, **f32)
        _lib.check(lib.aecf_sig_pass1(rows, cols, off, d, _ptr(t_dev), MIN_T, _ptr(bias_dev), _ptr(a), _ptr(b), _ptr(ws), n, _ptr(loss),
                                      _ptr(d_bias), _stream()), "sig_pass1")
        _lib.check(lib.aecf_sig_grads(rows, cols, off, d, _ptr(t_dev), MIN_T, 1.0 / cols, _ptr(a), _ptr(b), _ptr(ws), n, _ptr(up),
                                      _lib.AECF_F32, _ptr(da), _ptr(db), _ptr(d_t), _stream()), "sig_grads")
        show(f"sig_tile {case}", loss_rows=loss, d_bias=d_bias, da=da, db=db, d_t=d_t)

    for case in RANKS:
        rows, cols, off, d = case
        a, b = views(*case)
        n = lib.aecf_retrieval_workspace_bytes(rows, cols, d)
        assert n > 0
        i32 = dict(dtype=torch.int32, device=dev)
        pos, pos_col = torch.zeros(rows, **f32), (b.float() * b.float().roll(1, 0)).sum(1).contiguous()
        _lib.check(lib.aecf_retrieval_positive(rows, cols, off, d, _ptr(a), _ptr(b), _ptr(pos), _stream()), "retrieval_positive")
        pos_col[off:off + rows] = pos
        rg, re, cg, ce = torch.zeros(rows, **i32), torch.zeros(rows, **i32), torch.zeros(cols, **i32), torch.zeros(cols, **i32)
        ws = zeros_ws(n)
        _lib.check(lib.aecf_retrieval_ranks(rows, cols, off, d, _ptr(a), _ptr(b), _ptr(pos), _ptr(pos_col), _ptr(rg), _ptr(re), _ptr(cg),
                                            _ptr(ce), _ptr(ws), n, _stream()), "retrieval_ranks")
        show(f"retrieval {case}", pos_row=pos, row_greater=rg, row_equal=re, col_greater=cg, col_equal=ce)


if __name__ == "__main__":
    main()
