"""Retrieval ranks of the contrastive views: losses.retrieval_ranks / retrieval_metrics and the C ABI behind them
(aecf_retrieval_positive / aecf_retrieval_ranks).

Two yardsticks, both float64 torch on the rows the kernels read:
  * integer-valued bf16 rows (entries in {-2..2}): every dot product is an integer far below 2^24, float32 accumulation is exact
    in any order, so the greater / equal counts must match float64 bit for bit;
  * unit-norm random rows: two float32 dot products of unit vectors are each within d 2^-24 of exact, so with eps = d 2^-23 the
    kernel's greater is at least #{s > pos + eps} and its greater + equal at most #{s > pos - eps}."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# rows, cols, d, row_offset, p
CASES = [(300, 1000, 128, 200, 0.1), (257, 513, 64, 256, 0.1), (64, 320, 1024, 256, 0.05)]
BIG = (4096, 8192, 64, 2048, 0.1)       # 16 x 32 output tiles: more than the 256 CUs hold at one block each
_cache = {}


def _int_views(cols, d, p, seed=7):
    """b [cols, d] and its partner view a_full [cols, d] (row i of one is the positive of row i of the other), entries uniform
    in {-2..2}; the partner copies an entry with probability p, so positives score high and ties are common."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(-2, 3, (cols, d), generator=g)
    a = torch.randint(-2, 3, (cols, d), generator=g)
    a = torch.where(torch.rand(cols, d, generator=g) < p, b, a)
    return a.to(torch.bfloat16).to(DEV), b.to(torch.bfloat16).to(DEV)


def _ref_counts(a, b, off, pos_col, lo=None, hi=None):
    """float64 counts for rows a [R, d] (positives at off + i) against b [C, d]: row greater / equal against the row's own
    positive, column greater / equal against pos_col [C] (float64), the positive excluded from both.  lo / hi widen the
    comparison into a band (test 2): greater counts s > pos + hi-shift etc. are formed by the caller from two calls."""
    s = a.double() @ b.double().T
    rows, cols = s.shape
    i = torch.arange(rows, device=s.device)
    is_pos = torch.zeros_like(s, dtype=torch.bool)
    is_pos[i, off + i] = True
    pr = s[i, off + i][:, None]
    pc = pos_col.double()[None, :]
    other = ~is_pos
    return dict(rg=((s > pr) & other).sum(1), re=((s == pr) & other).sum(1), cg=((s > pc) & other).sum(0), ce=((s == pc) & other).sum(0),
                s=s, other=other, pr=pr, pc=pc)


def _positive(a, b, off):
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    pos = torch.empty(a.shape[0], dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().aecf_retrieval_positive(a.shape[0], b.shape[0], off, a.shape[1], _ptr(a), _ptr(b), _ptr(pos), _stream()),
               "aecf_retrieval_positive")
    return pos


def _ranks_call(a, b, off, pos_row, pos_col, guard=0):
    """aecf_retrieval_ranks with exactly the workspace it asks for; guard > 0 puts that many 0xA5 bytes behind the workspace and
    behind every output (returned as `guards`)."""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    rows, d = a.shape
    cols = b.shape[0]
    wsb = lib.aecf_retrieval_workspace_bytes(rows, cols, d)
    assert wsb > 0
    ws = torch.full((wsb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    g4 = guard // 4
    fill = torch.tensor([0xA5A5A5A5 - (1 << 32)], dtype=torch.int64).to(torch.int32).item()
    out = {k: torch.full((n + g4,), fill, dtype=torch.int32, device=DEV) for k, n in (("rg", rows), ("re", rows), ("cg", cols), ("ce", cols))}
    _lib.check(lib.aecf_retrieval_ranks(rows, cols, off, d, _ptr(a), _ptr(b), _ptr(pos_row), _ptr(pos_col), _ptr(out["rg"]),
                                        _ptr(out["re"]), _ptr(out["cg"]) if pos_col is not None else None,
                                        _ptr(out["ce"]) if pos_col is not None else None, _ptr(ws), wsb, _stream()),
               "aecf_retrieval_ranks")
    torch.cuda.synchronize()
    res = {k: v[:n] for (k, v), n in zip(out.items(), (rows, rows, cols, cols))}
    res["guards"] = [ws[wsb:]] + [v[n:].view(torch.uint8) for (k, v), n in zip(out.items(), (rows, rows, cols, cols))]
    return res


def _case(idx):
    """Inputs, thresholds and float64 counts of an integer case, computed once."""
    if idx not in _cache:
        rows, cols, d, off, p = BIG if idx == "big" else CASES[idx]
        a_full, b = _int_views(cols, d, p)
        a = a_full[off:off + rows].contiguous()
        pos_col = _positive(a_full, b, 0)
        ref = _ref_counts(a, b, off, pos_col)
        want = {k: ref[k].to(torch.int32) for k in ("rg", "re", "cg", "ce")}
        _cache[idx] = dict(a_full=a_full, a=a, b=b, off=off, pos_col=pos_col, want=want, smax=float(ref["s"].abs().max()))
    return _cache[idx]


@pytest.mark.parametrize("idx", [0, 1, 2, "big"])
def test_integer_rows_give_the_float64_counts_bit_for_bit(idx):
    c = _case(idx)
    a, b, off, want = c["a"], c["b"], c["off"], c["want"]
    # the reference itself exercises both counters and a spread of ranks
    tied = float((want["re"] > 0).float().mean())
    med = float(want["rg"].float().median())
    print(f"retrieval exact {tuple(a.shape)} x {b.shape[0]}: |s| <= {c['smax']:.0f}, rows with a tie {100 * tied:.0f} %, median greater {med:.0f}")
    assert c["smax"] < 2 ** 24 and tied >= 0.10 and med > 0
    pos_row = _positive(a, b, off)
    assert torch.equal(pos_row.double(), (a.double() * b[off:off + a.shape[0]].double()).sum(1))
    assert torch.equal(pos_row, c["pos_col"][off:off + a.shape[0]])
    got = _ranks_call(a, b, off, pos_row, c["pos_col"])
    for k in ("rg", "re", "cg", "ce"):
        assert torch.equal(got[k], want[k]), k
    # the column direction off: the same row counts, the column outputs untouched
    rows_only = _ranks_call(a, b, off, pos_row, None, guard=0)
    assert torch.equal(rows_only["rg"], want["rg"]) and torch.equal(rows_only["re"], want["re"])
    assert bool((rows_only["cg"].view(torch.uint8) == 0xA5).all()) and bool((rows_only["ce"].view(torch.uint8) == 0xA5).all())


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_retrieval_ranks_on_one_rank_gives_both_directions(idx):
    """losses.retrieval_ranks(normalize=False) on the whole square problem: a -> b are the row counts, b -> a the column counts."""
    from aecf_amd import losses
    c = _case(idx)
    a_full, b = c["a_full"], c["b"]
    ref = _ref_counts(a_full, b, 0, c["pos_col"])
    r = losses.retrieval_ranks(a_full, b, normalize=False)
    assert all(t.dtype == torch.int32 and t.shape == (b.shape[0],) and not t.requires_grad for t in r)
    assert torch.equal(r.a2b_greater, ref["rg"].to(torch.int32)) and torch.equal(r.a2b_equal, ref["re"].to(torch.int32))
    assert torch.equal(r.b2a_greater, ref["cg"].to(torch.int32)) and torch.equal(r.b2a_equal, ref["ce"].to(torch.int32))


# rows, cols, d, off
BAND_CASES = [(300, 1000, 128, 200), (257, 513, 64, 256), (512, 512, 768, 0)]


@pytest.mark.parametrize("rows,cols,d,off", BAND_CASES)
def test_unit_norm_rows_stay_inside_the_rounding_band(rows, cols, d, off):
    from aecf_amd import losses
    g = torch.Generator().manual_seed(11)
    zb = torch.randn(cols, d, generator=g)
    za_full = 0.15 * zb + torch.randn(cols, d, generator=g)
    na_full = losses.l2_normalize(za_full.to(torch.bfloat16).to(DEV)).detach()
    nb = losses.l2_normalize(zb.to(torch.bfloat16).to(DEV)).detach()
    a = na_full[off:off + rows].contiguous()
    eps = d * 2.0 ** -23
    pos_col64 = (na_full.double() * nb.double()).sum(1)
    ref = _ref_counts(a, nb, off, pos_col64)
    s, other = ref["s"], ref["other"]
    L_r, U_r = ((s > ref["pr"] + eps) & other).sum(1), ((s > ref["pr"] - eps) & other).sum(1)
    L_c, U_c = ((s > ref["pc"] + eps) & other).sum(0), ((s > ref["pc"] - eps) & other).sum(0)
    amb_r, amb_c = float((L_r != U_r).float().mean()), float((L_c != U_c).float().mean())
    print(f"retrieval band ({rows}, {cols}, {d}, off {off}): ambiguous rows {100 * amb_r:.1f} %, columns {100 * amb_c:.1f} %, "
          f"median rank {float(L_r.float().median()):.0f}")
    assert amb_r <= 0.10 and amb_c <= 0.10
    pos_col = _positive(na_full, nb, 0)
    assert float((pos_col.double() - pos_col64).abs().max()) <= d * 2.0 ** -24
    got = _ranks_call(a, nb, off, _positive(a, nb, off), pos_col)
    assert bool((got["rg"] >= L_r).all()) and bool((got["rg"] + got["re"] <= U_r).all())
    assert bool((got["cg"] >= L_c).all()) and bool((got["cg"] + got["ce"] <= U_c).all())
    if rows == cols:                                # the public call, normalising by itself, reads the same unit rows
        r = losses.retrieval_ranks(za_full.to(torch.bfloat16).to(DEV), zb.to(torch.bfloat16).to(DEV))
        assert torch.equal(r.a2b_greater, got["rg"]) and torch.equal(r.a2b_equal, got["re"])
        assert torch.equal(r.b2a_greater, got["cg"]) and torch.equal(r.b2a_equal, got["ce"])


def test_emulated_ranks_sum_to_the_global_values():
    """The 300 rows of the first case as three unequal shards with their own row_offset, all reading one pos_col: the row outputs
    concatenate to the one-call result and the column shares add up to it, exactly."""
    c = _case(0)
    a, b, off, want = c["a"], c["b"], c["off"], c["want"]
    parts = []
    for lo, hi in [(0, 37), (37, 256), (256, 300)]:
        sh = a[lo:hi].contiguous()
        parts.append(_ranks_call(sh, b, off + lo, _positive(sh, b, off + lo), c["pos_col"]))
    assert torch.equal(torch.cat([p["rg"] for p in parts]), want["rg"]) and torch.equal(torch.cat([p["re"] for p in parts]), want["re"])
    assert torch.equal(sum(p["cg"] for p in parts), want["cg"]) and torch.equal(sum(p["ce"] for p in parts), want["ce"])


def _metrics_ref(rg, re_, cg, ce, ks, f):
    out = {}
    for side, g, e in (("a2b", rg, re_), ("b2a", cg, ce)):
        rank = g.double() + f * e.double()
        for k in ks:
            out[f"{side}_R@{k}"] = float((rank < k).double().mean())
        out[f"{side}_mrr"] = float((1.0 / (rank + 1.0)).mean())
        out[f"{side}_mean_rank"] = float(rank.mean())
    return out


@pytest.mark.parametrize("ties,f", [("optimistic", 0.0), ("average", 0.5), ("pessimistic", 1.0)])
def test_metrics_equal_the_values_formed_from_the_float64_counts(ties, f):
    from aecf_amd import losses
    c = _case(0)
    a_full, b = c["a_full"], c["b"]
    ref = _ref_counts(a_full, b, 0, c["pos_col"])
    ks = (1, 5, 10)
    want = _metrics_ref(ref["rg"], ref["re"], ref["cg"], ref["ce"], ks, f)
    got = losses.retrieval_metrics(a_full, b, ks=ks, ties=ties, normalize=False)
    assert set(got) == set(want)
    tol = b.shape[0] * 2.0 ** -24                   # float32 rounding of a mean over `rows` terms
    for k, w in want.items():
        v = got[k]
        assert v.dtype == torch.float32 and v.dim() == 0 and v.device.type == "cuda"
        assert abs(float(v) - w) <= tol * abs(w), (k, float(v), w)
    assert want["a2b_R@10"] > want["a2b_R@1"] > 0 and want["a2b_mean_rank"] > 0


def test_guard_bands_stay_intact():
    """Exactly aecf_retrieval_workspace_bytes bytes, 0xA5 behind them and behind every output, at the 257 x 513 shape."""
    c = _case(1)
    a, b, off = c["a"], c["b"], c["off"]
    got = _ranks_call(a, b, off, _positive(a, b, off), c["pos_col"], guard=4096)
    for k in ("rg", "re", "cg", "ce"):
        assert torch.equal(got[k], c["want"][k]), k
    assert len(got["guards"]) == 5 and all(g.numel() == 4096 and bool((g == 0xA5).all()) for g in got["guards"])


def test_captured_call_replays_on_new_inputs():
    from aecf_amd import losses
    g = torch.Generator().manual_seed(5)
    mk = lambda: torch.randn(512, 128, generator=g).to(torch.bfloat16).to(DEV)
    za, zb, za2, zb2 = mk(), mk(), mk(), mk()
    zb2[:256] = za2[:256]                            # ranks of the second problem differ from the first's
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            losses.retrieval_ranks(za, zb)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = losses.retrieval_ranks(za, zb)
    first = [t.clone() for t in r]
    za.copy_(za2)
    zb.copy_(zb2)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in r]
    want = losses.retrieval_ranks(za2, zb2)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not all(torch.equal(x, y) for x, y in zip(got, first))


def test_no_rows_by_cols_allocation():
    """Two [4096, 512] views: the peak above the inputs is the two normalised copies, the workspace -- (rows + cols) cols / 256
    integers -- and O(rows) outputs, far from the 64 MiB of a float32 logits block."""
    from aecf_amd import _lib, losses
    n, d = 4096, 512
    g = torch.Generator().manual_seed(2)
    za, zb = (torch.randn(n, d, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    losses.retrieval_metrics(za, zb)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    m = losses.retrieval_metrics(za, zb)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    wsb = _lib.load().aecf_retrieval_workspace_bytes(n, n, d)
    assert wsb <= 4 * 2 * n * (n // 256) + 1024
    assert peak <= 2 * n * d * 2 + wsb + (1 << 20), peak
    assert 0.0 <= float(m["a2b_R@1"]) <= 1.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


N2 = 300
KS2 = (1, 5, 10)


def _two_rank_views():
    """The 300 positive pairs of the first case (CPU tensors; the children build them again from the seed)."""
    rows, cols, d, off, p = CASES[0]
    g = torch.Generator().manual_seed(7)
    b = torch.randint(-2, 3, (cols, d), generator=g)
    a = torch.randint(-2, 3, (cols, d), generator=g)
    a = torch.where(torch.rand(cols, d, generator=g) < p, b, a)
    return a[off:off + rows].to(torch.bfloat16), b[off:off + rows].to(torch.bfloat16)


def _worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, losses
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        za, zb = _two_rank_views()
        lo, hi = dp.shard_bounds(N2, rank, world)
        a, b = za[lo:hi].to(dev), zb[lo:hi].to(dev)
        r = losses.retrieval_ranks(a, b, normalize=False)
        m = losses.retrieval_metrics(a, b, ks=KS2, normalize=False)
        torch.cuda.synchronize()
        q.put((rank, [t.cpu() for t in r], {k: float(v) for k, v in m.items()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_rank():
    from aecf_amd import losses
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    za, zb = _two_rank_views()
    one = losses.retrieval_ranks(za.to(DEV), zb.to(DEV), normalize=False)
    want_m = {k: float(v) for k, v in losses.retrieval_metrics(za.to(DEV), zb.to(DEV), ks=KS2, normalize=False).items()}
    half = N2 // world
    for rank, counts, metrics in res:
        rows = slice(rank * half, (rank + 1) * half)
        for got, want in zip(counts, one):
            assert torch.equal(got, want[rows].cpu())
        assert metrics == want_m
