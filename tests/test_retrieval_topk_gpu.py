"""Top-k retrieval: losses.retrieval_topk and the C ABI behind it (aecf_retrieval_topk).

The yardstick is float64 torch on the rows the kernels read.  The order the library specifies is total -- higher score first,
lower column first among equal scores, NaN below -inf -- and on exact scores it is what a STABLE descending sort gives:
  * integer-valued bf16 rows (entries in {-2..2}): every dot product is an integer far below 2^24, float32 accumulation is exact
    in any order, so values and indices must equal torch.sort(s64, descending=True, stable=True) cut at k, bit for bit; the
    inputs are required to hold ties at the k-th place, many of them across two column tiles;
  * unit-norm random rows: a float32 dot product of unit vectors is within d 2^-24 of exact, so with eps = d 2^-23 and t the k-th
    largest float64 score every returned column scores at least t - eps and every column above t + eps is returned."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# rows, cols, d, row_offset, p
CASES = [(300, 1000, 128, 200, 0.1), (257, 513, 64, 256, 0.1), (64, 320, 1024, 256, 0.05),
         (4096, 8192, 64, 2048, 0.1)]       # the last: 16 x 32 output tiles, more than the 256 CUs hold at one block each
KS = (1, 10, 16)
_cache = {}


def _int_views(cols, d, p, seed=7):
    """b [cols, d] and its partner view a_full [cols, d] (row i of one is the positive of row i of the other), entries uniform
    in {-2..2}; the partner copies an entry with probability p, so positives score high and ties are common."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(-2, 3, (cols, d), generator=g)
    a = torch.randint(-2, 3, (cols, d), generator=g)
    a = torch.where(torch.rand(cols, d, generator=g) < p, b, a)
    return a.to(torch.bfloat16), b.to(torch.bfloat16)


def _topk_call(a, b, k, off=0, exclude=False, guard=0):
    """aecf_retrieval_topk with exactly the workspace it asks for; guard > 0 puts that many 0xA5 bytes behind the workspace and
    behind both outputs (returned as `guards`)."""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    rows, d = a.shape
    cols = b.shape[0]
    wsb = lib.aecf_retrieval_topk_workspace_bytes(rows, cols, d, k)
    assert wsb > 0
    ws = torch.full((wsb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    vals = torch.full((rows * k * 4 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    idx = torch.full((rows * k * 4 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(lib.aecf_retrieval_topk(rows, cols, off, d, k, 1 if exclude else 0, _ptr(a), _ptr(b), _ptr(vals), _ptr(idx), _ptr(ws),
                                       wsb, _stream()), "aecf_retrieval_topk")
    torch.cuda.synchronize()
    n = rows * k * 4
    return dict(values=vals[:n].view(torch.float32).view(rows, k), indices=idx[:n].view(torch.int32).view(rows, k),
                guards=[ws[wsb:], vals[n:], idx[n:]])


def _case(idx):
    """Inputs and the float64 stable descending sort of an integer case (with and without the partner), computed once."""
    if idx not in _cache:
        rows, cols, d, off, p = CASES[idx]
        a_full, b = _int_views(cols, d, p)
        a_full, b = a_full.to(DEV), b.to(DEV)
        a = a_full[off:off + rows].contiguous()
        s = a.double() @ b.double().T
        ref = {}
        for excl in (False, True):
            sm = s
            if excl:
                sm = s.clone()
                sm[torch.arange(rows, device=DEV), off + torch.arange(rows, device=DEV)] = -float("inf")
            v, i = torch.sort(sm, dim=1, descending=True, stable=True)
            ref[excl] = (v[:, :17].contiguous(), i[:, :17].contiguous())
        _cache[idx] = dict(a=a, b=b, off=off, ref=ref, smax=float(s.abs().max()))
    return _cache[idx]


def _assert_exact(got, ref, k):
    v, i = ref
    assert got["indices"].dtype == torch.int32 and got["values"].dtype == torch.float32
    assert torch.equal(got["indices"].long(), i[:, :k])
    assert torch.equal(got["values"].double(), v[:, :k])


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_integer_rows_give_the_stable_float64_sort_bit_for_bit(idx, k, exclude):
    c = _case(idx)
    assert c["smax"] < 2 ** 24
    _assert_exact(_topk_call(c["a"], c["b"], k, c["off"], exclude), c["ref"][exclude], k)


@pytest.mark.parametrize("idx", [0, 3])
def test_the_integer_inputs_exercise_the_tie_rule(idx):
    """On the reference alone: at k = 10 a good share of the rows has s[k-1] == s[k] -- the k-th place is decided by the column
    rule -- and in a good share of the rows that tie lies across two column tiles, where only the merge can decide it (both
    shares are of all rows: the second is the stricter reading of "ties that straddle")."""
    c = _case(idx)
    k = 10
    v, i = c["ref"][False]
    tie = v[:, k - 1] == v[:, k]
    share = float(tie.double().mean())
    straddle = float(((i[:, k - 1] // 256 != i[:, k] // 256) & tie).double().mean())
    print(f"top-k ties {tuple(c['a'].shape)} x {c['b'].shape[0]}: rows with s[k-1] == s[k] {share:.2f}, with that tie across two tiles {straddle:.2f}")
    assert share >= 0.30 and straddle >= 0.20


def _check_well_formed(got, cols):
    idx = got["indices"].long()
    assert bool(((idx >= 0) & (idx < cols)).all())                       # no sentinel, no padding column
    srt = idx.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())                      # distinct per row


def test_degenerate_sizes():
    a_full, b = _int_views(16, 64, 0.1)
    a_full, b = a_full.to(DEV), b.to(DEV)
    # 5 x 16, k = 16: every column comes back, in order
    a = a_full[:5].contiguous()
    s = a.double() @ b.double().T
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    got = _topk_call(a, b, 16)
    _check_well_formed(got, 16)
    _assert_exact(got, (v, i), 16)
    # 16 x 16 with the partner left out, k = 15: every other column
    s = a_full.double() @ b.double().T
    s[torch.arange(16, device=DEV), torch.arange(16, device=DEV)] = -float("inf")
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    got = _topk_call(a_full, b, 15, 0, True)
    _check_well_formed(got, 16)
    _assert_exact(got, (v, i), 15)
    assert bool((got["indices"].long() != torch.arange(16, device=DEV)[:, None]).all())
    # one row, against one tile and against several
    c = _case(0)
    for keys in (b, c["b"]):
        a1 = torch.randint(-2, 3, (1, keys.shape[1]), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(DEV)
        s = a1.double() @ keys.double().T
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        for k in (1, 16):
            got = _topk_call(a1, keys, k)
            _check_well_formed(got, keys.shape[0])
            _assert_exact(got, (v, i), k)


# rows, cols, d, off, largest share of rows the band may leave undetermined
BAND_CASES = [(300, 1000, 128, 200, 0.05), (257, 513, 64, 256, 0.05), (512, 512, 768, 0, 0.25)]
_band = {}


def _band_case(rows, cols, d, off):
    if (rows, cols, d) not in _band:
        from aecf_amd import losses
        g = torch.Generator().manual_seed(11)
        zb = torch.randn(cols, d, generator=g)
        za_full = 0.15 * zb + torch.randn(cols, d, generator=g)
        za_full, zb = za_full.to(torch.bfloat16).to(DEV), zb.to(torch.bfloat16).to(DEV)
        na_full, nb = losses.l2_normalize(za_full).detach(), losses.l2_normalize(zb).detach()
        a = na_full[off:off + rows].contiguous()
        s = a.double() @ nb.double().T
        _band[(rows, cols, d)] = dict(za_full=za_full, zb=zb, a=a, nb=nb, s=s, sorted=torch.sort(s, dim=1, descending=True).values)
    return _band[(rows, cols, d)]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows,cols,d,off,max_share", BAND_CASES)
def test_unit_norm_rows_stay_inside_the_rounding_band(rows, cols, d, off, max_share, k):
    c = _band_case(rows, cols, d, off)
    s, a, nb = c["s"], c["a"], c["nb"]
    eps = d * 2.0 ** -23
    t = c["sorted"][:, k - 1:k]                                          # the k-th largest float64 score of the row
    # the band leaves the set undetermined where something other than the k-th element lies within eps of t
    undetermined = float((((s - t).abs() <= eps).sum(1) > 1).double().mean())
    print(f"top-k band ({rows}, {cols}, {d}) k = {k}: rows the band leaves undetermined {undetermined:.3f}")
    assert undetermined <= max_share
    got = _topk_call(a, nb, k)
    _check_well_formed(got, cols)
    idx, vals = got["indices"].long(), got["values"].double()
    at = s.gather(1, idx)
    assert bool((at >= t - eps).all())                                   # every returned column is in the band or above
    returned = torch.zeros_like(s, dtype=torch.bool).scatter_(1, idx, True)
    assert bool((returned | ~(s > t + eps)).all())                       # everything clearly above is returned
    assert float((vals - at).abs().max()) <= d * 2.0 ** -24
    assert bool((vals[:, 1:] <= vals[:, :-1]).all())                     # in order
    if rows == cols:                                # the public call, normalising by itself, reads the same unit rows
        from aecf_amd import losses
        r = losses.retrieval_topk(c["za_full"], c["zb"], k)
        assert r.indices.dtype == torch.int64 and r.values.dtype == torch.float32 and not r.values.requires_grad
        assert torch.equal(r.indices, idx) and torch.equal(r.values, got["values"])


def test_nan_scores_come_last():
    c = _case(0)
    a, b, off = c["a"], c["b"], c["off"]
    rows, cols = a.shape[0], b.shape[0]
    # one key row NaN: that column is in no row's top 16 (every other column of the row scores above it)
    bn = b.clone()
    bn[517] = float("nan")
    got = _topk_call(a, bn, 16)
    _check_well_formed(got, cols)
    assert not bool((got["indices"] == 517).any()) and not bool(got["values"].isnan().any())
    s = a.double() @ b.double().T
    s[:, 517] = -float("inf")
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    _assert_exact(got, (v, i), 16)
    # one query row NaN: all its scores are equal, so the column rule alone orders them; the other rows are untouched
    an = a.clone()
    an[41] = float("nan")
    for k in (10, 16):
        got = _topk_call(an, b, k)
        assert torch.equal(got["indices"][41].long(), torch.arange(k, device=DEV)) and bool(got["values"][41].isnan().all())
        keep = torch.arange(rows, device=DEV) != 41
        rv, ri = c["ref"][False]
        assert torch.equal(got["indices"][keep].long(), ri[keep][:, :k]) and torch.equal(got["values"][keep].double(), rv[keep][:, :k])


def test_guard_bands_stay_intact():
    """Exactly aecf_retrieval_topk_workspace_bytes bytes, 0xA5 behind them and behind both outputs, at the 257 x 513 shape."""
    c = _case(1)
    got = _topk_call(c["a"], c["b"], 10, c["off"], guard=4096)
    _assert_exact(got, c["ref"][False], 10)
    assert len(got["guards"]) == 3 and all(g.numel() == 4096 and bool((g == 0xA5).all()) for g in got["guards"])


def test_shards_concatenate_to_the_one_call_result():
    """The 300 rows of the first case as three unequal shards with their own row_offset and the partner left out."""
    c = _case(0)
    a, b, off = c["a"], c["b"], c["off"]
    whole = _topk_call(a, b, 10, off, True)
    parts = [_topk_call(a[lo:hi].contiguous(), b, 10, off + lo, True) for lo, hi in [(0, 37), (37, 256), (256, 300)]]
    assert torch.equal(torch.cat([p["indices"] for p in parts]), whole["indices"])
    assert torch.equal(torch.cat([p["values"] for p in parts]), whole["values"])
    _assert_exact(whole, c["ref"][True], 10)


def test_captured_call_replays_on_new_inputs():
    from aecf_amd import losses
    g = torch.Generator().manual_seed(5)
    mk = lambda: torch.randn(512, 128, generator=g).to(torch.bfloat16).to(DEV)
    za, zb, za2, zb2 = mk(), mk(), mk(), mk()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            losses.retrieval_topk(za, zb, 10)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = losses.retrieval_topk(za, zb, 10)
    first = [t.clone() for t in r]
    za.copy_(za2)
    zb.copy_(zb2)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in r]
    want = losses.retrieval_topk(za2, zb2, 10)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not all(torch.equal(x, y) for x, y in zip(got, first))


def test_no_rows_by_cols_allocation():
    """Two [4096, 512] views, k = 10: the peak above the inputs is the two normalised copies, the workspace -- 8 KP bytes per row
    and column tile -- and O(rows k) outputs, far from the 64 MiB of a float32 logits block."""
    from aecf_amd import _lib, losses
    n, d, k = 4096, 512, 10
    g = torch.Generator().manual_seed(2)
    za, zb = (torch.randn(n, d, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    losses.retrieval_topk(za, zb, k)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    r = losses.retrieval_topk(za, zb, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    wsb = _lib.load().aecf_retrieval_topk_workspace_bytes(n, n, d, k)
    assert wsb <= 8 * 16 * n * (n // 256) + 4096
    assert peak <= 2 * n * d * 2 + wsb + 16 * n * k + (1 << 20), peak
    assert peak < 64 << 20
    assert r.indices.shape == (n, k)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


N2 = 300
K2 = 10


def _two_rank_views():
    """The 300 positive pairs of the first case (CPU tensors; the children build them again from the seed)."""
    rows, cols, d, off, p = CASES[0]
    a, b = _int_views(cols, d, p)
    return a[off:off + rows], b[off:off + rows]


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
        out = []
        for excl in (False, True):
            r = losses.retrieval_topk(a, b, K2, normalize=False, exclude_partner=excl)
            torch.cuda.synchronize()
            out.append((r.values.cpu(), r.indices.cpu()))
        q.put((rank, out))
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
    half = N2 // world
    for n, excl in enumerate((False, True)):
        one = losses.retrieval_topk(za.to(DEV), zb.to(DEV), K2, normalize=False, exclude_partner=excl)
        if excl:
            assert bool((one.indices != torch.arange(N2, device=DEV)[:, None]).all())
        for rank, out in res:
            rows = slice(rank * half, (rank + 1) * half)
            values, indices = out[n]
            assert indices.dtype == torch.int64
            assert torch.equal(values, one.values[rows].cpu()) and torch.equal(indices, one.indices[rows].cpu())
