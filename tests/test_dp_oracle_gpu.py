"""Two data-parallel ranks against the float64 oracle of the GLOBAL batch.

Each rank runs its shard (``dp.shard_bounds``) of one global batch through an attached pool (``dp.attach``), reduces with
``dp.all_reduce_grads`` / ``dp.GradOverlap`` in the call shapes a training loop uses, and every gradient it ends with must be
the float64 oracle's gradient of the global loss (y . dy + wbar . dwbar summed over the batch) at the one-rank bounds of
tests/test_dp_routes_gpu.py.  Before each backward the caching allocator is poisoned with NaN blocks the size of the gradient
run, so that a gradient read before anything wrote it is not finite instead of passing by luck.

Two ranks on two GPUs use RCCL; on a one-GPU box both share device 0 and rendezvous over gloo (tests/test_dp_gpu.py)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import BF16_BOUNDS, f32grad_bounds, rel_err

pytestmark = pytest.mark.gpu

B, M, E, H = 600, 3, 128, 4
GENERAL_BF16_TOL = 1e-2            # the general kernels in bf16 (tests/test_pool_gpu_shapes.py)
CONFIGS = {"bf16": (torch.bfloat16, torch.bfloat16), "f32": (torch.float32, torch.float32),
           "master": (torch.float32, torch.bfloat16)}          # (parameter dtype, activation dtype)
# scenario -> how the step is reduced; every one ends with each rank holding the global-batch gradient
SCENARIOS = {
    "bf16": ["plain", "deferred", "params_then_query", "two_pools", "unrelated_first", "overlap_subset", "computed_query",
             "computed_query_overlap", "key_is_not_value", "fused_and_general"],
    "f32": ["plain", "key_is_not_value", "fused_and_general"],
    "master": ["plain", "fused_and_general"],
}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _data(seed):
    """bf16-representable float64 parameters, fusion query, inputs (x, a second value tensor v) and upstream gradients."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t_: t_.to(torch.bfloat16).double()
    return dict(w_in=bf(r(3 * E, E) / E ** 0.5), b_in=bf(r(3 * E) * 0.05), w_out=bf(r(E, E) / E ** 0.5), b_out=bf(r(E) * 0.05),
                q=bf(r(1, 1, E) * (2.0 / E) ** 0.5), x=bf(r(B, M, E) * torch.tensor([1.0, 1.5, 2.0]).view(1, M, 1)),
                v=bf(r(B, M, E)), dy=bf(r(B, 1, E)), dwbar=bf(r(B, 1, M)))


def _pool(d, dev, pdt):
    import aecf_amd
    pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H)
    a = pool.attention
    with torch.no_grad():
        for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"), (a.out_proj.bias, "b_out")):
            p.copy_(d[k])
    return pool.to(dev, pdt).train(), torch.nn.Parameter(d["q"].to(dev, pdt))


def _poison(dev, pdt):
    """NaN blocks the size of the gradient run (float32 sums and parameter dtype), freed: the caching allocator hands them to
    the next allocations of that size -- the run of the backward that follows."""
    n = 4 * E * E + 5 * E
    for dt in {torch.float32, pdt}:
        torch.full((n,), float("nan"), dtype=dt, device=dev)


def _rows(d, key, lo, hi, dev, adt):
    return d[key][lo:hi].to(dev, adt)


def _loss(pool, q, d, lo, hi, dev, adt, world, general=False):
    """This rank's part of the global loss, times world: after the averaging collective the gradients are those of the global
    loss.  ``general``: value != key, which the general kernels serve."""
    x = _rows(d, "x", lo, hi, dev, adt)
    v = _rows(d, "v", lo, hi, dev, adt) if general else x
    y, info = pool(q.expand(hi - lo, -1, -1), x, v, return_info=True)
    w = info["attention_weights"]
    return world * ((y.float() * _rows(d, "dy", lo, hi, dev, torch.float32)).sum()
                    + (w.float() * _rows(d, "dwbar", lo, hi, dev, torch.float32)).sum())


def _worker(rank, world, port, backend, config, q_out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pdt, adt = CONFIGS[config]
        d, d2 = _data(1), _data(2)
        lo, hi = dp.shard_bounds(B, rank, world)
        mid = B // 2                                       # fused_and_general: rows [0, mid) fused, [mid, B) general
        (alo, ahi), (blo, bhi) = dp.shard_bounds(mid, rank, world), dp.shard_bounds(B - mid, rank, world)
        results = {}
        for name in SCENARIOS[config]:
            pool, q = _pool(d, dev, pdt)
            params = [q] + list(pool.parameters())
            dp.attach(pool, defer_rounding=name not in ("plain", "key_is_not_value"))
            out = {}
            if name == "two_pools":
                pool2, q2 = _pool(d2, dev, pdt)
                dp.attach(pool2, defer_rounding=True)
                _poison(dev, pdt)
                (_loss(pool, q, d, lo, hi, dev, adt, world) + _loss(pool2, q2, d2, lo, hi, dev, adt, world)).backward()
                dp.all_reduce_grads(params + [q2] + list(pool2.parameters()))
                out["second"] = [p.grad.float().cpu().numpy() for p in [q2] + list(pool2.parameters())]
                dp.detach(pool2)
            elif name in ("computed_query", "computed_query_overlap"):
                # the query is computed from a leaf (its producer): the gradient that reaches the leaf must be finished values
                q_src = torch.nn.Parameter((q.detach() * 0.5).clone())
                params = [q_src] + list(pool.parameters())
                _poison(dev, pdt)
                if name == "computed_query":
                    _loss(pool, 2 * q_src, d, lo, hi, dev, adt, world).backward()
                    dp.all_reduce_grads(params)
                else:
                    overlap = dp.GradOverlap(params=params)
                    with overlap:
                        _loss(pool, 2 * q_src, d, lo, hi, dev, adt, world).backward()
                        overlap.finish(params)
            elif name == "fused_and_general":
                # one pool applied twice, feeding one loss: the shared-query kernels on rows [0, mid), the general ones on the rest
                _poison(dev, pdt)
                (_loss(pool, q, d, alo, ahi, dev, adt, world)
                 + _loss(pool, q, d, mid + blo, mid + bhi, dev, adt, world, general=True)).backward()
                dp.all_reduce_grads(params)
            elif name == "overlap_subset":
                overlap = dp.GradOverlap(params=params)
                _poison(dev, pdt)
                with overlap:
                    _loss(pool, q, d, lo, hi, dev, adt, world).backward()
                    overlap.finish(list(pool.parameters()))              # the hook's collective covered the query's gradient too
            else:
                _poison(dev, pdt)
                _loss(pool, q, d, lo, hi, dev, adt, world, general=name == "key_is_not_value").backward()
                if name == "params_then_query":
                    dp.all_reduce_grads(list(pool.parameters()))
                    dp.all_reduce_grads([q])
                elif name == "unrelated_first":
                    lin = torch.nn.Linear(8, 8, device=dev)
                    lin(torch.ones(2, 8, device=dev)).sum().backward()
                    dp.all_reduce_grads(list(lin.parameters()))
                    dp.all_reduce_grads(params)
                else:
                    dp.all_reduce_grads(params)
            torch.cuda.synchronize()
            out["first"] = [p.grad.float().cpu().numpy() for p in params]
            results[name] = out
            dp.detach(pool)
        q_out.put((rank, results))
    finally:
        dist.destroy_process_group()


def _oracle(d, rows=slice(None), general=False):
    from oracle import aecf_oracle as O
    x, v = d["x"][rows], (d["v"] if general else d["x"])[rows]
    qe = d["q"].expand(x.shape[0], -1, -1)
    f = O.mha_forward(qe, x, v, d["w_in"], d["b_in"], d["w_out"], d["b_out"], H)
    b = O.mha_backward(qe, x, v, d["w_in"], d["b_in"], d["w_out"], H, f, d["dy"][rows], d["dwbar"][rows])
    return [b["dquery"].sum(0, keepdim=True), b["dw_in"], b["db_in"], b["dw_out"], b["db_out"]]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_two_ranks_reduce_to_the_global_batch_oracle(config):
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, config, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=500) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    pdt, adt = CONFIGS[config]
    d, d2 = _data(1), _data(2)
    names = ("dquery", "dw_in", "db_in", "dw_out", "db_out")
    if adt == torch.float32:
        bounds = dict(dquery=2e-5, dw_in=2e-5, db_in=2e-5, dw_out=2e-5, db_out=2e-5)
    else:
        bounds = f32grad_bounds(B, M, E, H) if pdt != adt else BF16_BOUNDS
    general_bounds = bounds if adt == torch.float32 else {k: GENERAL_BF16_TOL for k in names}
    fused = _oracle(d)
    mid = B // 2
    want = {"key_is_not_value": (_oracle(d, general=True), general_bounds),
            "fused_and_general": ([a + b for a, b in zip(_oracle(d, slice(0, mid)), _oracle(d, slice(mid, B), general=True))],
                                  general_bounds)}
    for rank, results in res:
        for name, out in results.items():
            ref, bnd = want.get(name, (fused, bounds))
            if name.startswith("computed_query"):
                ref = [2 * ref[0]] + ref[1:]                # the producer q = 2 * q_src: d q_src = 2 dquery
            checks = [(out["first"], ref)]
            if name == "two_pools":
                checks.append((out["second"], _oracle(d2)))
            for got_all, ref_all in checks:
                for k, g, r in zip(names, got_all, ref_all):
                    g = torch.from_numpy(g)
                    assert torch.isfinite(g).all(), (config, name, rank, k, "a gradient read before it was written")
                    e = rel_err(g, r.reshape(g.shape))
                    assert e < bnd[k], (config, name, rank, k, e, bnd[k])
