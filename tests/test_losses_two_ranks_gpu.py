"""The label-aware and pooled two-view losses of aecf_amd/losses.py on TWO ranks against float64: supervised_contrastive,
nt_xent, pooled_supervised_contrastive, multilabel_contrastive, pooled_multilabel_contrastive and fusion_objective over them,
every form, through their data-parallel paths (the row-count exchange, the gathers of rows and labels or sets, the agreement on a
form, the all-reduce of the column statistics, the reduce of the gathered rows' gradients, _dp_value).  One pair of worker
processes, spawned once for the file, runs every route of tests/losses_two_ranks_cases.ROUTES on its uneven shard (151 and 150
of 301 rows); the parent holds each route against the float64 reference of the whole batch with the bounds derived in that
module (tests/test_losses_two_ranks_cpu.py shows that they catch a wrong offset, labels that were not gathered, swapped self and
partner keys, statistics that were not reduced, a dropped share, a missing ``world`` and a padding row left among the keys)."""
import datetime
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import losses_two_ranks_cases as K
from tests.helpers import record_errors

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(420)]

DEV = torch.device("cuda:0")
F32 = torch.float32
FIELDS = ("loss", "quiet", "dT", "dza", "dzb")


def _meta(inp, key, dev):
    if key is None:
        return None
    if key == "labels32":
        return inp["labels"].to(torch.int32).to(dev)
    if key == "unlabeled":
        return torch.full((inp["labels"].shape[0],), -1, dtype=torch.int64, device=dev)
    return inp[key].to(dev)


def _run_route(losses, route, za0, zb0, meta, world, dev):
    name, kw, _, _ = K.ROUTES[route]
    za, zb = za0.clone().requires_grad_(True), zb0.clone().requires_grad_(True)
    T = torch.tensor(K.T0, dtype=F32, device=dev, requires_grad=True)

    def call():
        if name == "fusion_objective":
            task = torch.tensor(K.FUSION_TASK, dtype=F32, device=dev)
            return losses.fusion_objective(task, None, None, za, zb, temperature=T, group=dist.group.WORLD, labels=meta, **kw)
        if name == "nt_xent":
            return losses.nt_xent(za, zb, temperature=T, **kw)
        return getattr(losses, name)(za, zb, meta, temperature=T, **kw)

    loss = call()
    loss.backward()
    with torch.no_grad():
        quiet = call()
    torch.cuda.synchronize()
    # gradients follow the data-parallel convention (averaged over ranks later): undo the factor `world`
    return dict(loss=float(loss.detach()), quiet=float(quiet), dT=float(T.grad / world),
                dza=(za.grad.float() / world).cpu().numpy(), dzb=(zb.grad.float() / world).cpu().numpy())


def _two_ranks_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, losses
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    limit = datetime.timedelta(seconds=90)          # a collective without its partner raises here instead of hanging
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=limit)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    done, error = {}, None
    try:
        inp = K.inputs()
        lo, hi = dp.shard_bounds(K.N, rank, world)
        assert (lo, hi) == K.SHARDS[rank]
        za0, zb0 = inp["za"][lo:hi].to(dev), inp["zb"][lo:hi].to(dev)
        for route in K.ROUTE_IDS:
            meta = _meta(inp, K.ROUTES[route][2], dev)
            try:
                done[route] = _run_route(losses, route, za0, zb0, None if meta is None else meta[lo:hi], world, dev)
            except Exception:                       # reported; no further route runs on this rank
                error = f"rank {rank}, route {route}:\n{traceback.format_exc()}"
                break
    finally:
        q.put((rank, done, error))
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    """(per rank: route -> what the worker returned, na, nb): one spawn of two workers for the whole file; the unit rows are the
    library's own l2_normalize outputs (the rows the kernels read), formed here on the parent's device"""
    from aecf_amd import losses
    world = K.WORLD
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_ranks_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    try:
        got = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
        for p in procs:
            p.join(60)
    finally:
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.kill()
        for p in alive:
            p.join(30)
    errors = [e for _, _, e in got if e is not None]
    assert not errors, "\n".join(errors)
    assert not alive and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    inp = K.inputs()
    with torch.no_grad():
        na, nb = losses.l2_normalize(inp["za"].to(DEV)).cpu(), losses.l2_normalize(inp["zb"].to(DEV)).cpu()
    return [done for _, done, _ in got], na, nb


_REFERENCES = {}


def _reference(form, na, nb):
    """(reference, what a caller sees of it with its bounds) of a form, computed once for the routes that share it"""
    if form not in _REFERENCES:
        inp = K.inputs()
        ref = K.reference(form, na, nb, K.meta_of(form, inp))
        _REFERENCES[form] = (ref, K.caller_view(ref, inp["za"], inp["zb"], na, nb))
    return _REFERENCES[form]


def _same_bits(one, two):
    return all(np.array_equal(one[f], two[f]) for f in FIELDS)


@pytest.mark.parametrize("route", K.ROUTE_IDS)
def test_two_ranks_against_float64(two_ranks, route):
    """The loss on both ranks is the global loss and one number; each rank's dza and dzb are its rows of the reference; the ranks'
    shares of dT add up to it; under torch.no_grad() the value has the same bits.  The fusion_objective route is the task loss
    plus the term, bit for bit."""
    ranks, na, nb = two_ranks
    form = K.ROUTES[route][3]
    ref, view = _reference(form, na, nb)
    res = [dict(r[route]) for r in ranks]
    assert res[0]["loss"] == res[1]["loss"]
    for r in res:
        assert r["quiet"] == r["loss"]
        assert r["dza"].shape == r["dzb"].shape and np.isfinite(r["dza"]).all() and np.isfinite(r["dzb"]).all()
    extra = 0.0
    if K.ROUTES[route][0] == "fusion_objective":
        task = torch.tensor(K.FUSION_TASK, dtype=F32)
        for r, other in zip(res, ranks):
            assert r["loss"] == float(task + torch.tensor(other["pool_tile"]["loss"], dtype=F32))
            assert all(np.array_equal(r[f], other["pool_tile"][f]) for f in ("dT", "dza", "dzb"))
            extra = 2.0 ** -24 * abs(r["loss"])                  # the float32 sum with the task loss
            r["loss"] = r["loss"] - float(task)
    for r in res:
        r["dza"], r["dzb"] = torch.from_numpy(r["dza"]), torch.from_numpy(r["dzb"])
    bounded = dict(ref, b_loss=ref["b_loss"] + extra)
    ratios = K.ratios(bounded, view, res)
    print(f"losses_two_ranks_parity route {route} (form {form}) N {K.N} d {K.D} T {K.T0}: "
          + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    record_errors("losses_two_ranks_" + route, T=K.T0, **ratios)
    assert not K.outside(ratios), ratios


@pytest.mark.parametrize("route,twin", K.SAME_BITS)
def test_routes_that_promise_the_same_bits(two_ranks, route, twin):
    """low_memory=None has the bits of False (the ranks agree on the tile form); int32 labels those of int64 labels;
    pooled_supervised_contrastive(low_memory=True) those of supervised_contrastive(intra_view=True); nt_xent those of the pooled
    forms with every label -1 -- loss, both gradients and dT, on each rank."""
    ranks, _, _ = two_ranks
    for done in ranks:
        assert _same_bits(done[route], done[twin])
