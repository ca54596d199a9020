"""World-size-2 CPU (gloo) test of the data-parallel helpers every contrastive driver of aecf_amd/losses.py goes through: the
row-count exchange, the agreement on a refusal and the returned value.  The collectives of two ranks must pair up, so a
mismatch shows here as a hang (the timeout) and a wrong policy as a wrong value.  No compiled library, no device."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from aecf_amd import losses

REFUSAL = "d % 64 == 0 with 64 <= d <= 4096 (got d = 65)"
ANOTHER_RANK = "the same on every rank (another rank refused it)"
SHARDS = (3, 2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cpu = torch.device("cpu")
        ranges = losses._row_ranges(SHARDS[rank], cpu, None)
        rows = torch.arange(SHARDS[rank] * 2, dtype=torch.float32).reshape(SHARDS[rank], 2) + 100.0 * rank
        gathered = losses._all_rows(rows, None, ranges[0])
        one_refuses = losses._agreed_refusal(None if rank == 0 else REFUSAL, cpu, None)
        none_refuses = losses._agreed_refusal(None, cpu, None)
        share = torch.tensor(1.5 + rank, requires_grad=True)
        value = losses._dp_value(share, None)
        value.backward()
        q.put((rank, ranges, gathered.numpy(), one_refuses, none_refuses, float(value), float(share.grad)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_ranks_exchange_rows_agree_on_a_refusal_and_return_the_global_value():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=150) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    all_rows = torch.cat([torch.arange(n * 2, dtype=torch.float32).reshape(n, 2) + 100.0 * r for r, n in enumerate(SHARDS)])
    for rank, ranges, gathered, one_refuses, none_refuses, value, grad in res:
        assert ranges == ([3, 2], (0, 3)[rank], 5)                          # uneven shards: sizes, this rank's first row, total
        assert torch.equal(torch.from_numpy(gathered), all_rows)            # ... which gather the rows in rank order
        assert one_refuses == (ANOTHER_RANK, REFUSAL)[rank]                 # the rank that would have run refuses too
        assert none_refuses is None
        assert value == 1.5 + 2.5                                           # the sum of the shares, on both ranks
        assert grad == float(world)                                         # the local term carries `world`


def test_one_rank_issues_no_collective():
    """without a process group: nothing to exchange, the arguments come back as they went in"""
    assert not dist.is_initialized()
    cpu = torch.device("cpu")
    assert losses._row_ranges(7, cpu, None) == (None, 0, 7)
    rows = torch.ones(7, 2)
    assert losses._all_rows(rows, None, None) is rows
    assert losses._agreed_refusal(REFUSAL, cpu, None) == REFUSAL and losses._agreed_refusal(None, cpu, None) is None
    share = torch.tensor(2.0, requires_grad=True)
    assert losses._dp_value(share, None) is share
