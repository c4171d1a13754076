"""``logprobs=`` under a plain sequence shard: two ranks share cuda:0 and talk over gloo, ``tree_spec_generate(shard=...)`` with
the sequence-sharded prefill -- the tail rank computes the first token's log-prob rows and broadcasts them with the token.  Both
ranks must hold the same bits, emit the golden tokens, and the first alternative of every (greedy) column is its token."""
import math
import os
import sys
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_dist import HERE, _find_run, _free_port

pytestmark = pytest.mark.gpu
TOP_N = 2


def _worker(rank, world, port, run_name, q):
    """Puts its result, or its traceback, on the queue: the parent never waits for a worker that has failed."""
    try:
        _run_rank(rank, world, port, run_name, q)
    except Exception:                                        # noqa: BLE001
        q.put((rank, traceback.format_exc()))


def _run_rank(rank, world, port, run_name, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from longspec_amd import Logprobs
    from longspec_amd.dist import KVShard
    from longspec_amd.llama_glide import LlamaGlide
    run = _find_run(run_name)
    m = LlamaGlide(run["cfg"], device="cuda")
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    P = run["prompt_len"]
    shard = KVShard(rank, world, shard_rows=(P + world - 1) // world, vocab_parallel=False)
    out, count, num, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([P], device="cuda"), tree_shape=run["tree_shape"],
                                                 max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], shard=shard,
                                                 logprobs=Logprobs(TOP_N))
    torch.cuda.synchronize()
    lp = m.last_logprobs
    # plain lists: nothing the parent has to fetch from a worker that may have left already
    q.put((rank, out.cpu().tolist(), int(count), int(num), lp.token.view(torch.int32).cpu().tolist(),
           lp.top.view(torch.int32).cpu().tolist(), lp.top_ids.cpu().tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_both_ranks_hold_the_same_logprobs():
    world, run_name = 2, "mixed"
    run = _find_run(run_name)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, run_name, q)) for r in range(world)]
    [p.start() for p in procs]
    res = []
    for _ in range(world):
        res.append(q.get(timeout=300))
        if len(res[-1]) == 2:                                 # a traceback: its peer may be waiting in a collective for good
            [p.terminate() for p in procs]
            pytest.fail(f"rank {res[-1][0]} failed:\n{res[-1][1]}")
    [p.join(timeout=60) for p in procs]
    res.sort()
    assert res[0][1:] == res[1][1:], "the ranks differ"
    _, out, count, num, token_bits, top_bits, top_ids = res[0]
    assert out == run["tree_out"].tolist() and (count, num) == (run["tree_count"], run["tree_num"])
    token = torch.tensor(token_bits, dtype=torch.int32).view(torch.float32)[0]
    n = int((~torch.isnan(token)).sum())
    assert n == min(count + num, len(out[0])) and n >= 8 and torch.isnan(token[n:]).all()
    # an arg-max has at least the probability 1 / V
    assert (token[:n] <= 0).all() and (token[:n] >= -math.log(run["cfg"].vocab_size) - 1e-3).all()
    assert [row[0] for row in top_ids[0][:n]] == out[0][:n]                      # column 0 too: the broadcast first token
    assert [row[0] for row in top_bits[0][:n]] == token_bits[0][:n]
    assert all(row == [-1] * TOP_N for row in top_ids[0][n:])
