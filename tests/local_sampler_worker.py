"""Worker of tests/test_gpu_local_sampler.py: one rank of a sharded mh_select_greedy over a batch proposed with the
neighbourhood-guided sampler, over gloo on a shared GPU (the host-synchronised transport).  Prints one JSON line per rank."""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mh = importlib.import_module("multi-h_amd")
sh = importlib.import_module("multi-h_amd.sharding")

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
THR2, TOTAL, K, U = 2.2 ** 2, 3000, 16, 4
sc = mh.synth.make_scene(3000, 3, seed=3, with_neighbours=False)
eng = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
eng.set_tuning(5, 64)                                   # the ranks share one GPU: a quarter of the chip each
eng.set_correspondences(sc.src, sc.dst, sc.aff)
eng.build_sample_neighbours(K)
hook = sh.make_allgather_hook(world, dev)
eng.set_transport(rank, world, host_fn=hook)
first, mine = sh.shard_range(TOTAL, world, rank)
out = {"rank": rank}


def attempt(name, sampler, u):
    try:
        eng.set_sampler(sampler, u)
        eng.propose_dlt4(77, first, mine)
        H, counters, counts, _ = eng.select_greedy(THR2, 20, 8, np.ones(sc.n, np.uint8), total_m=TOTAL)
        out[name] = {"ok": True, "counters": counters.tolist(), "counts": counts.tolist(), "H": H.view(np.uint64).tolist()}
    except mh.MultiHError as ex:
        out[name] = {"ok": False, "code": ex.code, "msg": str(ex)}
    dist.barrier()


attempt("local", mh.SAMPLER_LOCAL, U)
# rank 0 proposes uniformly, rank 1 locally: the records' mode words differ
attempt("mixed", mh.SAMPLER_UNIFORM if rank == 0 else mh.SAMPLER_LOCAL, U)
# both local, but with another share of uniform tuples on rank 1
attempt("other_share", mh.SAMPLER_LOCAL, U if rank == 0 else U + 1)
attempt("local_again", mh.SAMPLER_LOCAL, U)
for r in range(world):                                  # one rank at a time: the launcher merges the ranks' stdout
    if r == rank:
        print(json.dumps(out), flush=True)
    dist.barrier()
eng.close()
dist.barrier()
dist.destroy_process_group()
