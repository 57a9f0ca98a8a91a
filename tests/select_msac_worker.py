"""Worker of tests/test_gpu_select_msac.py: one rank of a sharded mh_select_greedy_msac over gloo on a shared GPU (the
host-synchronised transport).  Prints one JSON line per rank."""
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
THR2, TOTAL = 2.2 ** 2, 3001
sc = mh.synth.make_scene(3000, 3, seed=3, with_neighbours=False)
eng = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
eng.set_tuning(5, 64)                                   # the ranks share one GPU: a quarter of the chip each
eng.set_correspondences(sc.src, sc.dst, sc.aff)
hook = sh.make_allgather_hook(world, dev)
eng.set_transport(rank, world, host_fn=hook)
first, mine = sh.shard_range(TOTAL, world, rank)
out = {"rank": rank}


def attempt(name, by_weight):
    try:
        eng.propose_dlt4(77, first, mine)
        ones = np.ones(sc.n, np.uint8)
        if by_weight:
            H, counters, counts, weights, mask = eng.select_greedy_msac(THR2, 20, 8, ones, total_m=TOTAL)
        else:
            H, counters, counts, mask = eng.select_greedy(THR2, 20, 8, ones, total_m=TOTAL)
            weights = np.zeros(0, np.int32)
        out[name] = {"ok": True, "counters": counters.tolist(), "counts": counts.tolist(), "weights": weights.tolist(),
                     "H": H.view(np.uint64).tolist(), "left": int(mask.sum())}
    except mh.MultiHError as ex:
        out[name] = {"ok": False, "code": ex.code, "msg": str(ex)}
    dist.barrier()


attempt("msac", True)
# rank 0 ranks by count, rank 1 by weight: the records' mode words differ, the collectives do not
attempt("mixed", rank != 0)
attempt("msac_again", True)
for r in range(world):                                  # one rank at a time: the launcher merges the ranks' stdout
    if r == rank:
        print(json.dumps(out), flush=True)
    dist.barrier()
eng.close()
dist.barrier()
dist.destroy_process_group()
