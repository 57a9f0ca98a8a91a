"""Worker of tests/test_gpu_reestimate_dlt.py: one rank of a sharded mh_select_greedy whose winners are refitted (mh_set_tuning
key 30) by the N-point DLT estimator (mh_set_estimator), over gloo on a shared GPU (the host-synchronised transport).  Prints one
JSON line per rank."""
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
THR2, N, M, SEED, NEED, MAX_MODELS = 6.25, 600, 600, 77, 20, 8
sc = mh.synth.make_scene(N, 3, seed=99, with_neighbours=False)
eng = mh.Engine(0, 2.6, 2.5, 0.005, 0.5, 20)
eng.set_tuning(5, 64)                                   # the ranks share one GPU: a quarter of the chip each
eng.set_correspondences(sc.src, sc.dst)                 # points alone
eng.set_epipolar(sc.F, sc.e2)                           # (for the rank that takes "3pt" in the mixed attempt: its engine lacks nothing)
hook = sh.make_allgather_hook(world, dev)
eng.set_transport(rank, world, host_fn=hook)
first, mine = sh.shard_range(M, world, rank)
out = {"rank": rank}


def attempt(name, estimator):
    try:
        eng.set_estimator(estimator)
        eng.set_tuning(30, 1)
        eng.propose_dlt4(SEED, first, mine)
        H, counters, counts, _ = eng.select_greedy(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8), total_m=M)
        out[name] = {"ok": True, "counters": counters.tolist(), "counts": counts.tolist(), "H": H.view(np.uint64).tolist()}
    except mh.MultiHError as ex:
        out[name] = {"ok": False, "code": ex.code, "msg": str(ex)}
    dist.barrier()


attempt("dlt_refit", "dlt")
# rank 0 refits by the DLT, rank 1 by the 3-point fit: the records' mode words differ in bits 2 and 24
attempt("mixed", "dlt" if rank == 0 else "3pt")
attempt("dlt_again", "dlt")
for r in range(world):                                  # one rank at a time: the launcher merges the ranks' stdout
    if r == rank:
        print(json.dumps(out), flush=True)
    dist.barrier()
eng.close()
dist.barrier()
dist.destroy_process_group()
