"""Worker of tests/test_gpu_propose_3pt.py: one rank of a sharded mh_select_greedy over a batch of 3-point proposals
(mh_propose_3pt), over gloo on a shared GPU (the host-synchronised transport).  Prints one JSON line per rank."""
import ctypes as C
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
eng.set_correspondences(sc.src, sc.dst, sc.aff)
eng.set_epipolar(sc.F, sc.e2)
hook = sh.make_allgather_hook(world, dev)
eng.set_transport(rank, world, host_fn=hook)
first, mine = sh.shard_range(M, world, rank)
out = {"rank": rank}


def attempt(name, three, refit):
    try:
        eng.set_tuning(30, refit)
        if three:
            eng.propose_3pt(SEED, first, mine)
        else:
            eng.propose_dlt4(SEED, first, mine)
        H, counters, counts, _ = eng.select_greedy(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8), total_m=M)
        out[name] = {"ok": True, "counters": counters.tolist(), "counts": counts.tolist(), "H": H.view(np.uint64).tolist()}
    except mh.MultiHError as ex:
        out[name] = {"ok": False, "code": ex.code, "msg": str(ex)}
    dist.barrier()


attempt("p3", True, 0)
attempt("p3_refit", True, 1)
# rank 0 proposes 3-point hypotheses, rank 1 DLT ones: the records' mode words differ in bit 23
attempt("mixed", rank == 0, 0)
attempt("p3_again", True, 0)


# The host class over a batch smaller than the world: ONE hypothesis, so rank 1's shard is empty.  It still proposes (m = 0) and
# so carries the batch's record into the selection; the result is the unsharded one.  (Seed 6: the tuple of counter 0 lies on
# one plane of this scene.)
def process(sharded):
    host.mhh_set_sharding(rank if sharded else 0, world if sharded else 1, hook if sharded else None, None)
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((16, 9))
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.5), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(6), 1, 8, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 16, None, None, None, 0, 4)
    dist.barrier()
    return {"k": int(k), "labels": labels.tolist(), "H": Hout[:max(k, 0)].view(np.uint64).tolist()}


host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
host.mhh_set_engine_tuning(5, 64)
host.mhh_set_proposal_source(2, 0, 1)
try:
    out["class_empty_shard"] = process(True)
    out["class_unsharded"] = process(False)
finally:
    host.mhh_set_proposal_source(0, 16, 1)
    host.mhh_set_sharding(0, 1, None, None)
for r in range(world):                                  # one rank at a time: the launcher merges the ranks' stdout
    if r == rank:
        print(json.dumps(out), flush=True)
    dist.barrier()
eng.close()
dist.barrier()
dist.destroy_process_group()
