"""Inputs of tests/test_semi_engine.py and the worker of its two-rank test: one rank of a world-size-2 data-parallel `semi_mt` step on
the CPU (gloo) with the kernel sources running in the host emulator.  Writes the all-reduced gradient and the parameters after the step
to an .npz for the parent test (as tests/dp_worker.py does for the single-forward compositions)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

# generator seeds, searched so that no pre-activation / pooling window of either student forward lies within fp32 noise of a LeakyReLU /
# max-pool kink (1e-5 for the one-step batch, the 4e-6 / 1e-6 of tests/test_dp.py for the 32 x 32 shards); the tests re-check the
# margins with the oracle.  STEP: the one-step tests; (rank): the shards of the two-rank test
STEP_SEED = 69
SHARD_SEEDS = {0: 80, 1: 321}
SHARD_SHAPE = (2, 2, 32)        # N_l, N_u, size of a rank's shard: the 2 x 32 x 32 of tests/dp_worker.py per half
IT0, MAX_IT = 30000, 60000


def semi_inputs(seed, N_l=3, N_u=2, S=16):
    """labeled batch + dense labels, unlabeled batch, the teacher's noises (1 + 4 double batches) and every dropout mask of one step"""
    from oracle import torch_ref as R
    gen = torch.Generator().manual_seed(seed)

    def masks(n):
        return [(torch.rand((n, 16 << l, S >> l, S >> l), generator=gen) >= R.DROP[l]).to(torch.uint8) for l in range(5)]
    d = {"x_l": torch.rand((N_l, 1, S, S), generator=gen), "x_u": torch.rand((N_u, 1, S, S), generator=gen),
         "lab": torch.randint(0, 4, (N_l, S, S), generator=gen).to(torch.uint8)}
    d["m_l"], d["m_u"] = masks(N_l), masks(N_u)
    d["m_t"] = {N_u: masks(N_u), 2 * N_u: masks(2 * N_u)}
    d["noise"] = [torch.clamp(torch.randn((N_u, 1, S, S), generator=gen) * 0.1, -0.2, 0.2)] + \
                 [torch.clamp(torch.randn((2 * N_u, 1, S, S), generator=gen) * 0.1, -0.2, 0.2) for _ in range(4)]
    return d


def run_rank(rank, world, outdir):
    import torch.distributed as dist
    from detinit import det_state
    from wsl4mis_amd.engine import TrainEngine
    eng = TrainEngine("unet", 1, 4, base_lr=0.01, max_iterations=MAX_IT, loss="semi_mt")
    assert eng.dp and eng.world == world
    for i, m in enumerate((eng.model, eng.teacher)):
        vals = det_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, (23 + i) if rank == 0 else 777 + i)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
        dist.broadcast(m._param_arena, src=0)          # rank 1 was given OTHER weights: what the engine does at construction
        dist.broadcast(m._buf_arena, src=0)
    d = semi_inputs(SHARD_SEEDS[rank], *SHARD_SHAPE)
    eng.it = IT0
    eng.teacher.set_dropout_masks(d["m_t"][d["x_u"].shape[0]])
    eng.forward_backward(d["x_l"], d["lab"], unlabeled=d["x_u"], noise=d["noise"][0], masks=(d["m_l"], d["m_u"]))
    out = {"loss": np.float32(eng.losses()["loss"]), "grads": (eng.model.flat_grads() / world).numpy().copy()}
    eng.optimizer_step()
    out["params_after"] = eng.model.flat_params().numpy().copy()
    out["teacher_after"] = eng.teacher.flat_params().numpy().copy()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)


def main():
    import torch.distributed as dist
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from wsl4mis_amd import _lib
    _lib.use_library_for_tests(C.CDLL(os.path.join(ROOT, "tests", "emul", "libwslhip_emul.so")))
    run_rank(rank, world, outdir)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
