"""Worker of the two-rank test of tests/test_dan_engine.py: one rank of a world-size-2 data-parallel `semi_dan` step on the CPU (gloo)
with the kernel sources running in the host emulator.  After the data-parallel generator update every rank computes the discriminator
gradient of its OWN shard the way a 1-rank engine would (from the state the generator update left), restores the discriminator, and then
runs the data-parallel discriminator update; the parent checks that the update is one Adam step on the mean of the two shard gradients."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dan_ref as R  # noqa: E402
import semi_dp_worker as W  # noqa: E402

NDF, DAN_SEED = 8, 9


def dan_masks(rank, n):
    g = torch.Generator().manual_seed(500 + rank)
    return [(torch.rand((n, c * NDF), generator=g) >= 0.5).float() * 2 for c in (2, 4)]


def run_rank(rank, world, outdir):
    import torch.distributed as dist
    from detinit import det_state
    from wsl4mis_amd.engine import TrainEngine
    eng = TrainEngine("unet", 1, 4, base_lr=0.01, max_iterations=W.MAX_IT, loss="semi_dan", consistency_rampup=0, dan_ndf=NDF, dan_pool=1)
    assert eng.dp and eng.world == world
    m, D = eng.model, eng.discriminator
    vals = det_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, 23 if rank == 0 else 777)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    D.load_state_dict(R.rand_state(DAN_SEED + 100 * rank, 4, NDF, 1))
    for arena in (m._param_arena, m._buf_arena, D._param_arena):      # rank 1 was given OTHER weights: what the engine does at construction
        dist.broadcast(arena, src=0)
    d = W.semi_inputs(W.SHARD_SEEDS[rank], *W.SHARD_SHAPE)
    eng.it = W.IT0
    eng.forward_backward(d["x_l"], d["lab"], unlabeled=d["x_u"], masks=(d["m_l"], d["m_u"]))
    eng.optimizer_step()
    masks = dan_masks(rank, d["x_l"].shape[0] + d["x_u"].shape[0])
    out = {"dan_before": D.flat_params().numpy().copy(), "net_after": m.flat_params().numpy().copy()}
    # ---- the shard's own gradient, as a 1-rank engine computes it from this state; then the discriminator is put back
    eng.dp, eng.world = False, 1
    eng.discriminator_step(d["x_l"], d["x_u"], masks)
    out["shard_grad"] = D.flat_grads().numpy().copy()
    with torch.no_grad():
        D._param_arena[:D.n_param].copy_(torch.from_numpy(out["dan_before"]))
        eng.dan_m.zero_(), eng.dan_v.zero_()
    eng.dan_it, eng.dp, eng.world = 0, True, world
    # ---- the data-parallel update
    eng.discriminator_step(d["x_l"], d["x_u"], masks)
    out["dan_after"] = D.flat_params().numpy().copy()
    out["dan_loss"] = np.float32(eng.losses()["dan_loss"])
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
