"""PNet2D training-step throughput (net_factory("pnet", 1, 4): F 64, dilations 1, 2, 4, 8, 16) through TrainEngine on cuda:0; prints
one JSON line.  Slices/s and ms/step are the median of 3 timed regions after warm-up; `roofline_frac` is the algorithmic fraction of
the f32 MFMA peak (157.3 TF) at 190.3 GFLOP per slice (direct-conv flops of forward + data + weight gradients at 256 x 256).

  python tools/bench_pnet.py [--loss pce|pce_gatedcrf] [--bs 64] [--size 256] [--steps 3] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from wsl4mis_amd import _lib  # noqa: E402
from wsl4mis_amd.engine import TrainEngine  # noqa: E402
from wsl4mis_amd.synthetic import batch  # noqa: E402

PEAK_TF = 157.3
GFLOP_PER_SLICE_256 = 190.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", default="pce", choices=["pce", "pce_gatedcrf"])
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3, help="steps per timed region")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eng = TrainEngine("pnet", 1, 4, loss=a.loss, crf_radius=5)
    x, lab = batch(a.bs, a.size, a.size, 1, dev)
    for _ in range(a.warmup):
        eng.step(x, lab)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            eng.step(x, lab)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.steps)
    step_ms = statistics.median(ms)
    sps = a.bs / (step_ms / 1e3)
    gflop = GFLOP_PER_SLICE_256 * (a.size / 256) ** 2
    print(json.dumps({"tool": "bench_pnet", "loss": a.loss, "bs": a.bs, "size": a.size, "ms_per_step": round(step_ms, 3),
                      "slices_per_s": round(sps, 2), "regions_ms": [round(m, 3) for m in ms],
                      "roofline_frac": round(sps * gflop / (PEAK_TF * 1e3), 4), "loss_value": eng.losses()["loss"],
                      "library_sha": _lib.library_sha256(), "tree_sha": _lib.source_sha256()}))


if __name__ == "__main__":
    main()
