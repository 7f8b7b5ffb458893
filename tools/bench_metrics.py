#!/usr/bin/env python3
"""Wall time of ONE volume's full evaluation in the offline test stage -- 3 classes x (Dice, HD95, ASD) with a voxel spacing
(wsl4mis_amd/test_2D_fully.py::calculate_metric_percase: label volumes uploaded once, surfaces and nearest-surface distances on
the device) -- beside the scipy restatement of what the reference runs (medpy: tests/metrics_sp_ref.py) on the same machine's host.

    python tools/bench_metrics.py --out profiles/metrics_bench.md        # needs the GPU; there is no fallback

Volumes: the committed ACDC volume (tests/golden/acdc, patient041_frame11, 6 x 224 x 154) with its label as ground truth and a
displaced, eroded copy as prediction; and a synthetic 10 x 256 x 216 volume of three nested structures.  Both are seeded.
Each arm is warmed up, then repeated for at least --seconds and --reps; every device repetition ends in a device -> host read of
the results (a synchronise).  The host arm is given sequentially and with the three classes in three processes (the restatement
has no finer parallelism: scipy's distance transform is single-threaded).  The two arms' results are compared before any time
is reported.  --emulator runs the same flow on the host emulator at a tiny size to rehearse it: it times nothing and writes nothing."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
from scipy.ndimage import binary_erosion  # noqa: E402


def acdc_volume():
    from wsl4mis_amd.dataloaders import h5lite
    with h5lite.File(os.path.join(ROOT, "tests", "golden", "acdc", "ACDC_training_volumes", "patient041_frame11.h5")) as f:
        lab = f["label"][:]
    pred = np.zeros_like(lab)
    for c in (1, 2, 3):                                           # a plausible prediction: each class eroded in plane and displaced
        m = binary_erosion(lab == c, structure=np.ones((1, 3, 3), bool))
        pred[np.roll(m, (2, -3), axis=(1, 2))] = c
    return pred, lab, (10.0, 1.5625, 1.5625)


def synthetic_volume(shape=(10, 256, 216), seed=7):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    out = []
    for k in range(2):                                            # ground truth, prediction: three nested rings, jittered per slice
        cy, cx = shape[1] / 2 + rng.uniform(-6, 6, shape[0]), shape[2] / 2 + rng.uniform(-6, 6, shape[0])
        r = np.sqrt((y - cy[:, None, None]) ** 2 + ((x - cx[:, None, None]) * 1.15) ** 2) + 3.0 * np.sin(0.2 * x + k) * np.cos(0.17 * y)
        v, q = np.zeros(shape, np.uint8), shape[2] / 216.0
        v[r < (70 + 4 * k) * q] = 1
        v[r < (48 + 3 * k) * q] = 2
        v[r < (30 - 2 * k) * q] = 3
        out.append(v)
    return out[1], out[0], (10.0, 1.40625, 1.40625)


def device_eval(pred_d, lab_d, spacing):
    from wsl4mis_amd.test_2D_fully import calculate_metric_percase
    return [calculate_metric_percase(pred_d == c, lab_d == c, spacing) for c in (1, 2, 3)]


def _host_class(args):
    import metrics_sp_ref as M
    pred, lab, c, spacing = args
    return M.calculate_metric_percase(pred == c, lab == c, spacing)


def host_eval(pred, lab, spacing, pool=None):
    jobs = [(pred, lab, c, spacing) for c in (1, 2, 3)]
    return pool.map(_host_class, jobs) if pool is not None else [_host_class(j) for j in jobs]


def timed(fn, seconds, reps):
    for _ in range(3):
        fn()
    t, t0 = [], time.perf_counter()
    while len(t) < reps or time.perf_counter() - t0 < seconds:
        a = time.perf_counter()
        fn()
        t.append(time.perf_counter() - a)
    return {"n": len(t), "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--emulator", action="store_true", help="rehearsal on the host emulator at a tiny size: no timing, no file")
    args = ap.parse_args(argv)
    import torch
    from wsl4mis_amd import _lib
    from wsl4mis_amd import runtime as rt
    if args.emulator:
        import ctypes
        _lib.use_library_for_tests(ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libwslhip_emul.so")))
        volumes = [("synthetic 3 x 48 x 40", synthetic_volume((3, 48, 40)))]
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_metrics needs the GPU: nothing is measured without it")
        volumes = [("ACDC patient041_frame11, 6 x 224 x 154", acdc_volume()), ("synthetic 10 x 256 x 216", synthetic_volume())]
    import multiprocessing as mp
    rows = []
    with mp.get_context("spawn").Pool(3) as pool:
        for name, (pred, lab, spacing) in volumes:
            pred_d, lab_d = torch.from_numpy(pred).to(rt.device()), torch.from_numpy(lab).to(rt.device())
            got, ref = device_eval(pred_d, lab_d, spacing), host_eval(pred, lab, spacing)
            for g, r in zip(got, ref):                            # same results first (bounds of tests/test_metrics_spacing.py)
                assert g[0] == r[0] and abs(g[1] - r[1]) <= 1e-12 * max(1.0, r[1]) and abs(g[2] - r[2]) <= 1e-10 * r[2], (name, g, r)
            from wsl4mis_amd import val_2D
            pts = [int(val_2D._surface_points(m == c).shape[0]) for c in (1, 2, 3) for m in (pred_d, lab_d)]
            if args.emulator:
                print(f"rehearsal ok ({name}): results agree; surface points {pts}; NOTHING MEASURED")
                continue

            def with_upload():
                return device_eval(torch.from_numpy(pred).to(rt.device()), torch.from_numpy(lab).to(rt.device()), spacing)
            rows.append((name, pts, timed(with_upload, args.seconds, args.reps),
                         timed(lambda: device_eval(pred_d, lab_d, spacing), args.seconds, args.reps),
                         timed(lambda: host_eval(pred, lab, spacing), args.seconds, 5),
                         timed(lambda: host_eval(pred, lab, spacing, pool), args.seconds, 5)))
    if args.emulator:
        return 0
    f = lambda r: f"{r['median_ms']:.2f} ({r['min_ms']:.2f} .. {r['max_ms']:.2f}, n = {r['n']})"
    lines = ["# Offline test stage: one volume's evaluation (3 classes x Dice / HD95 / ASD, spacing in mm)", "",
             f"`tools/bench_metrics.py` on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs), torch {torch.__version__}; wall time in ms, median (min .. max) "
             "after 3 warm-up calls; every device call ends in a device -> host read.  The host arm is the scipy restatement of medpy "
             "(`tests/metrics_sp_ref.py`) on the same machine's CPU, sequential and with the three classes in three processes.  "
             "Results of the two arms agree within the test bounds (asserted before timing).", "",
             "| volume | surface points (pred, gt per class) | device, incl. upload | device, volumes resident | host, sequential | host, 3 processes |",
             "|---|---|---|---|---|---|"]
    for name, pts, up, res, h1, h3 in rows:
        lines.append(f"| {name} | {pts} | {f(up)} | {f(res)} | {f(h1)} | {f(h3)} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
