#!/usr/bin/env python3
"""Wall time of ONE validation pass over a fold-sized set of volumes through the two paths of wsl4mis_amd/val_2D.py, beside the
200 training steps a validation period consists of:

  host    test_single_volume per volume, as the trainers call it: scipy zoom per slice -> upload -> eval forward -> argmax -> download
          -> scipy zoom back -> numpy masks -> Dice on the host, HD95 through the device kernels (masks uploaded per class)
  device  VolumeValidator.run: volumes resident, wsl_val_zoom_in -> eval forward -> wsl_val_labelmap (+ Dice counts), one read of the
          counts per pass, HD95 on the resident label maps

    python tools/bench_val.py --out profiles/val_bench.md            # needs the GPU; there is no fallback

Inputs (all seeded, no dataset needed): 20 synthetic volumes of 10 x 256 x 216 (three nested structures; intensity follows the
label, plus noise) and the committed ACDC volume (tests/golden/acdc, 6 x 224 x 154); `unet`, patch 256 x 256.  The net is what 200
`pce` steps at batch size 12 on slices of the synthetic volumes leave -- so that the label maps have structures with surfaces, as a
net in training has -- and those 200 steps (and 200 at batch size 64) are timed as well: validation's share of a period.
The two paths' metrics are compared before anything is timed (Dice ==, HD95 1e-12).  Passes alternate between the paths; each ends
with its metrics on the host.  --emulator rehearses the flow on the host emulator at a tiny size: it times nothing, writes nothing."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def synthetic_volume(shape, seed):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    cy, cx = shape[1] / 2 + rng.uniform(-6, 6, shape[0]), shape[2] / 2 + rng.uniform(-6, 6, shape[0])
    q = shape[2] / 216.0
    r = np.sqrt((y - cy[:, None, None]) ** 2 + ((x - cx[:, None, None]) * 1.15) ** 2) + 3.0 * q * np.sin(0.2 * x / q) * np.cos(0.17 * y / q)
    lab = np.zeros(shape, np.uint8)
    for c, rad in ((1, 70), (2, 48), (3, 30)):
        lab[r < rad * q] = c
    img = (0.15 + 0.2 * lab + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    return {"image": img, "label": lab}


def acdc_volume():
    from wsl4mis_amd.dataloaders import h5lite
    with h5lite.File(os.path.join(ROOT, "tests", "golden", "acdc", "ACDC_training_volumes", "patient041_frame11.h5")) as f:
        return {"image": f["image"][:].astype(np.float32), "label": f["label"][:].astype(np.uint8)}


def training_set(volumes, patch):
    """every slice of the volumes at the patch size (order-0 zoom, like the loaders), dense labels"""
    from scipy.ndimage import zoom
    xs, ys = [], []
    for v in volumes:
        for img, lab in zip(v["image"], v["label"]):
            f = (patch[0] / img.shape[0], patch[1] / img.shape[1])
            xs.append(zoom(img, f, order=0)), ys.append(zoom(lab, f, order=0))
    return np.stack(xs)[:, None].astype(np.float32), np.stack(ys).astype(np.uint8)


def train_steps(eng, x, y, bs, steps, seed):
    """`steps` optimiser steps on random batches; returns the seconds they took, ending in the host read of the last loss"""
    import torch
    from wsl4mis_amd import runtime as rt
    rng = np.random.default_rng(seed)
    xd, yd = torch.from_numpy(x).to(rt.device()), torch.from_numpy(y).to(rt.device())
    idx = [torch.from_numpy(rng.integers(0, x.shape[0], bs)).to(rt.device()) for _ in range(steps)]
    batches = [(xd[i].contiguous(), yd[i].contiguous()) for i in idx[:8]]      # eight resident batches, cycled: the step alone is timed
    if not _lib_is_emulation():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        eng.step(*batches[k % len(batches)])
    loss = eng.losses()["loss"]
    return time.perf_counter() - t0, loss


def _lib_is_emulation():
    from wsl4mis_amd import _lib
    return _lib.is_test_emulation()


def host_pass(volumes, net, patch, with_hd95):
    from wsl4mis_amd import val_2D
    return np.array([val_2D.test_single_volume(v["image"], v["label"], net, 4, patch, with_hd95=with_hd95) for v in volumes], np.float64)


def stats(t):
    return {"n": len(t), "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed passes per path and setting (after one warm-up pass each)")
    ap.add_argument("--emulator", action="store_true", help="rehearsal on the host emulator at a tiny size: no timing, no file")
    args = ap.parse_args(argv)
    import torch
    from wsl4mis_amd import _lib, val_2D
    from wsl4mis_amd.engine import TrainEngine
    if args.emulator:
        import ctypes
        _lib.use_library_for_tests(ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libwslhip_emul.so")))
        volumes, patch, period, sizes = [synthetic_volume((2, 20, 24), s) for s in (1, 2)], (16, 16), 2, (2,)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_val needs the GPU: nothing is measured without it")
        volumes = [synthetic_volume((10, 256, 216), 100 + s) for s in range(20)] + [acdc_volume()]
        patch, period, sizes = (256, 256), 200, (12, 64)
    x, y = training_set(volumes[:20], patch)
    train, net = {}, None
    for bs in sizes:
        eng = TrainEngine("unet", 1, 4, loss="pce")
        train_steps(eng, x, y, bs, 2 if args.emulator else 20, seed=bs)                       # warm-up: code objects, workspaces
        train[bs] = train_steps(eng, x, y, bs, period, seed=1000 + bs)
        if net is None:
            net = eng.model                                                                   # the batch-size-12 net validates
    val = val_2D.VolumeValidator(volumes, 4, patch)
    # same results first
    settings, skipped = [], ""
    for hd in (False,) if args.emulator else (False, True):
        try:
            ref_hd = host_pass(volumes, net, patch, hd)
        except RuntimeError as e:                 # medpy's error: the net predicts a class one of the volumes lacks -- no HD95 row then
            skipped = f"HD95 was NOT measured: the host path raised '{e}' for this net."
            continue
        ref, got = ref_hd, val.run(net, with_hd95=hd)
        settings.append(hd)
        assert np.array_equal(got[..., 0], ref[..., 0]), "Dice differs between the paths"
        assert (np.abs(got[..., 1] - ref[..., 1]) <= 1e-12 * np.maximum(1.0, ref[..., 1])).all(), "HD95 differs between the paths"
    if args.emulator:
        print(f"rehearsal ok: {len(volumes)} volumes, metrics of the two paths agree, mean Dice {ref[..., 0].mean():.4f}; NOTHING MEASURED")
        return 0
    mean_dice = float(ref[..., 0].mean())
    print("compared; training", {bs: round(t, 3) for bs, (t, _) in train.items()}, "s; mean Dice", mean_dice, flush=True)
    t_up = time.perf_counter()
    val_2D.VolumeValidator(volumes, 4, patch)
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t_up
    rows = {}
    for hd in settings:
        th, td = [], []
        for _ in range(args.reps):                                                            # alternating: both see the same machine
            a = time.perf_counter()
            host_pass(volumes, net, patch, hd)
            b = time.perf_counter()
            val.run(net, with_hd95=hd)
            c = time.perf_counter()
            th.append(b - a), td.append(c - b)
        rows[hd] = (stats(th), stats(td))
    net.train()
    f = lambda r: f"{r['median_ms']:.1f} ({r['min_ms']:.1f} .. {r['max_ms']:.1f}, n = {r['n']})"  # noqa: E731
    prop = torch.cuda.get_device_properties(0)
    n_sl = sum(v["image"].shape[0] for v in volumes)
    lines = ["# One validation pass: host path and device path", "",
             f"`python tools/bench_val.py --out profiles/val_bench.md` on {torch.cuda.get_device_name(0)} ({prop.gcnArchName}, "
             f"{prop.multi_processor_count} CUs), torch {torch.__version__}.  {len(volumes)} volumes, {n_sl} slices (20 synthetic "
             "10 x 256 x 216 and the committed ACDC volume 6 x 224 x 154), `unet`, patch 256 x 256, 3 foreground classes.  The net is what "
             f"200 `pce` steps at batch size 12 on the synthetic slices leave (mean Dice of the pass {mean_dice:.4f}).  Wall time in ms, "
             f"median (min .. max) of {args.reps} passes after one warm-up pass per path, the paths alternating in one process; every "
             "pass ends with its metrics on the host.  The two paths' metrics were compared first (Dice equal, HD95 within 1e-12)."
             "  The last column is the ratio of the unrounded medians, so it can differ in the last digit from the quotient of the rounded columns.", "",
             "| | host path (`test_single_volume` per volume) | device path (`VolumeValidator.run`) | host / device |",
             "|---|---|---|---|"]
    for hd in settings:
        h, d = rows[hd]
        lines.append(f"| {'Dice and HD95' if hd else 'Dice only (`--no_hd95`)'} | {f(h)} | {f(d)} | {h['median_ms'] / d['median_ms']:.2f} |")
    if skipped:
        lines += ["", skipped]
    lines += ["", f"Building the `VolumeValidator` (one upload of all volumes, once per training run): {1e3 * t_up:.1f} ms.", "",
              "## Beside the training steps of one validation period", "",
              "200 optimiser steps of `pce` on resident batches, timed in the same process (host clock, ending in the read of the loss):", "",
              "| batch size | 200 steps, ms | host pass / period (Dice and HD95) | device pass / period (Dice and HD95) | host pass / period (Dice only) | "
              "device pass / period (Dice only) |", "|---|---|---|---|---|---|"]
    for bs in sizes:
        ms = 1e3 * train[bs][0]
        share = lambda hd, k: f"{rows[hd][k]['median_ms'] / ms:.2f}" if hd in rows else "not measured"  # noqa: E731
        lines.append(f"| {bs} | {ms:.0f} | {share(True, 0)} | {share(True, 1)} | {share(False, 0)} | {share(False, 1)} |")
    lines += ["", "(pass / period = the pass's median over the time of the 200 steps: 1.00 means validation costs as much as the training "
              "between two validations.  A fold of ACDC has about twice these slices; one rank of a data-parallel run validates its share.)"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
