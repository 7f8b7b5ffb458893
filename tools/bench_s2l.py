"""Scribble2Label on cuda:0: what the fused loss head and the ensemble update cost (unet, 256 x 256).  Three sub-commands, meant to be
chained, each under its own time limit, the profiler in a run of its own:

  timeout 900 python tools/bench_s2l.py run --out profiles/s2l_bench.json &&
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o s2l -- python tools/bench_s2l.py head &&
  python tools/bench_s2l.py merge --stats <dir> --out profiles/s2l_bench.json &&
  python tools/bench_s2l.py table --out profiles/s2l_bench.json

run    a. engine `pce` slices/s            b. engine `s2l` slices/s from thr_iter on
       c. the same net, optimiser and step with the S2L loss composed from stock torch GPU ops as the reference writes it
          (train_s2l.py:124-147, everything kept on the GPU: the reference's .cpu() round trips are not charged)
       d. update_ensemble() per 1000 slices, mode "reference" (one train-mode forward per slice) and mode "eval" (batched)
       and what follows from them: b / a, b / c, the share of a 100-step period the reference-mode update of 1512 slices (an ACDC
       fold's training set) takes at bs 12 and at bs 64.  Warm-up and three timed regions per figure, medians, device events.
head   the fused head alone, 20 calls at bs 64 (what the profiler run traces)
merge  e. the head's kernel times from the profiler's kernel statistics: bytes per pixel the algorithm moves (from the shapes) over
       the summed kernel time, as a fraction of the HBM peak (8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches)
table  the record as a markdown table next to it (profiles/s2l_bench.md)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12
# the 4-class head per pixel: pass 1 reads 16 B logits + 1 B scribble + 16 B weights, writes 1 B target; pass 2 reads the target and
# (where any of four neighbouring pixels carries a loss) 16 B logits, writes 16 B gradient
HEAD_BYTES_PASS1, HEAD_BYTES_PASS2 = 34.0, 33.0


def timed(fn, steps, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return statistics.median(ms), [round(m, 3) for m in ms]


def s2l_inputs(bs, size, dev, torch):
    from wsl4mis_amd.synthetic import batch
    x, lab = batch(bs, size, size, 1, dev)
    g = torch.Generator().manual_seed(5)
    w = torch.rand((bs, size, size, 4), generator=g) * 0.7
    hot = torch.rand((bs, size, size), generator=g) < 0.6          # a store well into training: most pixels confident
    w[hot, torch.randint(0, 4, (bs, size, size), generator=g)[hot]] = 0.95
    return x, lab, w.to(dev)


def torch_s2l_loss(outputs, label_batch, weight_batch, thr_conf):
    """train_s2l.py:124-147 on the GPU"""
    import torch
    import torch.nn.functional as F
    loss_ce = F.cross_entropy(outputs, label_batch.long(), ignore_index=4)
    scribbles = label_batch.long()
    u = []
    for c in range(4):
        m = weight_batch[..., c]
        u.append(torch.where((m > thr_conf) & (scribbles == 4), torch.zeros_like(m) + c, 4. * torch.ones_like(scribbles)))
    u_labels = torch.ones_like(u[0]).long() * 4
    for c in range(4):
        u_labels[u[c] == c] = c
    loss_u = F.cross_entropy(outputs, u_labels, ignore_index=4)
    return loss_ce + 0.5 * loss_u


def synthetic_dataset(n, torch):
    import numpy as np
    from wsl4mis_amd.dataloaders.dataset_s2l import BaseDataSets_s2l
    rng = np.random.default_rng(7)
    sizes = [(256, 216), (216, 256), (224, 154), (232, 256), (256, 256), (428, 512), (174, 208), (154, 224)]     # ACDC's native sizes
    return BaseDataSets_s2l.from_slices([{"image": rng.random(sizes[i % len(sizes)], dtype=np.float32),
                                          "mask": np.zeros(sizes[i % len(sizes)], np.uint8),
                                          "scribble": np.full(sizes[i % len(sizes)], 4, np.uint16)} for i in range(n)])


def cmd_run(a):
    import torch
    from wsl4mis_amd import _lib
    from wsl4mis_amd import runtime as rt
    from wsl4mis_amd.engine import TrainEngine
    assert torch.cuda.is_available(), "bench_s2l needs cuda:0"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"tool": "bench_s2l", "net": "unet", "size": a.size, "steps_per_region": a.steps, "warmup": a.warmup,
           "library_sha": _lib.library_sha256(), "tree_sha": _lib.source_sha256()}
    for bs in (64, 12):
        x, lab, w = s2l_inputs(bs, a.size, dev, torch)
        r = {}
        eng = TrainEngine("unet", 1, 4, loss="pce")
        ms, reg = timed(lambda: eng.step(x, lab), a.steps, a.warmup, torch)
        r["a_pce"] = {"ms_per_step": round(ms, 3), "slices_per_s": round(bs / ms * 1e3, 1), "regions_ms": reg}
        eng = TrainEngine("unet", 1, 4, loss="s2l", thr_iter=0)
        ms, reg = timed(lambda: eng.step(x, lab, weight=w), a.steps, a.warmup, torch)
        o = eng.losses()
        r["b_s2l"] = {"ms_per_step": round(ms, 3), "slices_per_s": round(bs / ms * 1e3, 1), "regions_ms": reg, "loss": o["loss"],
                      "n_u_share": o["n_u"] / (bs * a.size * a.size)}
        eng = TrainEngine("unet", 1, 4, loss="pce")

        def torch_chain_step():
            m = eng.model
            z = m._run_forward(x, keep_for_backward=True)[0].requires_grad_()
            loss = torch_s2l_loss(z, lab, w, 0.8)
            (dz,) = torch.autograd.grad(loss, z)
            m._run_backward(x, [dz, None])
            eng.optimizer_step()
            torch_chain_step.loss = loss

        ms, reg = timed(torch_chain_step, a.steps, a.warmup, torch)
        r["c_torch_chain"] = {"ms_per_step": round(ms, 3), "slices_per_s": round(bs / ms * 1e3, 1), "regions_ms": reg,
                              "loss": float(torch_chain_step.loss)}
        r["b_over_a"] = round(r["b_s2l"]["slices_per_s"] / r["a_pce"]["slices_per_s"], 4)
        r["b_over_c"] = round(r["b_s2l"]["slices_per_s"] / r["c_torch_chain"]["slices_per_s"], 4)
        res[f"bs{bs}"] = r
        del eng
        rt._ws_cache.clear()
        torch.cuda.empty_cache()
    # d. the update pass
    n = a.update_slices
    eng = TrainEngine("unet", 1, 4, loss="s2l")
    ds = synthetic_dataset(n, torch)
    upd = {}
    for mode in ("reference", "eval"):
        ms, reg = timed(lambda: eng.update_ensemble(ds, mode=mode, patch_size=(a.size, a.size), batch_size=64), 1, 1, torch)
        upd[mode] = {"slices": n, "ms_per_pass": round(ms, 2), "s_per_1000_slices": round(ms / n, 4), "regions_ms": reg}
    res["d_update_ensemble"] = upd
    ref_s = upd["reference"]["s_per_1000_slices"] * 1.512
    for bs in (12, 64):
        period = 100 * res[f"bs{bs}"]["b_s2l"]["ms_per_step"] / 1e3
        res[f"bs{bs}"]["reference_update_share_of_a_100_step_period_1512_slices"] = round(ref_s / (ref_s + period), 4)
        res[f"bs{bs}"]["eval_update_share_of_a_100_step_period_1512_slices"] = round(
            upd["eval"]["s_per_1000_slices"] * 1.512 / (upd["eval"]["s_per_1000_slices"] * 1.512 + period), 4)
    write(a.out, res)
    assert res["bs64"]["b_over_c"] >= 1.0, ("the fused head loses to the torch chain", res["bs64"])


def write(path, res):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def cmd_head(a):
    import torch
    from wsl4mis_amd.utils import losses
    dev = torch.device("cuda:0")
    x, lab, w = s2l_inputs(64, a.size, dev, torch)
    z = torch.randn((64, 4, a.size, a.size), device=dev)
    for _ in range(20):
        losses.s2l_head(z, lab, w)
    torch.cuda.synchronize()
    print("head: 20 calls at 64 x 4 x %d x %d" % (a.size, a.size))


def cmd_merge(a):
    rows = []
    for f in glob.glob(os.path.join(a.stats, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    pick = {k: [r for r in rows if k in r["Name"]] for k in ("s2l_reduce4_kernel", "s2l_finalize_kernel", "s2l_bwd4_kernel")}
    assert all(len(v) == 1 for v in pick.values()), {k: len(v) for k, v in pick.items()}
    px = 64 * a.size * a.size
    ns = {k: float(v[0]["AverageNs"]) for k, v in pick.items()}
    e = {"pixels": px, "calls": int(pick["s2l_reduce4_kernel"][0]["Calls"]), "kernel_us": {k: round(v / 1e3, 2) for k, v in ns.items()},
         "bytes_per_pixel": {"pass1": HEAD_BYTES_PASS1, "pass2": HEAD_BYTES_PASS2, "total": HEAD_BYTES_PASS1 + HEAD_BYTES_PASS2},
         "hbm_fraction_of_8.0TBs": {"pass1": round(px * HEAD_BYTES_PASS1 / (ns["s2l_reduce4_kernel"] * 1e-9) / HBM_PEAK, 4),
                                    "pass2": round(px * HEAD_BYTES_PASS2 / (ns["s2l_bwd4_kernel"] * 1e-9) / HBM_PEAK, 4),
                                    "head": round(px * (HEAD_BYTES_PASS1 + HEAD_BYTES_PASS2) / (sum(ns.values()) * 1e-9) / HBM_PEAK, 4)},
         "note": "fraction of the %.1f TB/s spec peak; a float4 copy reaches %.2f TB/s = %.2f" % (HBM_PEAK / 1e12, HBM_COPY / 1e12, HBM_COPY / HBM_PEAK)}
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    res["e_head_kernels"] = e
    write(a.out, res)


def cmd_table(a):
    """the record of --out as a markdown table next to it (profiles/s2l_bench.md)"""
    r = json.load(open(a.out))
    L = ["# Scribble2Label: fused head and ensemble update (tools/bench_s2l.py)", "",
         "unet, %d x %d, f32; %d warm-up steps, three timed regions of %d steps per figure, the median region; one run on one MI355X.  "
         "Record: `%s`." % (r["size"], r["size"], r["warmup"], r["steps_per_region"], os.path.basename(a.out)), "",
         "| batch | a. engine `pce` slices/s | b. engine `s2l` slices/s | c. torch-chain loss slices/s | b / a | b / c | "
         "reference-mode update, share of a 100-step period | eval-mode update, share |", "|---|---|---|---|---|---|---|---|"]
    for bs in (64, 12):
        b = r[f"bs{bs}"]
        L.append("| %d | %.1f (%.2f ms) | %.1f (%.2f ms) | %.1f (%.2f ms) | %.3f | %.3f | %.1f %% | %.1f %% |" % (
            bs, b["a_pce"]["slices_per_s"], b["a_pce"]["ms_per_step"], b["b_s2l"]["slices_per_s"], b["b_s2l"]["ms_per_step"],
            b["c_torch_chain"]["slices_per_s"], b["c_torch_chain"]["ms_per_step"], b["b_over_a"], b["b_over_c"],
            100 * b["reference_update_share_of_a_100_step_period_1512_slices"], 100 * b["eval_update_share_of_a_100_step_period_1512_slices"]))
    u = r["d_update_ensemble"]
    L += ["", "The update shares are for the 1512 training slices of an ACDC fold, from d. below and b.'s step time.", "",
          "| d. `update_ensemble` | slices timed | s per 1000 slices |", "|---|---|---|"]
    L += ["| mode `%s` | %d | %.3f |" % (m, u[m]["slices"], u[m]["s_per_1000_slices"]) for m in ("reference", "eval")]
    e = r.get("e_head_kernels")
    if e:
        k, f = e["kernel_us"], e["hbm_fraction_of_8.0TBs"]
        L += ["", "e. the head alone at bs 64 (`rocprofv3 --kernel-trace --stats`, a run of its own, %d calls): %.0f B per pixel "
              "(%.0f pass 1 + %.0f pass 2, from the shapes)." % (e["calls"], e["bytes_per_pixel"]["total"], e["bytes_per_pixel"]["pass1"],
                                                                 e["bytes_per_pixel"]["pass2"]), "",
              "| kernel | mean us | algorithmic bytes / time, fraction of 8.0 TB/s |", "|---|---|---|",
              "| `s2l_reduce4_kernel` (pass 1) | %.2f | %.3f |" % (k["s2l_reduce4_kernel"], f["pass1"]),
              "| `s2l_finalize_kernel` | %.2f | |" % k["s2l_finalize_kernel"],
              "| `s2l_bwd4_kernel` (pass 2) | %.2f | %.3f |" % (k["s2l_bwd4_kernel"], f["pass2"]),
              "| head, all three | %.2f | %.3f |" % (sum(k.values()), f["head"]), "", e["note"] + "."]
    path = os.path.splitext(a.out)[0] + ".md"
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "head", "merge", "table"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50, help="steps per timed region (bench.py's default)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--update_slices", type=int, default=128)
    ap.add_argument("--stats", default=None, help="merge: the profiler's output directory")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"run": cmd_run, "head": cmd_head, "merge": cmd_merge, "table": cmd_table}[a.cmd](a)


if __name__ == "__main__":
    main()
