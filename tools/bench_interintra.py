"""Inter/intra-class variance training on cuda:0: what the regulariser costs (unet, 256 x 256).  Sub-commands meant to be chained, each
under its own time limit, the profiler in a run of its own (the method of tools/bench_s2l.py):

  timeout 900 python tools/bench_interintra.py run --out profiles/interintra_bench.json &&
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ii -- python tools/bench_interintra.py term &&
  python tools/bench_interintra.py merge --stats <dir> --out profiles/interintra_bench.json &&
  python tools/bench_interintra.py table --out profiles/interintra_bench.json

run    at bs 64 and bs 12 (the reference's batch), slices/s of
         a. engine `pce`            b. engine `pce_interintra`, fused head          c. engine `pce_interintra`, chain of calls
         d. the same net, optimiser and step with the loss composed from stock torch GPU ops as the trainer writes it
            (train_weakly_supervised_pCE_Inter&Intra_Class_2D.py:30-37,112-118)      m. engine `pce_ms` (the Mumford-Shah composition)
       and the two stand-alone entry points at bs 64 x 4 classes: wsl_class_variance_fwd_bwd against wsl_mumford_shah_fwd_bwd (the
       expectation to confirm or refute: the term costs about what Mumford-Shah does -- two reads of s + img and one ds write).
       Warm-up and three timed regions per figure, medians, device events.
term   wsl_class_variance_fwd_bwd alone, 20 calls at bs 64 (what the profiler run traces)
merge  the three kernels' times from the profiler's kernel statistics, with the bytes per pixel the algorithm moves (from the shapes)
       over the kernel time as a fraction of the HBM peak
table  the record as a markdown table next to it (profiles/interintra_bench.md)
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
# 4 classes, per pixel: the moment pass reads 16 B of s + 4 B of image; the gradient pass reads them again and writes 16 B
BYTES_MOMENT, BYTES_GRAD = 20.0, 36.0
KERNELS = ("cv_moment_kernel", "cv_coef_kernel", "cv_grad_kernel")


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


def torch_loss(outputs, volume_batch, label_batch, w):
    """the trainer's loss lines on the GPU"""
    import torch
    import torch.nn.functional as F
    outputs_soft = torch.softmax(outputs, dim=1)
    q = volume_batch * outputs_soft
    intra = torch.std(q, dim=[2, 3]).mean()
    inter = torch.std(q.mean(dim=[2, 3]), dim=1).mean()
    return F.cross_entropy(outputs, label_batch.long(), ignore_index=4) + w * (inter - intra)


def cmd_run(a):
    import torch
    from wsl4mis_amd import _lib
    from wsl4mis_amd import runtime as rt
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import batch
    assert torch.cuda.is_available(), "bench_interintra needs cuda:0"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"tool": "bench_interintra", "net": "unet", "size": a.size, "steps_per_region": a.steps, "warmup": a.warmup,
           "library_sha": _lib.library_sha256(), "tree_sha": _lib.source_sha256()}
    for bs in (64, 12):
        x, lab = batch(bs, a.size, a.size, 1, dev)
        r = {}

        def rate(key, eng, fn=None):
            ms, reg = timed(fn or (lambda: eng.step(x, lab)), a.steps, a.warmup, torch)
            r[key] = {"ms_per_step": round(ms, 3), "slices_per_s": round(bs / ms * 1e3, 1), "regions_ms": reg}

        rate("a_pce", TrainEngine("unet", 1, 4, loss="pce"))
        eng = TrainEngine("unet", 1, 4, loss="pce_interintra", var_rampup=0)
        rate("b_fused", eng)
        r["b_fused"]["losses"] = eng.losses()
        eng = TrainEngine("unet", 1, 4, loss="pce_interintra", var_rampup=0)
        eng.fused_heads = False
        rate("c_chain", eng)
        rate("m_pce_ms", TrainEngine("unet", 1, 4, loss="pce_ms"))
        eng = TrainEngine("unet", 1, 4, loss="pce")

        def torch_chain_step():
            m = eng.model
            z = m._run_forward(x, keep_for_backward=True)[0].requires_grad_()
            (dz,) = torch.autograd.grad(torch_loss(z, x, lab, 0.1), z)
            m._run_backward(x, [dz, None])
            eng.optimizer_step()

        rate("d_torch_chain", eng, torch_chain_step)
        for k in ("b_fused", "c_chain", "d_torch_chain", "m_pce_ms"):
            r[k + "_over_a"] = round(r[k]["slices_per_s"] / r["a_pce"]["slices_per_s"], 4)
        r["b_over_c"] = round(r["b_fused"]["slices_per_s"] / r["c_chain"]["slices_per_s"], 4)
        r["b_over_d"] = round(r["b_fused"]["slices_per_s"] / r["d_torch_chain"]["slices_per_s"], 4)
        res[f"bs{bs}"] = r
        del eng
        rt._ws_cache.clear()
        torch.cuda.empty_cache()
    # the two stand-alone regularisers at 64 x 4 x size x size
    N, C, S = 64, 4, a.size
    s = torch.softmax(torch.randn((N, C, S, S), device=dev) * 2, 1)
    img, ds, loss = torch.rand((N, 1, S, S), device=dev), torch.empty((N, C, S, S), device=dev), torch.zeros(3, device=dev)
    n = rt.L().wsl_loss_ws_bytes(N, C, S * S)
    ws = rt.workspace("loss", n)
    ms_cv, reg_cv = timed(lambda: rt.call("wsl_class_variance_fwd_bwd", rt.ptr(img), rt.ptr(s), rt.ptr(loss), rt.ptr(ds), 0.1, -0.1, N, C, S, S,
                                          rt.ptr(ws), n, rt.stream()), a.steps, a.warmup, torch)
    ms_ms, reg_ms = timed(lambda: rt.call("wsl_mumford_shah_fwd_bwd", rt.ptr(img), rt.ptr(s), rt.ptr(loss), rt.ptr(ds), 1e-6, N, C, S, S,
                                          rt.ptr(ws), n, rt.stream()), a.steps, a.warmup, torch)
    res["standalone_bs64"] = {"class_variance_us": round(ms_cv * 1e3, 2), "mumford_shah_us": round(ms_ms * 1e3, 2),
                              "class_variance_over_mumford_shah": round(ms_cv / ms_ms, 3),
                              "regions_us": {"class_variance": [round(v * 1e3, 2) for v in reg_cv], "mumford_shah": [round(v * 1e3, 2) for v in reg_ms]}}
    write(a.out, res)


def write(path, res):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def cmd_term(a):
    import torch
    from wsl4mis_amd.utils import losses
    dev = torch.device("cuda:0")
    p = torch.softmax(torch.randn((64, 4, a.size, a.size), device=dev) * 2, 1).requires_grad_()
    img = torch.rand((64, 1, a.size, a.size), device=dev)
    for _ in range(20):
        p.grad = None
        losses.class_variance_loss(p, img).backward()
    torch.cuda.synchronize()
    print("term: 20 forward + backward calls at 64 x 4 x %d x %d" % (a.size, a.size))


def cmd_merge(a):
    rows = []
    for f in glob.glob(os.path.join(a.stats, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    pick = {k: [r for r in rows if k in r["Name"]] for k in KERNELS}
    assert all(len(v) == 1 for v in pick.values()), {k: len(v) for k, v in pick.items()}
    px = 64 * a.size * a.size
    ns = {k: float(v[0]["AverageNs"]) for k, v in pick.items()}
    e = {"pixels": px, "calls": {k: int(v[0]["Calls"]) for k, v in pick.items()}, "kernel_us": {k: round(v / 1e3, 2) for k, v in ns.items()},
         "bytes_per_pixel": {"cv_moment_kernel": BYTES_MOMENT, "cv_grad_kernel": BYTES_GRAD},
         "hbm_fraction_of_8.0TBs": {"cv_moment_kernel": round(px * BYTES_MOMENT / (ns["cv_moment_kernel"] * 1e-9) / HBM_PEAK, 4),
                                    "cv_grad_kernel": round(px * BYTES_GRAD / (ns["cv_grad_kernel"] * 1e-9) / HBM_PEAK, 4)}}
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    res["kernels_bs64"] = e
    write(a.out, res)


def cmd_table(a):
    r = json.load(open(a.out))
    L = ["# Inter/intra-class variance training: what the regulariser costs (tools/bench_interintra.py)", "",
         "unet, %d x %d, f32; %d warm-up steps, three timed regions of %d steps per figure, the median region; one run on one MI355X.  "
         "Record: `%s`." % (r["size"], r["size"], r["warmup"], r["steps_per_region"], os.path.basename(a.out)), "",
         "| batch | a. `pce` slices/s | b. `pce_interintra` fused | c. `pce_interintra` chain | d. loss from torch ops | m. `pce_ms` | b / a | c / a | "
         "d / a | m / a | b / c | b / d |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for bs in (64, 12):
        b = r[f"bs{bs}"]
        L.append("| %d | %s | %s | %s | %s | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
            (bs,) + tuple("%.1f (%.2f ms)" % (b[k]["slices_per_s"], b[k]["ms_per_step"]) for k in ("a_pce", "b_fused", "c_chain", "d_torch_chain", "m_pce_ms"))
            + (b["b_fused_over_a"], b["c_chain_over_a"], b["d_torch_chain_over_a"], b["m_pce_ms_over_a"], b["b_over_c"], b["b_over_d"])))
    s = r["standalone_bs64"]
    L += ["", "The regulariser alone at 64 x 4 x %d x %d (device events around the entry point, value and gradient): "
          "`wsl_class_variance_fwd_bwd` %.1f us, `wsl_mumford_shah_fwd_bwd` %.1f us: ratio %.2f." % (
              r["size"], r["size"], s["class_variance_us"], s["mumford_shah_us"], s["class_variance_over_mumford_shah"])]
    e = r.get("kernels_bs64")
    if e:
        k, f = e["kernel_us"], e["hbm_fraction_of_8.0TBs"]
        L += ["", "The three kernels at bs 64 (`rocprofv3 --kernel-trace --stats`, a run of its own; the value-only forward call runs the "
              "first two, the backward call all three):", "",
              "| kernel | calls | mean us | algorithmic bytes per pixel | bytes / time, fraction of 8.0 TB/s |", "|---|---|---|---|---|",
              "| `cv_moment_kernel` | %d | %.2f | %.0f | %.3f |" % (e["calls"]["cv_moment_kernel"], k["cv_moment_kernel"], BYTES_MOMENT, f["cv_moment_kernel"]),
              "| `cv_coef_kernel` | %d | %.2f | | |" % (e["calls"]["cv_coef_kernel"], k["cv_coef_kernel"]),
              "| `cv_grad_kernel` | %d | %.2f | %.0f | %.3f |" % (e["calls"]["cv_grad_kernel"], k["cv_grad_kernel"], BYTES_GRAD, f["cv_grad_kernel"])]
    path = os.path.splitext(a.out)[0] + ".md"
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "term", "merge", "table"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50, help="steps per timed region (bench.py's default)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stats", default=None, help="merge: the profiler's output directory")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"run": cmd_run, "term": cmd_term, "merge": cmd_merge, "table": cmd_table}[a.cmd](a)


if __name__ == "__main__":
    main()
