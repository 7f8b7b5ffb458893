"""Semi-supervised training on cuda:0: what the two-forward step costs (unet, 256 x 256).  Sub-commands meant to be chained, each under
its own time limit, the profiler in a run of its own (the method of tools/bench_interintra.py):

  timeout 900 python tools/bench_semi.py run --out profiles/semi_bench.json &&
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o semi -- python tools/bench_semi.py term &&
  python tools/bench_semi.py merge --stats <dir> --out profiles/semi_bench.json &&
  python tools/bench_semi.py table --out profiles/semi_bench.json

run    at bs 32 + 32 and 6 + 6 (the reference's batch of 12, half labeled), for each of semi_mt / semi_uamt / semi_entmin, slices/s of
         f. the engine step, fused heads      c. the engine step, chains of calls (fused_heads = False)
         t. the interleaved module-path loop of INTEGRATION 10b with the losses composed from stock torch GPU ops and torch's SGD
       The variants ALTERNATE in one process: region 1 of f, c, t, then region 2 of each, then region 3; the figure is the median region and
       the spread (max - min) / median of a variant's three identical regions stands beside it.  For scale: the `ce_dice` step at N = 32 and
       the `mean_teacher` step at N = 64.
term   the two new heads alone, 20 calls each at 32 x 4 x 256 x 256 (what the profiler run traces)
merge  their kernels' times from the profiler's kernel statistics, with the bytes per pixel the algorithm moves (from the shapes) over
       the kernel time as a fraction of the HBM peak
table  the record as a markdown table next to it (profiles/semi_bench.md)
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
KINDS = ("semi_mt", "semi_uamt", "semi_entmin")
# 4 classes, per pixel: the supervised head's reduction reads 16 B of logits + 1 B of label, its gradient pass reads them again and writes
# 16 B; the entropy head reads 16 B and writes 16 B
BYTES = {"sup_reduce_kernel": 17.0, "sup_bwd_kernel": 33.0, "ent_logits_kernel": 32.0}
KERNELS = ("sup_reduce_kernel", "sup_finalize_kernel", "sup_bwd_kernel", "ent_logits_kernel", "ent_finalize_kernel")


def region(fn, steps, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(variants, steps, warmup, torch):
    """{name: fn} -> {name: (median ms, [three regions], spread)}: warm every variant up, then time region r of each before region r + 1"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ms[k].append(region(fn, steps, torch))
    return {k: (statistics.median(v), [round(m, 3) for m in v], (max(v) - min(v)) / statistics.median(v)) for k, v in ms.items()}


def torch_step(kind, model, teacher, opt, x_l, lab, x_u, w, thr, torch):
    """the trainers' loop on the package's modules, interleaved as INTEGRATION 10b has it, every loss line a stock torch op"""
    import torch.nn.functional as F

    def noisy(x):
        return x + torch.clamp(torch.randn_like(x) * 0.1, -0.2, 0.2)

    def step():
        opt.zero_grad()
        z = model(x_l)
        s = torch.softmax(z, 1)
        dice = 0.0
        for c in range(4):
            t = (lab == c).float()
            dice = dice + (1 - (2 * torch.sum(s[:, c] * t) + 1e-5) / (torch.sum(s[:, c] * s[:, c]) + torch.sum(t * t) + 1e-5))
        (0.5 * (dice / 4 + F.cross_entropy(z, lab.long()))).backward()
        if kind != "semi_entmin":
            with torch.no_grad():
                st = torch.softmax(teacher(noisy(x_u)), 1)
                if kind == "semi_uamt":
                    xr = x_u.repeat(2, 1, 1, 1)
                    p = torch.cat([torch.softmax(teacher(noisy(xr)), 1) for _ in range(4)], 0)
                    p = p.reshape(8, x_u.shape[0], 4, x_u.shape[2], x_u.shape[3]).mean(0)
                    mask = (-1.0 * torch.sum(p * torch.log(p + 1e-6), dim=1, keepdim=True) < thr).float()
        su = torch.softmax(model(x_u), 1)
        if kind == "semi_mt":
            cons = torch.mean((su - st) ** 2)
        elif kind == "semi_uamt":
            cons = torch.sum(mask * (su - st) ** 2) / (2 * torch.sum(mask) + 1e-16)
        else:
            cons = torch.mean(-1 * torch.sum(su * torch.log(su + 1e-6), dim=1) / math.log(4))
        (w * cons).backward()
        opt.step()
        if teacher is not None:
            with torch.no_grad():
                for e, p_ in zip(teacher.parameters(), model.parameters()):
                    e.mul_(0.99).add_(p_, alpha=0.01)
    return step


def cmd_run(a):
    import torch
    from wsl4mis_amd import _lib
    from wsl4mis_amd import runtime as rt
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.networks.net_factory import net_factory
    from wsl4mis_amd.synthetic import batch
    assert torch.cuda.is_available(), "bench_semi needs cuda:0"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"tool": "bench_semi", "net": "unet", "size": a.size, "steps_per_region": a.steps, "warmup": a.warmup,
           "library_sha": _lib.library_sha256(), "tree_sha": _lib.source_sha256()}
    for half in (32, 6):
        x_l, _ = batch(half, a.size, a.size, 1, dev)
        x_u, _ = batch(half, a.size, a.size, 2, dev)
        lab = torch.randint(0, 4, (half, a.size, a.size), device=dev).to(torch.uint8)
        r = {}
        for kind in KINDS:
            engs = {}
            for name, fused in (("f_fused", True), ("c_chain", False)):
                e = TrainEngine("unet", 1, 4, loss=kind, consistency_rampup=0)
                e.fused_heads = fused
                engs[name] = e
            model = net_factory("unet", 1, 4)
            model.train()
            teacher = None
            if kind != "semi_entmin":
                teacher = net_factory("unet", 1, 4)
                teacher.load_state_dict(model.state_dict())
                teacher.train()
            opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
            variants = {"f_fused": lambda e=engs["f_fused"]: e.step(x_l, lab, unlabeled=x_u),
                        "c_chain": lambda e=engs["c_chain"]: e.step(x_l, lab, unlabeled=x_u),
                        "t_torch_loop": torch_step(kind, model, teacher, opt, x_l, lab, x_u, 0.1, 0.75 * math.log(2.0), torch)}
            out = alternate(variants, a.steps, a.warmup, torch)
            k = {n: {"ms_per_step": round(ms, 3), "slices_per_s": round(2 * half / ms * 1e3, 1), "regions_ms": reg, "spread": round(sp, 4)}
                 for n, (ms, reg, sp) in out.items()}
            k["f_fused"]["losses"] = engs["f_fused"].losses()
            k["f_over_c"] = round(k["c_chain"]["ms_per_step"] / k["f_fused"]["ms_per_step"], 4)
            k["f_over_t"] = round(k["t_torch_loop"]["ms_per_step"] / k["f_fused"]["ms_per_step"], 4)
            k["max_spread"] = max(v["spread"] for v in k.values() if isinstance(v, dict) and "spread" in v)
            r[kind] = k
            del engs, model, teacher, opt, variants
            rt._ws_cache.clear()
            torch.cuda.empty_cache()
        res[f"bs{half}+{half}"] = r
    # for scale: the dense-label step on one half, and the single-forward mean teacher on a whole batch
    x32, _ = batch(32, a.size, a.size, 1, dev)
    lab32 = torch.randint(0, 4, (32, a.size, a.size), device=dev).to(torch.uint8)
    x64, lab64 = batch(64, a.size, a.size, 3, dev)
    e1, e2 = TrainEngine("unet", 1, 4, loss="ce_dice"), TrainEngine("unet", 1, 4, loss="mean_teacher")
    out = alternate({"ce_dice_n32": lambda: e1.step(x32, lab32), "mean_teacher_n64": lambda: e2.step(x64, lab64)}, a.steps, a.warmup, torch)
    res["scale"] = {n: {"ms_per_step": round(ms, 3), "regions_ms": reg, "spread": round(sp, 4)} for n, (ms, reg, sp) in out.items()}
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
    from wsl4mis_amd import runtime as rt
    dev = torch.device("cuda:0")
    N, C, S = 32, 4, a.size
    z = torch.randn((N, C, S, S), device=dev) * 2
    lab = torch.randint(0, 4, (N, S, S), device=dev).to(torch.uint8)
    dz, out = torch.empty_like(z), torch.zeros(8, device=dev)
    n = rt.L().wsl_loss_ws_bytes(N, C, S * S)
    ws = rt.workspace("loss", n)
    for _ in range(20):
        rt.call("wsl_sup_head_fwd_bwd", rt.ptr(z), rt.ptr(lab), 4, 0.5, 0.5, 1.0, rt.ptr(out), rt.ptr(dz), N, C, S * S, rt.ptr(ws), n, rt.stream())
        rt.call("wsl_entropy_logits_fwd_bwd", rt.ptr(z), rt.ptr(out[4:]), rt.ptr(dz), 0.1, N, C, S * S, 4, rt.ptr(ws), n, rt.stream())
    torch.cuda.synchronize()
    print("term: 20 calls of each head at %d x %d x %d x %d" % (N, C, S, S))


def cmd_merge(a):
    rows = []
    for f in glob.glob(os.path.join(a.stats, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    pick = {k: [r for r in rows if k in r["Name"]] for k in KERNELS}
    assert all(len(v) == 1 for v in pick.values()), {k: len(v) for k, v in pick.items()}
    px = 32 * a.size * a.size
    ns = {k: float(v[0]["AverageNs"]) for k, v in pick.items()}
    e = {"pixels": px, "calls": {k: int(v[0]["Calls"]) for k, v in pick.items()}, "kernel_us": {k: round(v / 1e3, 2) for k, v in ns.items()},
         "bytes_per_pixel": BYTES, "hbm_fraction_of_8.0TBs": {k: round(px * b / (ns[k] * 1e-9) / HBM_PEAK, 4) for k, b in BYTES.items()}}
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    res["kernels_n32"] = e
    write(a.out, res)


def cmd_table(a):
    r = json.load(open(a.out))
    L = ["# Semi-supervised training: what the two-forward step costs (tools/bench_semi.py)", "",
         "unet, %d x %d, f32; %d warm-up steps per variant, then three timed regions of %d steps per variant, the variants alternating inside "
         "one process; the figure is the median region, `spread` = (max - min) / median of a variant's three identical regions; one run on one "
         "MI355X.  Record: `%s`." % (r["size"], r["size"], r["warmup"], r["steps_per_region"], os.path.basename(a.out)), "",
         "| batch | loss | f. fused step | c. chain step | t. module-path loop, torch losses | f / c | f / t | largest spread |", "|---|---|---|---|---|---|---|---|"]
    for bs in [k for k in r if k.startswith("bs")]:
        for kind in KINDS:
            b = r[bs][kind]
            L.append("| %s | `%s` | %s | %s | %s | %.3f | %.3f | %.3f |" % (
                (bs[2:], kind) + tuple("%.1f slices/s (%.2f ms, spread %.3f)" % (b[k]["slices_per_s"], b[k]["ms_per_step"], b[k]["spread"])
                                       for k in ("f_fused", "c_chain", "t_torch_loop")) + (b["f_over_c"], b["f_over_t"], b["max_spread"])))
    s = r["scale"]
    L += ["", "(f / c, f / t: rates, i.e. the other variant's time over the fused step's.)  For scale: the `ce_dice` step at N = 32 takes %.2f ms "
          "(spread %.3f), the single-forward `mean_teacher` step at N = 64 %.2f ms (spread %.3f)." % (
              s["ce_dice_n32"]["ms_per_step"], s["ce_dice_n32"]["spread"], s["mean_teacher_n64"]["ms_per_step"], s["mean_teacher_n64"]["spread"])]
    slower = [(bs, k) for bs in r if bs.startswith("bs") for k in KINDS
              if r[bs][k]["f_over_c"] < 1.0 - max(r[bs][k]["f_fused"]["spread"], r[bs][k]["c_chain"]["spread"])]
    L += ["", "Condition for keeping the fused heads the default -- the fused step is not slower than the chain step by more than the measured "
          "spread: " + ("MET in every row." if not slower else "NOT met in " + ", ".join(f"{b} {k}" for b, k in slower) + ".")]
    e = r.get("kernels_n32")
    if e:
        L += ["", "The new kernels at 32 x 4 x %d x %d (`rocprofv3 --kernel-trace --stats`, a run of its own):" % (r["size"], r["size"]), "",
              "| kernel | calls | mean us | algorithmic bytes per pixel | bytes / time, fraction of 8.0 TB/s |", "|---|---|---|---|---|"]
        for k in KERNELS:
            L.append("| `%s` | %d | %.2f | %s | %s |" % (k, e["calls"][k], e["kernel_us"][k], ("%.0f" % BYTES[k]) if k in BYTES else "",
                                                      ("%.3f" % e["hbm_fraction_of_8.0TBs"][k]) if k in BYTES else ""))
    path = os.path.splitext(a.out)[0] + ".md"
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "term", "merge", "table"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed region")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--stats", default=None, help="merge: the profiler's output directory")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"run": cmd_run, "term": cmd_term, "merge": cmd_merge, "table": cmd_table}[a.cmd](a)


if __name__ == "__main__":
    main()
