"""Adversarial semi-supervised training on cuda:0: what the adversary costs (unet, 256 x 256, ndf 64), and its kernels one by one.
Sub-commands meant to be chained, each under its own time limit:

  timeout 600 python tools/bench_dan.py step --out profiles/dan_bench.json &&
  timeout 600 python tools/bench_dan.py kernels --out profiles/dan_bench.json &&
  python tools/bench_dan.py table --out profiles/dan_bench.json

step     at 6 + 6 (the reference's batch of 12, half labeled) and 32 + 32, slices/s of
           d. the `semi_dan` engine step          e. the `semi_entmin` engine step (the same two forwards, the cheapest head)
           t. the module-path loop of INTEGRATION 10c on this package's UNet with the adversary and Adam composed from stock torch ops
              (F.conv2d stride 2, F.leaky_relu, F.dropout2d, F.avg_pool2d, F.linear, torch.optim.Adam)
         The variants ALTERNATE in one process (region 1 of each, then region 2, then region 3); the figure is the median region and the
         spread (max - min) / median of a variant's three identical regions stands beside it.
kernels  at the three heavy layers (64 -> 128 at 128 x 128, 128 -> 256 at 64 x 64, 256 -> 512 at 32 x 32 input) and N = 12 and 64: time and
         algorithmic TFLOP/s (2 * N * Ho * Wo * Co * Ci * 16 per pass) of wsl_conv4s2_fwd / _dgrad / _wgrad (the weight gradient with its
         fixed-order reduction), as a fraction of the 157.3 TFLOP/s f32-MFMA peak, beside torch's time for the same convolution, its data
         gradient and its weight gradient (torch.ops.aten.convolution_backward with one output at a time).  Same alternating regions.
table    the record as markdown next to it (profiles/dan_bench.md)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 157.3e12
LAYERS = [(64, 128, 128), (128, 256, 64), (256, 512, 32)]      # Ci, Co, input size


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
    return {k: (statistics.median(v), [round(m, 4) for m in v], (max(v) - min(v)) / statistics.median(v)) for k, v in ms.items()}


def write(path, res):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def load(path):
    return json.load(open(path)) if path and os.path.exists(path) else {}


def torch_dan_step(model, opt, x_l, lab, x_u, w, ndf, torch):
    """the trainer's loop on the package's UNet, interleaved as INTEGRATION 10c has it; adversary, losses and Adam on stock torch ops"""
    import torch.nn as nn
    import torch.nn.functional as F
    convs = nn.ModuleList([nn.Conv2d(ci, co, 4, 2, 1) for ci, co in ((4, ndf), (1, ndf), (ndf, 2 * ndf), (2 * ndf, 4 * ndf), (4 * ndf, 8 * ndf))]).cuda()
    cls = nn.Linear(32 * ndf, 2).cuda()
    dopt = torch.optim.Adam(list(convs.parameters()) + list(cls.parameters()), lr=1e-4, betas=(0.9, 0.99))
    n_l, n_u = x_l.shape[0], x_u.shape[0]
    target = torch.tensor([1] * n_l + [0] * n_u, device=x_l.device)

    def dan(m, f, train):
        x = convs[0](m) + convs[1](f)
        x = F.dropout2d(F.leaky_relu(convs[2](x), 0.2), 0.5, train)
        x = F.dropout2d(F.leaky_relu(convs[3](x), 0.2), 0.5, train)
        x = F.avg_pool2d(F.leaky_relu(convs[4](x), 0.2), 7)
        return cls(x.reshape(x.shape[0], -1))

    def step():
        opt.zero_grad()
        model.train()
        z = model(x_l)
        s = torch.softmax(z, 1)
        dice = 0.0
        for c in range(4):
            t = (lab == c).float()
            dice = dice + (1 - (2 * torch.sum(s[:, c] * t) + 1e-5) / (torch.sum(s[:, c] * s[:, c]) + torch.sum(t * t) + 1e-5))
        (0.5 * (dice / 4 + F.cross_entropy(z, lab.long()))).backward()
        su = torch.softmax(model(x_u), 1)
        (w * F.cross_entropy(dan(su, x_u, False), target[:n_u])).backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            soft = torch.cat([torch.softmax(model(x_l), 1), torch.softmax(model(x_u), 1)], 0)
        model.train()
        dopt.zero_grad()
        F.cross_entropy(dan(soft, torch.cat([x_l, x_u], 0), True), target).backward()
        dopt.step()
    return step


def cmd_step(a):
    import torch
    from wsl4mis_amd import _lib
    from wsl4mis_amd import runtime as rt
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.networks.net_factory import net_factory
    from wsl4mis_amd.synthetic import batch
    assert torch.cuda.is_available(), "bench_dan needs cuda:0"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = load(a.out)
    res.update({"tool": "bench_dan", "net": "unet", "size": a.size, "ndf": a.ndf, "steps_per_region": a.steps, "warmup": a.warmup,
                "library_sha": _lib.library_sha256(), "tree_sha": _lib.source_sha256()})
    for half in (6, 32):
        x_l, _ = batch(half, a.size, a.size, 1, dev)
        x_u, _ = batch(half, a.size, a.size, 2, dev)
        lab = torch.randint(0, 4, (half, a.size, a.size), device=dev).to(torch.uint8)
        e_dan = TrainEngine("unet", 1, 4, loss="semi_dan", consistency_rampup=0, dan_ndf=a.ndf)
        e_ent = TrainEngine("unet", 1, 4, loss="semi_entmin", consistency_rampup=0)
        model = net_factory("unet", 1, 4)
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        variants = {"d_semi_dan": lambda: e_dan.step(x_l, lab, unlabeled=x_u), "e_semi_entmin": lambda: e_ent.step(x_l, lab, unlabeled=x_u),
                    "t_torch_adversary": torch_dan_step(model, opt, x_l, lab, x_u, 0.1, a.ndf, torch)}
        out = alternate(variants, a.steps, a.warmup, torch)
        k = {n: {"ms_per_step": round(ms, 3), "slices_per_s": round(2 * half / ms * 1e3, 1), "regions_ms": reg, "spread": round(sp, 4)}
             for n, (ms, reg, sp) in out.items()}
        k["d_semi_dan"]["losses"] = e_dan.losses()
        k["adversary_ms"] = round(k["d_semi_dan"]["ms_per_step"] - k["e_semi_entmin"]["ms_per_step"], 3)
        k["d_over_t"] = round(k["t_torch_adversary"]["ms_per_step"] / k["d_semi_dan"]["ms_per_step"], 4)
        res[f"bs{half}+{half}"] = k
        del e_dan, e_ent, model, opt, variants
        rt._ws_cache.clear()
        torch.cuda.empty_cache()
    write(a.out, res)


def cmd_kernels(a):
    import torch
    from wsl4mis_amd import runtime as rt
    assert torch.cuda.is_available(), "bench_dan needs cuda:0"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    aten = torch.ops.aten
    res = load(a.out)
    rows = []
    for N in (12, 64):
        for Ci, Co, S in LAYERS:
            x = torch.randn((N, Ci, S, S), device=dev)
            w = torch.randn((Co, Ci, 4, 4), device=dev) * 0.05
            b = torch.randn((Co,), device=dev)
            g = torch.randn((N, Co, S // 2, S // 2), device=dev)
            z = torch.randn((N, Co, S // 2, S // 2), device=dev)
            cm_in = (torch.rand((N, Ci), device=dev) > 0.5).float() * 2
            cm_out = (torch.rand((N, Co), device=dev) > 0.5).float() * 2
            y, dx, dw, db = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
            nb = rt.L().wsl_conv4s2_wgrad_ws_bytes(N, S, S, Ci, Co)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            st = rt.stream()
            bw = lambda mask: aten.convolution_backward(g, x, w, [Co], [2, 2], [1, 1], [1, 1], False, [0, 0], 1, mask)  # noqa: E731
            variants = {
                "fwd": lambda: rt.call("wsl_conv4s2_fwd", rt.ptr(x), Ci, None, 0, 1, rt.ptr(cm_in), rt.ptr(w), None, rt.ptr(b), None, rt.ptr(y), N, S, S, Co, st),
                "dgrad": lambda: rt.call("wsl_conv4s2_dgrad", rt.ptr(g), rt.ptr(z), rt.ptr(cm_out), rt.ptr(w), rt.ptr(dx), N, Ci, S, S, Co, st),
                "wgrad": lambda: rt.call("wsl_conv4s2_wgrad", rt.ptr(x), 1, rt.ptr(cm_in), rt.ptr(g), rt.ptr(z), rt.ptr(cm_out), rt.ptr(dw), rt.ptr(db),
                                         N, Ci, S, S, Co, rt.ptr(ws), nb, st),
                "torch_fwd": lambda: torch.nn.functional.conv2d(x, w, b, stride=2, padding=1),
                "torch_dgrad": lambda: bw([True, False, False]),
                "torch_wgrad": lambda: bw([False, True, True]),
            }
            out = alternate(variants, a.ksteps, a.warmup, torch)
            flops = 2.0 * N * (S // 2) ** 2 * Co * Ci * 16
            r = {"N": N, "Ci": Ci, "Co": Co, "size": S, "gflop": round(flops / 1e9, 2)}
            for k, (ms, reg, sp) in out.items():
                r[k] = {"ms": round(ms, 4), "spread": round(sp, 4), "tflops": round(flops / ms / 1e9, 2), "of_peak": round(flops / (ms * 1e-3) / PEAK, 4)}
            rows.append(r)
            del x, w, g, z, y, dx, dw, ws, variants
            torch.cuda.empty_cache()
    res["kernels"] = rows
    res["kernel_steps_per_region"] = a.ksteps
    write(a.out, res)


def cmd_table(a):
    r = json.load(open(a.out))
    L = ["# Adversarial semi-supervised training: what the adversary costs (tools/bench_dan.py)", ""]
    if any(k.startswith("bs") for k in r):
        L += ["unet, %d x %d, f32, FCDiscriminator ndf %d; %d warm-up steps per variant, then three timed regions of %d steps per variant, the "
              "variants alternating inside one process; the figure is the median region, `spread` = (max - min) / median of a variant's three "
              "identical regions; one run on one MI355X.  Record: `%s`." % (r["size"], r["size"], r["ndf"], r["warmup"], r["steps_per_region"],
                                                                          os.path.basename(a.out)), "",
              "| batch | d. `semi_dan` step | e. `semi_entmin` step | t. module-path loop, adversary + Adam on torch ops | d - e: the adversary | t / d |",
              "|---|---|---|---|---|---|"]
        for bs in [k for k in r if k.startswith("bs")]:
            b = r[bs]
            L.append("| %s | %s | %s | %s | %.2f ms | %.3f |" % (
                (bs[2:],) + tuple("%.1f slices/s (%.2f ms, spread %.3f)" % (b[k]["slices_per_s"], b[k]["ms_per_step"], b[k]["spread"])
                                  for k in ("d_semi_dan", "e_semi_entmin", "t_torch_adversary")) + (b["adversary_ms"], b["d_over_t"])))
        L += ["", "(t / d: the torch-composed loop's time over the engine step's; above 1 the engine is faster.)"]
    if "kernels" in r:
        L += ["", "The 4x4 stride-2 kernels at the three heavy layers (HIP events around %d calls per region, three alternating regions, median; "
              "TFLOP/s algorithmic, fraction of the 157.3 TFLOP/s f32-MFMA peak; the weight gradient includes its reduction; torch = "
              "F.conv2d / aten.convolution_backward on the same tensors, without the loader's activation and masks):" % r["kernel_steps_per_region"], "",
              "| N | layer | GFLOP | forward | data gradient | weight gradient | torch fwd | torch dgrad | torch wgrad |", "|---|---|---|---|---|---|---|---|---|"]
        lost = []
        for k in r["kernels"]:
            ours = tuple("%.3f ms, %.1f TF (%.1f %%), spread %.3f" % (k[n]["ms"], k[n]["tflops"], 100 * k[n]["of_peak"], k[n]["spread"]) for n in ("fwd", "dgrad", "wgrad"))
            th = tuple("%.3f ms (%.1f TF)" % (k[n]["ms"], k[n]["tflops"]) for n in ("torch_fwd", "torch_dgrad", "torch_wgrad"))
            L.append("| %d | %d -> %d at %d x %d | %.1f | %s | %s | %s | %s | %s | %s |" % ((k["N"], k["Ci"], k["Co"], k["size"], k["size"], k["gflop"]) + ours + th))
            lost += ["%s N=%d %d->%d (%.2fx torch's time)" % (n, k["N"], k["Ci"], k["Co"], k[n]["ms"] / k["torch_" + n]["ms"])
                     for n in ("fwd", "dgrad", "wgrad") if k[n]["ms"] > k["torch_" + n]["ms"]]
        L += ["", "Slower than torch's kernel for the same convolution: " + ("none." if not lost else "; ".join(lost) + ".") +
              "  A finding, not a route: the product has no path through torch's convolutions."]
    path = os.path.splitext(a.out)[0] + ".md"
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["step", "kernels", "table"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ndf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed region (step)")
    ap.add_argument("--ksteps", type=int, default=20, help="calls per timed region (kernels)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"step": cmd_step, "kernels": cmd_kernels, "table": cmd_table}[a.cmd](a)


if __name__ == "__main__":
    main()
