"""Random-walker pseudo labels on cuda:0: what `random_walker.precompute` costs for an ACDC fold, beside the direct solve the reference
pays per read.  Sub-commands, meant to be chained, each under its own time limit, the profiler in a run of its own:

  timeout 600 python tools/bench_rw.py run --out profiles/rw_bench.json &&
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o rw -- python tools/bench_rw.py solve &&
  python tools/bench_rw.py merge --stats <dir> --out profiles/rw_bench.json &&
  python tools/bench_rw.py table --out profiles/rw_bench.json

run    a. `precompute` over 1512 slices (an ACDC fold's training set): the committed volume's five full-class slices (224 x 154), tiled.
          One warm-up pass, then three timed passes on fresh caches, host clock (the pass ends in device-to-host copies); the median.
       b. the solver calls of such a pass alone (device events), and the iteration counts of all 6048 systems
       c. on the host of the same machine, in the same run: the fp64 scipy `splu` solve of the same systems (tests/rw_ref.py) on a
          subset of the slices, EXTRAPOLATED to 1512 (the slices repeat, so the mean per slice carries over)
solve  one batched solver call of 380 slices, 3 times (what the profiler run traces)
merge  the share of kernel time in setup (statistics + weights), solve and finish, from the profiler's kernel statistics
table  the record as markdown next to it (profiles/rw_bench.md)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FOLD_SLICES = 1512


class TiledSlices:
    """what random_walker.precompute uses of a BaseDataSets, over the five full-class slices of the committed volume repeated to n"""

    def __init__(self, n):
        import rw_ref
        img, scr = rw_ref.volume()
        self.base = [(img[z].copy(), scr[z].astype("uint16")) for z in range(1, 6)]
        self.sample_list = ["tile%04d_slice_%d.h5" % (i, 1 + i % 5) for i in range(n)]
        self._rw_cache = {}

    def _rw_inputs(self, case):
        return self.base[int(case[-4]) - 1]


def write(path, res):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def cmd_run(a):
    import numpy as np
    import torch
    import rw_ref
    from wsl4mis_amd import _lib
    from wsl4mis_amd.dataloaders import random_walker as rw
    assert torch.cuda.is_available(), "bench_rw needs cuda:0"
    res = {"tool": "bench_rw", "slices": a.slices, "shape": [224, 154], "n_class": 4, "tol": 1e-5, "max_iter": 10000,
           "library_sha": _lib.library_sha256(), "tree_sha": _lib.source_sha256()}
    # a. precompute, end to end
    rw.precompute(TiledSlices(a.slices))                                      # warm-up: code objects, workspace, allocator
    torch.cuda.synchronize()
    secs, info = [], None
    for _ in range(3):
        ds = TiledSlices(a.slices)
        t0 = time.perf_counter()
        info = rw.precompute(ds)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    it = np.asarray(info["iterations"])
    res["a_precompute"] = {"seconds": round(statistics.median(secs), 4), "passes_s": [round(s, 4) for s in secs],
                           "slices_per_s": round(a.slices / statistics.median(secs), 1), "zeroed_by_class_rule": info["zeroed_by_class_rule"]}
    res["iterations"] = {"systems": int(it.size), "min": int(it.min()), "median": float(np.median(it)), "max": int(it.max())}
    # b. the solver calls alone
    ds = TiledSlices(a.slices)
    img = np.stack([ds._rw_inputs(c)[0] for c in ds.sample_list])
    sd = np.stack([ds._rw_inputs(c)[1] for c in ds.sample_list]).astype(np.uint8)
    per = max(1, int(rw.MAX_BATCH_BYTES // _lib.lib().wsl_random_walker_ws_bytes(1, 224, 154, 4)))
    chunks = [(torch.from_numpy(img[b:b + per]).cuda(), torch.from_numpy(sd[b:b + per]).cuda()) for b in range(0, a.slices, per)]
    ms = []
    for rep in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for ci, cs in chunks:
            rw._solve(ci, cs, 4, 100.0, 1e-5, 10000, False)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    res["b_solver_calls"] = {"ms": round(statistics.median(ms), 2), "passes_ms": [round(m, 2) for m in ms], "calls": len(chunks),
                             "slices_per_call": per}
    # c. the direct solve on this machine's host
    t = []
    for i in range(a.cpu_slices):
        im, sc = ds._rw_inputs(ds.sample_list[i])
        t0 = time.perf_counter()
        rw_ref.solve(im, sc.astype(np.uint8), 4)
        t.append(time.perf_counter() - t0)
    per_slice = statistics.mean(t[5:]) if len(t) > 10 else statistics.mean(t)          # (the first round over the five slices: warm-up)
    res["c_scipy_splu_fp64_host"] = {"slices_measured": len(t), "s_per_slice": round(per_slice, 4),
                                     "EXTRAPOLATED_seconds_for_%d_slices" % a.slices: round(per_slice * a.slices, 1),
                                     "note": "assembly + splu + 4 right-hand sides per slice, one thread"}
    res["ratio_cpu_extrapolated_over_precompute"] = round(per_slice * a.slices / res["a_precompute"]["seconds"], 1)
    write(a.out, res)


def cmd_solve(a):
    import numpy as np
    import torch
    from wsl4mis_amd.dataloaders import random_walker as rw
    ds = TiledSlices(380)
    img = torch.from_numpy(np.stack([ds._rw_inputs(c)[0] for c in ds.sample_list])).cuda()
    sd = torch.from_numpy(np.stack([ds._rw_inputs(c)[1] for c in ds.sample_list]).astype(np.uint8)).cuda()
    for _ in range(3):
        rw._solve(img, sd, 4, 100.0, 1e-5, 10000, False)
    torch.cuda.synchronize()
    print("solve: 3 calls of 380 x 224 x 154, 4 classes")


def cmd_merge(a):
    rows = []
    for f in glob.glob(os.path.join(a.stats, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    ns = {k: sum(float(r["TotalDurationNs"]) for r in rows if k in r["Name"]) for k in ("rw_stats_kernel", "rw_setup_kernel", "rw_pcg_kernel",
                                                                                       "rw_finish_kernel")}
    assert all(v > 0 for v in ns.values()), ns
    tot = sum(ns.values())
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    res["d_kernel_shares"] = {"calls": 3, "slices_per_call": 380, "kernel_ms_per_call": {k: round(v / 3e6, 3) for k, v in ns.items()},
                              "share": {"setup": round((ns["rw_stats_kernel"] + ns["rw_setup_kernel"]) / tot, 4),
                                        "solve": round(ns["rw_pcg_kernel"] / tot, 4), "finish": round(ns["rw_finish_kernel"] / tot, 4)}}
    write(a.out, res)


def cmd_table(a):
    r = json.load(open(a.out))
    p, b, c, it = r["a_precompute"], r["b_solver_calls"], r["c_scipy_splu_fp64_host"], r["iterations"]
    ext = c["EXTRAPOLATED_seconds_for_%d_slices" % r["slices"]]
    L = ["# Random-walker pseudo labels: `precompute` for an ACDC fold (tools/bench_rw.py)", "",
         "%d slices of %d x %d (the committed volume's five full-class slices, tiled), %d classes, tol %.0e; one warm-up pass, three timed "
         "passes, the median; one run on one MI355X and its host.  Record: `%s`." % (r["slices"], r["shape"][0], r["shape"][1], r["n_class"],
                                                                                  r["tol"], os.path.basename(a.out)), "",
         "| | seconds | slices/s |", "|---|---|---|",
         "| a. `precompute`, end to end (stacking, copies, %d solver calls, labels back on the host) | %.3f | %.0f |" % (
             b["calls"], p["seconds"], p["slices_per_s"]),
         "| b. the solver calls alone (device events) | %.3f | %.0f |" % (b["ms"] / 1e3, r["slices"] / (b["ms"] / 1e3)),
         "| c. fp64 scipy `splu` on the host, %d slices measured, **extrapolated** to %d | %.1f | %.2f |" % (
             c["slices_measured"], r["slices"], ext, 1.0 / c["s_per_slice"]), "",
         "Ratio c / a: **%.0f x** (c is extrapolated from %.3f s per slice)." % (r["ratio_cpu_extrapolated_over_precompute"], c["s_per_slice"]), "",
         "Iterations of the %d systems: min %d, median %.0f, max %d." % (it["systems"], it["min"], it["median"], it["max"])]
    d = r.get("d_kernel_shares")
    if d:
        k, s = d["kernel_ms_per_call"], d["share"]
        L += ["", "Kernel time of one call of %d slices (`rocprofv3 --kernel-trace --stats`, a run of its own, %d calls):" % (
            d["slices_per_call"], d["calls"]), "", "| phase | kernels | ms per call | share |", "|---|---|---|---|",
              "| setup | `rw_stats_kernel`, `rw_setup_kernel` | %.3f | %.1f %% |" % (k["rw_stats_kernel"] + k["rw_setup_kernel"], 100 * s["setup"]),
              "| solve | `rw_pcg_kernel` | %.3f | %.1f %% |" % (k["rw_pcg_kernel"], 100 * s["solve"]),
              "| finish | `rw_finish_kernel` | %.3f | %.1f %% |" % (k["rw_finish_kernel"], 100 * s["finish"])]
    path = os.path.splitext(a.out)[0] + ".md"
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "solve", "merge", "table"])
    ap.add_argument("--slices", type=int, default=FOLD_SLICES)
    ap.add_argument("--cpu_slices", type=int, default=25, help="slices of the host's direct solve (at least 20)")
    ap.add_argument("--stats", default=None, help="merge: the profiler's output directory")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"run": cmd_run, "solve": cmd_solve, "merge": cmd_merge, "table": cmd_table}[a.cmd](a)


if __name__ == "__main__":
    main()
