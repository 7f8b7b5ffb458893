"""The engine's contract, pinned: a step is "a fixed sequence of C-ABI calls" (wsl4mis_amd/engine.py).  Every composition's first two
steps are recorded call by call -- entry-point name and every argument -- WITHOUT running a kernel, and compared with
tests/golden/engine_call_trace.json.  A change to engine.py that leaves these sequences as they are cannot change a result or the device
time of a step; one that reorders, drops, adds or re-parametrises a call fails here in milliseconds, before any numerical test runs.

What a recorded argument looks like: None stays None; floats and small ints verbatim; a ctypes.c_uint64 (a drawn seed) is "seed"; any
other ctypes object is its type name; an address is "p<k>", k the order in which it first appeared within the step.  The streams, the
collectives and the device copies between loss slots are not runtime.call()s: the numerical engine tests keep those.

A new composition regenerates the fixture ON PURPOSE:  WSL_REGEN_CALL_TRACE=1 pytest tests/test_engine_call_trace.py"""
import ctypes
import json
import os
import random

import pytest
import torch

from conftest import GOLDEN, get_backend

FIXTURE = os.path.join(GOLDEN, "engine_call_trace.json")
REGEN = os.environ.get("WSL_REGEN_CALL_TRACE") == "1"
N, N_U, S, CLASSES = 2, 3, 32, 4
BOTH_ROUTES = ("pce_tv", "pce_ms", "pce_entropy", "ce_dice", "mean_teacher", "pce_interintra", "semi_mt", "semi_uamt", "semi_entmin",
               "semi_dan")


def _cases():
    """(id, net, loss, fused_heads or None = the engine's default, constructor extras, data-parallel route)"""
    c = [(f"unet_cct-{k}", "unet_cct", k, None, {}, False) for k in ("ours_proposed", "pce", "pce_gatedcrf")]
    c += [(f"unet-{k}", "unet", k, None, {}, False) for k in ("pce", "pce_gatedcrf", "ustm")]
    c += [(f"{net}-s2l", net, "s2l", None, {"thr_iter": 1}, False) for net in ("unet", "pnet")]      # step 1: plain head, step 2: the s2l head
    for fused in (True, False):
        route = "fused" if fused else "chain"
        c += [(f"unet-{k}-{route}", "unet", k, fused, {}, False) for k in BOTH_ROUTES]
        c += [(f"pnet-{k}-{route}", "pnet", k, fused, {}, False) for k in ("pce_interintra", "semi_entmin")]
    c.append(("unet-semi_mt-frozen", "unet", "semi_mt", None, {"teacher_update": "frozen"}, False))
    c += [("dp-unet_cct-pce_gatedcrf", "unet_cct", "pce_gatedcrf", None, {}, True), ("dp-unet-semi_mt", "unet", "semi_mt", None, {}, True)]
    return c


CASES = _cases()


class _Addr(int):
    """what the patched runtime.ptr returns: an address stays recognisable wherever the allocator placed it"""


class Recorder:
    def __init__(self, real_call):
        self.real_call, self.calls, self.held, self.names = real_call, [], [], {}

    def ptr(self, t):
        if t is None:
            return None
        self.held.append(t)          # alive until the step ends: a freed temporary's address would be handed out again
        return _Addr(t.data_ptr())

    def _arg(self, a):
        if a is None or isinstance(a, (float, str)):
            return a
        if isinstance(a, ctypes.c_uint64):
            return "seed"
        if isinstance(a, int):
            if isinstance(a, _Addr) or a > 2 ** 32:
                return self.names.setdefault(int(a), f"p{len(self.names)}")
            return int(a)
        return type(a).__name__

    def call(self, name, *args):
        if name.endswith("_entry"):                       # module construction enumerates its state through these
            return self.real_call(name, *args)
        self.calls.append([name] + [self._arg(a) for a in args])

    def take_step(self):
        calls, self.calls, self.held, self.names = self.calls, [], [], {}
        return calls


@pytest.fixture
def recorder(monkeypatch):
    from wsl4mis_amd import _lib, runtime
    _lib._reset_for_tests()
    _lib.use_library_for_tests(get_backend("emul").lib)
    rec = Recorder(runtime.call)
    monkeypatch.setattr(runtime, "call", rec.call)
    monkeypatch.setattr(runtime, "ptr", rec.ptr)
    yield rec
    _lib._reset_for_tests()
    runtime._ws_cache.clear()


def record(rec, net, loss, fused, extra, dp):
    """the calls of two consecutive step()s: it == 0 (wsl_sgd_step's `first`, alpha 0, the base learning rate), then it == 1"""
    import torch.distributed as dist
    from wsl4mis_amd import runtime
    from wsl4mis_amd.engine import TrainEngine
    runtime._ws_cache.clear()      # the grow-only workspaces: their byte counts would otherwise depend on the cases that ran before
    torch.manual_seed(0)
    random.seed(0)                 # 'ustm' draws its rotation from python's generator
    if dp:
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        eng = TrainEngine(net, 1, CLASSES, loss=loss, dan_ndf=8, dan_pool=1, force_dp=dp, **extra)
        assert eng.dp == dp
        if fused is not None:
            eng.fused_heads = fused
        x, lab = torch.rand(N, 1, S, S), torch.randint(0, CLASSES + 1, (N, S, S), dtype=torch.uint8)
        kw = {}
        if loss in TrainEngine.SEMI:
            kw["unlabeled"] = torch.rand(N_U, 1, S, S)
        if loss == "s2l":
            kw["weight"] = torch.rand(N, S, S, CLASSES)
        rec.take_step()
        steps = []
        for _ in range(2):
            eng.step(x, lab, **kw)
            steps.append(rec.take_step())
        assert eng.it == 2
        return steps
    finally:
        if dp:
            dist.destroy_process_group()


def _dump(traces):
    """one call per line: a regenerated fixture then diffs call by call"""
    out = ["{"]
    for ci, (cid, steps) in enumerate(traces.items()):
        out.append(f" {json.dumps(cid)}: [")
        for si, calls in enumerate(steps):
            out.append("  [")
            out += ["   " + json.dumps(c) + ("," if i + 1 < len(calls) else "") for i, c in enumerate(calls)]
            out.append("  ]" + ("," if si + 1 < len(steps) else ""))
        out.append(" ]" + ("," if ci + 1 < len(traces) else ""))
    out.append("}")
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def golden_traces():
    if REGEN:                      # the cases fill an empty mapping, written out when the module is done
        traces = {}
        yield traces
        with open(FIXTURE, "w") as fh:
            fh.write(_dump({c[0]: traces[c[0]] for c in CASES}))
        return
    with open(FIXTURE) as fh:
        yield json.load(fh)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_step_is_the_recorded_call_sequence(recorder, golden_traces, case):
    got = json.loads(json.dumps(record(recorder, *case[1:])))      # through JSON, as the fixture went
    if REGEN:
        golden_traces[case[0]] = got
        return
    want = golden_traces[case[0]]
    for s, (g, w) in enumerate(zip(got, want)):
        for i, (cg, cw) in enumerate(zip(g, w)):
            assert cg == cw, f"{case[0]}, step {s + 1}, call {i}:\n  recorded {cw}\n  now      {cg}"
        assert len(g) == len(w), f"{case[0]}, step {s + 1}: {len(g)} calls, recorded {len(w)}; first surplus / missing call: " \
                                 f"{max(g, w, key=len)[min(len(g), len(w))]}"
    assert got == want


def test_fixture_holds_exactly_the_cases(golden_traces):
    assert sorted(golden_traces) == sorted(c[0] for c in CASES)
