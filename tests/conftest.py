import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


class _Fixture(dict):
    """the arrays of a fixture stored in parts, as one mapping with NpzFile's `files`"""

    @property
    def files(self):
        return list(self)


def golden(name):
    """name.npz; a fixture that tests/golden/make_golden.py::save() split to keep every file under 1 MiB also has
    name.part2.npz, ... (disjoint keys), read back as one mapping"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    parts = sorted(f for f in os.listdir(GOLDEN) if f.startswith(name + ".part") and f.endswith(".npz"))
    if not parts:
        return g
    out = _Fixture((k, g[k]) for k in g.files)
    for f in parts:
        with np.load(os.path.join(GOLDEN, f), allow_pickle=False) as p:
            out.update((k, p[k]) for k in p.files)
    return out


def rel_err(a, b, floor=1e-6):
    """max |a-b| / (max|b| + floor): the 1e-4 'relative fp32' criterion of BASELINE.json, taken
    against the tensor's scale (per-element relative error is meaningless near zero crossings)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + floor)) if a.size else 0.0


def mixed_err(a, b, tol=1e-4):
    """Second criterion beside rel_err: every element must satisfy
        |a - b| <= tol * |b| + tol * rms(b)
    i.e. element-wise relative error with an absolute floor at the tensor's RMS instead of its maximum, so an entry
    1000x below the maximum may not be 10 % off.  Returns max over elements of |a-b| / (tol*|b| + tol*rms(b)); pass = <= 1."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    if not a.size:
        return 0.0
    rms = float(np.sqrt(np.mean(b * b)))
    return float(np.max(np.abs(a - b) / (tol * np.abs(b) + tol * rms + 1e-30)))


def close(a, b, tol=1e-4):
    """both parity criteria: tensor-scale (rel_err) and element-wise with an RMS floor (mixed_err)"""
    return rel_err(a, b) < tol and mixed_err(a, b, tol) <= 1.0


_RATES = []
_SUMMARY = []


def summary_line(text):
    """A measured margin that should reach the terminal even under `pytest -q` (the driver's record keeps the tail of the
    output): printed by pytest_terminal_summary below."""
    _SUMMARY.append(str(text))


def pytest_terminal_summary(terminalreporter, exitstatus, config):
    if _RATES or _SUMMARY:
        terminalreporter.write_sep("-", "measured margins (label-map mismatches in pixels; error budgets)")
        for r in _RATES:
            terminalreporter.write_line(f"LABELMAP {r['test']}: {r['mismatched_px']} of {r['pixels']} px differ (allowed {r['allowed_px']})")
        for t in _SUMMARY:
            terminalreporter.write_line(t)


def labelmap_mismatch(name, got, ref, allow_px):
    """Label maps are bit-exact at op level (mix+argmax given identical inputs); end to end the softmax / conv rounding can
    flip a pixel whose two best classes tie to the last ulp.  The measured count is printed (pytest -s / -rP shows it) and
    appended to gpurun_out/labelmap_rates.jsonl on the GPU box; `allow_px` is the allowance in PIXELS."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = int(np.count_nonzero(got != ref))
    rec = {"test": name, "mismatched_px": bad, "pixels": int(got.size), "rate": bad / max(1, got.size), "allowed_px": allow_px}
    _RATES.append(rec)
    print("LABELMAP", rec)
    try:
        import json
        d = os.path.join(ROOT, "gpurun_out")
        if os.path.isdir(d):
            with open(os.path.join(d, "labelmap_rates.jsonl"), "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    assert bad <= allow_px, rec
    return bad


@pytest.fixture(scope="session")
def gold():
    return golden


def grad_tol(key, ref, tol=1e-4):
    """Allowed abs error for a parameter-gradient tensor.  Conv biases that feed a BatchNorm have a
    mathematically-zero gradient (the batch mean absorbs the bias); both sides hold fp32 round-off noise
    there, so those keys are compared with an absolute floor (SURVEY 8a note R)."""
    ref = np.asarray(ref)
    bn_fed_bias = key.endswith(("conv_conv.0.bias", "conv_conv.4.bias"))
    return tol * float(np.max(np.abs(ref))) + (1e-5 if bn_fed_bias else 1e-7)


# ---------------------------------------------------------------------------------------------- backends
import subprocess


def _emul_stale():
    so = os.path.join(ROOT, "tests", "emul", "libwslhip_emul.so")
    if not os.path.exists(so):
        return True
    t = os.path.getmtime(so)
    srcs = [os.path.join(ROOT, "include", "wsl_hip.h"), os.path.join(ROOT, "tests", "emul", "hip_emul.h"),
            os.path.join(ROOT, "tests", "emul", "hip_emul.cpp")]
    cs = os.path.join(ROOT, "wsl4mis_amd", "csrc")
    srcs += [os.path.join(cs, f) for f in os.listdir(cs) if f.endswith((".hip", ".h"))]
    return any(os.path.getmtime(s) > t for s in srcs)


_BACKENDS = {}


def get_backend(name):
    if name not in _BACKENDS:
        import backends
        if name == "emul":
            if _emul_stale():
                subprocess.run([os.path.join(ROOT, "wsl4mis_amd", "csrc", "build.sh"), "emul"], check=True,
                               stdout=subprocess.DEVNULL)
            _BACKENDS[name] = backends.EmulBackend()
        elif name == "hip_exp":
            _BACKENDS[name] = backends.HipExpBackend()
        else:
            _BACKENDS[name] = backends.HipBackend()
    return _BACKENDS[name]


@pytest.fixture(params=[pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    """The C ABI behind either the host emulator (kernel-logic check, CPU) or the real library on cuda:0."""
    return get_backend(request.param)


@pytest.fixture(params=[pytest.param("emul"), pytest.param("hip_exp", marks=pytest.mark.gpu)])
def be_route(request):
    """For the tests that FORCE a route (tile plan, Winograd off, few persistent workgroups): the routing overrides exist only in builds with
    -DWSL_EXPERIMENTS -- the host emulator and tools/exp/libwslhip_exp.so (same kernel sources, hipcc, gfx950).  The product library has
    no such state."""
    return get_backend(request.param)
