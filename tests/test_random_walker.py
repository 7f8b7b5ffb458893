"""wsl_random_walker (csrc/wsl_rw.hip) against the float64 restatement of its contract (tests/rw_ref.py: scipy.sparse + splu):

  1 probabilities and labels on two small synthetic inputs (24 x 20, 33 x 47; two slices each) at tol 1e-6
  2 the residual contract at tol 1e-5: the true float64 residual of the returned probabilities against the reported one
  3 the five full-class slices of the committed ACDC volume at the default tol (labels only: see the test)
  4 the class rule (zeros, nothing solved), the prostate rule (K = 3)
  5 edges: constant image, fully seeded slice, H or W = 2, K = 2 and 8, max_iter = 3, unsupported sizes
  6 guard words around exactly the queried workspace
  7 bit-reproducibility (gpu)

Bounds.  1e-4 on the probabilities at tol 1e-6: an fp32 Jacobi-PCG restated in numpy reaches 7.8e-6 on both synthetic inputs; the bound
leaves an order of magnitude for another summation order.  Labels must agree wherever the float64 top-two gap is at least 1e-3 on the
synthetic inputs (every pixel: asserted) and 1e-2 on the real slices (at most 0.5 % of a slice may fall under it: asserted)."""
import os

import numpy as np
import pytest

import rw_ref
from conftest import get_backend, summary_line
from wsl4mis_amd import _lib
from wsl4mis_amd.dataloaders import h5lite

MAX_ITER = 10000


def rw_call(be, img, seed, K, tol, max_iter=MAX_ITER, beta=100.0, want_prob=True, ws=None):
    N, H, W = img.shape
    d = [be.arr(img.astype(np.float32)), be.arr(seed.astype(np.uint8))]
    lab, prob = be.zeros((N, H, W), np.uint8), be.zeros((N, K, H, W))
    it, res = be.zeros((N, K)), be.zeros((N, K))           # (iters: int32 words in a float32 buffer, viewed below)
    n = be.lib.wsl_random_walker_ws_bytes(N, H, W, K)
    assert n > 0
    wsb = be.ws(n)
    be.call("wsl_random_walker", be.ptr(d[0]), be.ptr(d[1]), be.ptr(lab), be.ptr(prob) if want_prob else None, be.ptr(it), be.ptr(res),
            N, H, W, K, beta, tol, max_iter, be.ptr(wsb), n, be.stream)
    be.sync()
    return be.np(lab).copy(), be.np(prob).copy(), be.np(it).view(np.int32).copy(), be.np(res).copy()


def check_against_ref(be, key, img, seed, K, tol=1e-6, gap=1e-3, every_pixel=False):
    """labels where the float64 gap is at least `gap`, probabilities within 1e-4, iteration counts and reported residuals"""
    ref = rw_ref.cached(key, img, seed, K)
    lab, prob, it, res = rw_call(be, img, seed, K, tol)
    worst = 0.0
    for n, r in enumerate(ref):
        sure = r["gap"] >= gap
        if every_pixel:
            assert sure.all(), (key, n, float(r["gap"].min()))
        assert np.array_equal(lab[n][sure], r["label"][sure]), (key, n, int((lab[n] != r["label"])[sure].sum()))
        err = float(np.abs(prob[n] - r["prob"]).max())
        print(f"random walker {key} slice {n} [{be.name}]: max |x - x_f64| {err:.2e}, iterations {it[n].tolist()}, residuals {res[n].tolist()}")
        assert err <= 1e-4, (key, n, err)
        worst = max(worst, err)
    assert np.all(it <= MAX_ITER) and np.all(it >= 0) and np.all(res <= tol), (it, res)
    return lab, prob, it, res, worst


# ================================================================================================ 1: small synthetic
@pytest.mark.parametrize("shape", [(24, 20), (33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_probabilities_and_labels_match_float64(be, shape):
    img, seed = rw_ref.synthetic()[shape]
    *_, it, _, worst = check_against_ref(be, ("syn", shape), img, seed, 4, tol=1e-6, every_pixel=True)
    assert np.all(it > 0)
    summary_line(f"RANDOM WALKER {shape[0]}x{shape[1]} [{be.name}]: max |x - x_f64| {worst:.2e} (allowed 1e-4), iterations {int(it.min())}..{int(it.max())}")


# ================================================================================================ 2: residual contract
# The recursively updated fp32 residual the kernel reports and the true float64 residual of the returned probabilities differ by
# rounding; by how much is not derivable, so it is measured (profiles/rw_margins.md): true residual / tol at tol 1e-5 on the two inputs
# is 1.015 and 0.992 on the host emulator.  Bound: 10 x the larger measured ratio, and never looser than 100 x tol.
TRUE_RESIDUAL_OVER_TOL = min(10 * 1.015, 100.0)


@pytest.mark.parametrize("shape", [(24, 20), (33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_true_residual_of_the_returned_probabilities(be, shape):
    tol = 1e-5
    img, seed = rw_ref.synthetic()[shape]
    ref = rw_ref.cached(("syn", shape), img, seed, 4)
    _, prob, it, res = rw_call(be, img, seed, 4, tol)
    assert np.all(res <= tol) and np.all(it <= MAX_ITER)
    worst = 0.0
    for n, r in enumerate(ref):
        true = rw_ref.true_residuals(r, prob[n])
        print(f"random walker residual {shape} slice {n} [{be.name}]: reported {res[n].tolist()}, true {true.tolist()}, "
              f"true / tol {(true / tol).tolist()}")
        worst = max(worst, float((true / tol).max()))
    summary_line(f"RANDOM WALKER residual {shape[0]}x{shape[1]} [{be.name}]: true residual / tol {worst:.3f} (allowed {TRUE_RESIDUAL_OVER_TOL})")
    assert worst <= TRUE_RESIDUAL_OVER_TOL, worst


# ================================================================================================ 3: real slices
def real_case(be):
    """GPU: slices 1..5 whole.  Emulator: a 64 x 64 crop of slice 3 that keeps all four classes (seconds, not minutes)."""
    img, scr = rw_ref.volume()
    assert img.shape == (6, 224, 154)
    if be.name != "emul":
        return "acdc_1to5", img[1:6].copy(), scr[1:6].copy()
    for y0 in range(0, 224 - 64 + 1, 8):
        for x0 in range(0, 154 - 64 + 1, 8):
            s = scr[3, y0:y0 + 64, x0:x0 + 64]
            if all(k in s for k in range(4)):
                return f"acdc_3_crop_{y0}_{x0}", img[3:4, y0:y0 + 64, x0:x0 + 64].copy(), s[None].copy()
    raise AssertionError("no 64 x 64 crop of slice 3 holds all four classes")


def check_real(be, lab, key, img, seed):
    ref = rw_ref.cached(key, img, seed, 4)
    for n, r in enumerate(ref):
        assert rw_ref.class_rule(seed[n], 4)
        sure = r["gap"] >= 1e-2
        share = 1.0 - float(sure.mean())
        bad = int((lab[n] != r["label"])[sure].sum())
        print(f"random walker {key} slice {n} [{be.name}]: {bad} mismatches, {share:.4%} excluded, {int((lab[n] != r['label']).sum())} "
              "mismatches anywhere")
        assert share <= 0.005, (key, n, share)
        assert bad == 0, (key, n, bad)


def test_real_slices_labels_match_float64(be):
    """Probabilities are NOT compared here: at tol 1e-5 they differ from the direct solve by up to 0.16 in nearly isolated regions
    while the labels agree -- conditioning, not a defect."""
    key, img, seed = real_case(be)
    lab, _, it, res = rw_call(be, img, seed, 4, 1e-5)
    assert np.all(res <= 1e-5) and np.all(it <= MAX_ITER) and np.all(it > 0), (it, res)
    summary_line(f"RANDOM WALKER {key} [{be.name}]: iterations {int(it.min())}..{int(it.max())}")
    check_real(be, lab, key, img, seed)


# ================================================================================================ 4: class rule
def assert_zeroed(out):
    lab, prob, it, res = out
    assert not lab.any() and not prob.any() and not it.any() and not res.any()


def test_class_rule_zeroes_slices_that_lack_a_foreground_class(be):
    img, scr = rw_ref.volume()
    assert not rw_ref.class_rule(scr[0], 4) and 1 not in scr[0]
    assert_zeroed(rw_call(be, img[:1], scr[:1], 4, 1e-5))
    files = sorted(os.listdir(rw_ref.SLICES))
    assert len(files) == 4
    for f in files:
        with h5lite.File(os.path.join(rw_ref.SLICES, f)) as h:
            im, sc = h["image"][:], h["scribble"][:]
        assert 1 not in sc
        assert_zeroed(rw_call(be, im[None], sc[None], 4, 1e-5))
    # a batch where only the second slice fails: the first is solved
    im, sd = (a.copy() for a in rw_ref.synthetic()[(24, 20)])
    sd[1][sd[1] == 3] = 4
    lab, prob, it, res = rw_call(be, im, sd, 4, 1e-6)
    assert_zeroed((lab[1], prob[1], it[1], res[1]))
    assert np.array_equal(lab[0], rw_ref.cached(("syn", (24, 20)), *rw_ref.synthetic()[(24, 20)], 4)[0]["label"]) and np.all(it[0] > 0)


def test_prostate_rule_solves_three_classes(be):
    im, sd = (a.copy() for a in rw_ref.synthetic()[(24, 20)])
    sd[sd == 3] = 4                                          # classes 0, 1, 2; 3 and 4 both mean unlabelled for K = 3
    *_, it, _, _ = check_against_ref(be, "syn_k3", im, sd, 3)
    assert np.all(it > 0)


# ================================================================================================ 5: edges
def test_constant_image_takes_the_limit_weights(be):
    """std(d) == 0: w = 1 + 1e-6 everywhere (the limit value; skimage would return NaN) -- DELIBERATE"""
    _, sd = rw_ref.synthetic()[(24, 20)]
    sd = sd[:1].copy()
    sd[0][sd[0] == 3] = 4
    sd[0, 20, 3:6] = 3                                       # off the symmetry axis: no exact ties in the harmonic solution
    im = np.full((1, 24, 20), 0.37, np.float32)
    lab, prob, *_ = check_against_ref(be, "constant", im, sd, 4, every_pixel=True)
    assert np.all(np.isfinite(prob)) and set(np.unique(lab).tolist()) == {0, 1, 2, 3}


def test_fully_seeded_slice_returns_its_seeds(be):
    rng = np.random.default_rng(2)
    sd = rng.integers(0, 4, (1, 9, 7)).astype(np.uint8)
    lab, prob, it, res = rw_call(be, rng.random((1, 9, 7), dtype=np.float32), sd, 4, 1e-5)
    assert np.array_equal(lab, sd) and not it.any() and not res.any()
    assert np.array_equal(prob[0], (sd[0][None] == np.arange(4)[:, None, None]).astype(np.float32))


def random_case(seed, H, W, K):
    """noise of amplitude 0.1: the exponent beta (d_p - d_q)^2 / (10 std) scales with the amplitude, so every weight stays above
    e^-5 and the system is as well conditioned as the synthetic ones -- the same 1e-4 on the probabilities applies.  (White noise of
    amplitude 1 gives weights down to 1e-6: nearly isolated pixels, whose probabilities no iterative solve at tol 1e-6 pins down.)"""
    rng = np.random.default_rng(seed)
    im = (0.45 + 0.1 * rng.random((1, H, W))).astype(np.float32)
    sd = np.full((1, H, W), K, np.uint8)
    pos = rng.permutation(H * W)[:2 * K]
    sd.reshape(-1)[pos] = np.arange(2 * K) % K               # two seeds per class
    return im, sd


@pytest.mark.parametrize("case", [(2, 9, 2), (9, 2, 2), (2, 2, 2), (16, 12, 2), (16, 12, 8)], ids=lambda c: "{}x{}_K{}".format(*c))
def test_thin_slices_and_class_counts(be, case):
    H, W, K = case
    im, sd = random_case(H * 100 + W + K, H, W, K)
    check_against_ref(be, ("random", case), im, sd, K)


def test_max_iter_is_a_hard_bound(be):
    img, seed = rw_ref.synthetic()[(33, 47)]
    lab, prob, it, res = rw_call(be, img, seed, 4, 1e-6, max_iter=3)
    assert np.all(it == 3) and np.all(res > 1e-6) and np.all(np.isfinite(prob))
    lab, prob, it, res = rw_call(be, img, seed, 4, 1e-6, max_iter=0)
    assert not it.any() and np.all(res == 1.0)


def test_unsupported_sizes_are_reported(be):
    x, s, o = be.zeros((1, 4, 4)), be.zeros((1, 4, 4), np.uint8), be.zeros((64,))
    ws = be.ws(1 << 16)
    P = be.ptr

    def call(N=1, H=4, W=4, K=4, mi=10, img=P(x)):
        return be.lib.wsl_random_walker(img, P(s), P(s), None, P(o), P(o), N, H, W, K, 100.0, 1e-5, mi, P(ws), 1 << 16, be.stream)

    for kw in (dict(H=1), dict(W=1), dict(K=1), dict(K=9), dict(N=0), dict(mi=-1), dict(mi=100001), dict(H=2048, W=1024)):
        assert call(**kw) == -2, kw                          # WSL_EUNSUPPORTED
        assert b"random_walker" in be.lib.wsl_last_error()
    assert call(img=None) == -1
    assert be.lib.wsl_random_walker_ws_bytes(1, 1, 4, 4) == 0 and be.lib.wsl_random_walker_ws_bytes(1, 4, 4, 9) == 0
    be.sync()


# ================================================================================================ 6: workspace
GUARD, FILL = 64 * 1024, 0x5A                               # the pattern of tests/test_workspace_guards.py


def _filled(be, shape, dtype=np.float32):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return be.arr(np.full(n, FILL, np.uint8).view(dtype).reshape(shape))


def _pattern_only(be, a):
    return bool(np.all(be.np(a).reshape(-1).view(np.uint8) == FILL))


@pytest.mark.parametrize("case", [(1, 24, 20, 4), (3, 33, 47, 4), (2, 16, 12, 8)], ids=lambda c: "-".join(map(str, c)))
def test_call_stays_inside_its_workspace(be, case):
    """[guard | workspace of exactly the queried bytes | guard], pattern-filled: both guards untouched after the call; one byte less
    returns WSL_EWORKSPACE and writes nothing anywhere"""
    N, H, W, K = case
    rng = np.random.default_rng(sum(case))
    if (H, W) in rw_ref.synthetic():
        im, sd = (np.concatenate([a, a])[:N] for a in rw_ref.synthetic()[(H, W)])
    else:
        one = [random_case(7 + n, H, W, K) for n in range(N)]
        im, sd = np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one])
    im, sd = be.arr(im.astype(np.float32)), be.arr(sd.astype(np.uint8))
    nbytes = int(be.lib.wsl_random_walker_ws_bytes(N, H, W, K))
    assert nbytes > 0 and nbytes % 4 == 0
    words = nbytes // 4
    P = be.ptr

    def run(nb):
        buf = _filled(be, (GUARD + words + GUARD,))
        outs = [_filled(be, (N, H, W), np.uint8), _filled(be, (N, K, H, W)), _filled(be, (N, K)), _filled(be, (N, K))]
        rc = be.lib.wsl_random_walker(P(im), P(sd), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), N, H, W, K, 100.0, 1e-5, 200,
                                      P(buf) + 4 * GUARD, nb, be.stream)
        be.sync()
        return rc, buf, outs

    rc, buf, outs = run(nbytes)
    assert rc == 0, be.lib.wsl_last_error()
    w = be.np(buf).view(np.uint32)
    word = np.uint32(FILL * 0x01010101)
    assert int((w[:GUARD] != word).sum()) == 0 and int((w[GUARD + words:] != word).sum()) == 0
    assert be.np(outs[2]).view(np.int32).max() > 0 and not _pattern_only(be, outs[0])
    rc, buf, outs = run(nbytes - 1)
    msg = be.lib.wsl_last_error().decode()
    assert rc == -4 and str(nbytes - 1) in msg and str(nbytes) in msg, (rc, msg)
    assert _pattern_only(be, buf) and all(_pattern_only(be, o) for o in outs)
    del rng


# ================================================================================================ 7: reproducibility
@pytest.mark.gpu
def test_two_runs_are_bit_identical_gpu():
    be = get_backend("hip")
    _, img, seed = real_case(be)
    a = rw_call(be, img, seed, 4, 1e-5)
    b = rw_call(be, img, seed, 4, 1e-5)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ================================================================================================ python wrapper
@pytest.fixture(params=[pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)])
def mode(request):
    from wsl4mis_amd import runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    if request.param == "emul":
        _lib.use_library_for_tests(get_backend("emul").lib)
    yield request.param
    _lib._reset_for_tests()
    runtime._ws_cache.clear()


def test_wrapper_returns_labels_and_raises_above_tol(mode):
    import torch
    from wsl4mis_amd import runtime
    from wsl4mis_amd.dataloaders.random_walker import random_walker_labels
    img, seed = rw_ref.synthetic()[(24, 20)]
    ref = rw_ref.cached(("syn", (24, 20)), img, seed, 4)
    lab, prob = random_walker_labels(torch.from_numpy(img), torch.from_numpy(seed), tol=1e-6, return_prob=True)
    assert lab.dtype == torch.uint8 and lab.device == runtime.device() and tuple(prob.shape) == (2, 4, 24, 20)
    assert np.array_equal(lab.cpu().numpy(), np.stack([r["label"] for r in ref]))
    assert np.array_equal(random_walker_labels(img, seed.astype(np.uint16)).cpu().numpy(), lab.cpu().numpy())
    with pytest.raises(_lib.WslError, match=r"slice 0, class \d: relative residual .* after 3 iterations"):
        random_walker_labels(img, seed, tol=1e-6, max_iter=3)
    with pytest.raises(_lib.WslError, match="unsupported"):
        random_walker_labels(img[:, :1], seed[:, :1])
