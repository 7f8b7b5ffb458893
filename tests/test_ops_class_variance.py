"""wsl_class_variance_fwd_bwd and the WSL_REG_CLASS_VAR kind of wsl_head_reg_fwd_bwd (include/wsl_hip.h) against float64.

Reference: the float64 torch expression of the inter/intra-class trainer's two functions,
    intra = std(img * p, dim=[2, 3]).mean()                     inter = std(mean(img * p, dim=[2, 3]), dim=1).mean()
evaluated here with autograd on the EXACT float32 inputs.  Criteria: those of tests/test_ops_loss_sweep.py -- tensors close(., ., 1e-4) (both
criteria of conftest.py), loss scalars 1e-5 relative, for inter, intra and inter - intra separately.  For the fused head the sweep's rule:
the regulariser is evaluated on the softmax the kernel returned and its gradient is propagated through the float64 softmax backward.

Sizes: C in {2, 3, 4, 5, 8} (one moment-kernel instantiation each), (N, H, W) from two pixels to 96 x 128; 64 x 80 = 5120 pixels is one full
4096-pixel chunk and a ragged second one, 96 x 128 exactly three chunks; odd H * W take the scalar gradient kernel, H * W % 4 == 0 the
128-bit one; on the GPU also 5 x 256 x 256.  Logits are 2 randn + c per class c: with unbiased logits the class means differ only by
~1 / sqrt(H W) and `inter` itself becomes ill-conditioned (a float32 model reaches 5e-6 relative there, against < 1e-6 with the bias).
The worst measured errors reach the terminal summary (recorded in profiles/interintra_margins.md)."""
import numpy as np
import pytest
import torch

from conftest import close, golden, mixed_err, rel_err, summary_line
from test_workspace_guards import filled, guard_check

TOL, LTOL = 1e-4, 1e-5
EINVAL, EWORKSPACE = -1, -4
CLASSES = (2, 3, 4, 5, 8)
SHAPES = [(1, 1, 2), (2, 7, 9), (3, 17, 23), (2, 40, 44), (2, 64, 80), (1, 96, 128)]
WEIGHTS = [(1.0, -1.0), (0.3, 0.0), (0.0, -0.7)]
CASES = [(c,) + s for c in CLASSES for s in SHAPES]
GPU_CASE = (4, 5, 256, 256)


def _id(c):
    return "C{}_{}x{}x{}".format(*c)


_WORST = {}


def _note(entry, be, kind, err, what):
    rec = _WORST.setdefault((entry, be.name), {})
    if err >= rec.get(kind, (-1.0, ""))[0]:
        rec[kind] = (err, what)


def check_t(entry, be, got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (entry, what)
    r, m = rel_err(got, ref), mixed_err(got, ref, TOL)
    print(f"CLASS-VAR {entry} [{be.name}] {what}: rel_err {r:.3e} mixed_err {m:.3e}")
    _note(entry, be, "rel_err", r, what)
    _note(entry, be, "mixed_err", m, what)
    assert close(got, ref, TOL), (entry, what, r, m)


def check_s(entry, be, got, ref, what):
    got, ref = float(got), float(ref.detach() if isinstance(ref, torch.Tensor) else ref)
    assert np.isfinite(got), (entry, what, got)
    e = rel_err(got, ref)
    print(f"CLASS-VAR {entry} [{be.name}] {what}: {got!r} vs {ref!r} ({e:.3e})")
    _note(entry, be, "loss", e, what)
    assert e < LTOL, (entry, what, got, ref, e)


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    lines = [f"CLASS-VAR {entry} [{name}]: " + "; ".join(
        f"worst {k} {v[0]:.2e} (bound {'1e-5' if k == 'loss' else ('1e-4' if k == 'rel_err' else '1')}) at {v[1]}" for k, v in sorted(rec.items()))
        for (entry, name), rec in sorted(_WORST.items())]
    for ln in lines:
        summary_line(ln)
    _WORST.clear()


# ------------------------------------------------------------------------------------------------ inputs and the float64 reference
def _rng(case, salt):
    return np.random.default_rng([salt] + [int(v) + 1 for v in case])


def biased_logits(rng, shape):
    return (2.0 * rng.standard_normal(shape) + 1.0 * np.arange(shape[1]).reshape(1, -1, 1, 1)).astype(np.float32)


def d64(a):
    return torch.from_numpy(np.asarray(a)).double()


def ref_terms(p, img):
    q = img * p
    return torch.std(q.mean(dim=[2, 3]), dim=1).mean(), torch.std(q, dim=[2, 3]).mean()


def lws(be, N, C, HW):
    n = be.lib.wsl_loss_ws_bytes(N, C, HW)
    return be.ws(n), n


def _inputs(case, salt):
    C, N, H, W = case
    rng = _rng(case, salt)
    z = biased_logits(rng, (N, C, H, W))
    img = (rng.random((N, 1, H, W)) + 0.05).astype(np.float32)
    return z, torch.softmax(torch.from_numpy(z), 1).numpy(), img


def _standalone(be, p, img, wi, wa, entry="wsl_class_variance_fwd_bwd", what=""):
    N, C, H, W = p.shape
    dp_, di = be.arr(p), be.arr(img)
    loss, dp = be.arr(np.full(3, 7.0, np.float32)), be.arr(np.full(p.shape, 7.0, np.float32))
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_class_variance_fwd_bwd", be.ptr(di), be.ptr(dp_), be.ptr(loss), be.ptr(dp), wi, wa, N, C, H, W, be.ptr(ws), n, be.stream)
    o = be.np(loss)
    pt = d64(p).requires_grad_()
    inter, intra = ref_terms(pt, d64(img))
    (float(np.float32(wi)) * inter + float(np.float32(wa)) * intra).backward()
    check_s(entry, be, o[1], inter, what + " inter")
    check_s(entry, be, o[2], intra, what + " intra")
    check_s(entry, be, o[0], inter - intra, what + " inter-intra")
    check_t(entry, be, be.np(dp), pt.grad, what + " dp")
    return o, be.np(dp)


def _run_standalone(be, case):
    _, p, img = _inputs(case, 31)
    for wi, wa in WEIGHTS:
        _standalone(be, p, img, wi, wa, what=f"{_id(case)} w=({wi},{wa})")


def _run_fused(be, case, teacher):
    C, N, H, W = case
    z, _, img = _inputs(case, 32)
    rng = _rng(case, 33)
    shape, w_ce, rw, cw, ignore = (N, C, H, W), 0.8, 0.6, 0.07, C
    zt = biased_logits(rng, shape)
    lab = np.full((N, H, W), C, np.uint8)
    m = rng.random((N, H, W)) < 0.25
    lab[m] = rng.integers(0, C, int(m.sum()))
    lab.reshape(-1)[0] = 0
    d = {k: be.arr(v) for k, v in dict(z=z, zt=zt, lab=lab, img=img).items()}
    out, dz, s, ds = be.arr(np.full((8,), 7.0, np.float32)), be.zeros(shape), be.zeros(shape), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_head_reg_fwd_bwd", be.ptr(d["z"]), be.ptr(d["lab"]), ignore, w_ce, 4, rw, be.ptr(d["img"]),
            be.ptr(d["zt"]) if teacher else None, cw, be.ptr(out), be.ptr(dz), be.ptr(s), be.ptr(ds), N, C, H, W, be.ptr(ws), n, be.stream)
    entry, what = "wsl_head_reg_fwd_bwd(kind 4)", f"{_id(case)} teacher={int(teacher)}"
    o = be.np(out)
    t = d64(z).requires_grad_()
    st = torch.softmax(t, 1)
    check_t(entry, be, be.np(s), st, what + " s")
    sk = d64(be.np(s)).requires_grad_()                         # the regulariser on the softmax the kernel returned
    inter, intra = ref_terms(sk, d64(img))
    cons = torch.mean((sk - torch.softmax(d64(zt), 1)) ** 2) if teacher else None
    check_s(entry, be, o[6], inter, what + " inter")
    check_s(entry, be, o[7], intra, what + " intra")
    check_s(entry, be, o[4], inter - intra, what + " inter-intra")
    if teacher:
        check_s(entry, be, o[5], cons, what + " cons")
    else:
        assert o[5] == 0.0, what
    (float(np.float32(rw)) * (inter - intra) + (cw * cons if teacher else 0.0)).backward()
    st.backward(sk.grad, retain_graph=True)                     # ... propagated through the float64 softmax backward
    ce = torch.nn.functional.cross_entropy(t, torch.from_numpy(lab.astype(np.int64)), ignore_index=ignore)
    check_s(entry, be, o[0], ce, what + " loss")
    check_s(entry, be, o[1], ce, what + " ce")
    assert o[3] == int(np.sum(lab != ignore)) and o[2] == 0.0, what
    (w_ce * ce).backward()
    check_t(entry, be, be.np(dz), t.grad, what + " dz")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_class_variance_sweep(be, case):
    _run_standalone(be, case)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_head_class_variance_sweep(be, case):
    _run_fused(be, case, teacher=CASES.index(case) % 2 == 1)


@pytest.mark.gpu
def test_class_variance_full_size():
    """5 x 256 x 256 at C = 4: 16 chunks per sample, the size of a training step"""
    from conftest import get_backend
    be = get_backend("hip")
    _run_standalone(be, GPU_CASE)
    _run_fused(be, GPU_CASE, True)


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("shape", [(2, 4, 40, 44), (2, 4, 64, 80), (1, 3, 96, 128)], ids=lambda s: "x".join(map(str, s)))
def test_near_constant_planes_need_centred_moments(be, shape):
    """img = 0.9 + 0.01 randn and +12 on class 0: q of class 0 is 0.9 +- 0.01, its variance 1e-4 of its squared mean -- the one-pass
    sum q^2 - (sum q)^2 / M form in float32 is off by 3e-5 .. 2e-4 here, the centred chunked form by < 1e-7.  Same bounds as the sweep."""
    N, C, H, W = shape
    rng = np.random.default_rng([7, N, C, H, W])
    z = (0.5 * rng.standard_normal(shape)).astype(np.float32)
    z[:, 0] += 12.0
    img = (0.9 + 0.01 * rng.standard_normal((N, 1, H, W))).astype(np.float32)
    p = torch.softmax(torch.from_numpy(z), 1).numpy()
    for wi, wa in WEIGHTS:
        _standalone(be, p, img, wi, wa, entry="wsl_class_variance_fwd_bwd(conditioning)", what=f"{'x'.join(map(str, shape))} w=({wi},{wa})")


# ------------------------------------------------------------------------------------------------ zero variance, bad arguments
def test_all_zero_image_slice_gives_zero_gradient(be):
    """sigma[n, c] == 0 and tau[n] == 0 for the blank sample: its terms are 0 and its dp is EXACTLY 0 (the contract; what torch.std
    returns), everything finite; the other samples are unaffected"""
    case = (4, 3, 17, 23)
    _, p, img = _inputs(case, 41)
    img[1] = 0.0
    o, dp = _standalone(be, p, img, 1.0, -1.0, entry="wsl_class_variance_fwd_bwd(zero image)", what=_id(case))
    assert np.all(dp[1] == 0.0) and np.all(np.isfinite(dp)) and np.all(np.isfinite(o))
    assert np.any(dp[0] != 0.0) and np.any(dp[2] != 0.0)


def test_all_zero_logits_give_zero_inter(be):
    """equal class means: inter is exactly 0 and contributes no gradient -- through the fused head (softmax of zeros) and stand-alone"""
    N, C, H, W = 2, 4, 40, 44
    rng = np.random.default_rng(5)
    img = (rng.random((N, 1, H, W)) + 0.05).astype(np.float32)
    p = np.full((N, C, H, W), 0.25, np.float32)
    got, di, dp_ = [], be.arr(img), be.arr(p)
    for wi, wa in ((1.0, -1.0), (0.0, -1.0)):
        loss, dp = be.zeros((3,)), be.arr(np.full(p.shape, 7.0, np.float32))
        ws, n = lws(be, N, C, H * W)
        be.call("wsl_class_variance_fwd_bwd", be.ptr(di), be.ptr(dp_), be.ptr(loss), be.ptr(dp), wi, wa, N, C, H, W, be.ptr(ws),
                n, be.stream)
        got.append((be.np(loss).copy(), be.np(dp).copy()))
    (l1, d1), (l0, d0) = got
    assert l1[1] == 0.0 and l1[0] == -l1[2] and l1[2] > 0 and np.all(np.isfinite(d1))
    assert np.array_equal(d1, d0), "the gradient must equal the intra part alone"
    pt = d64(p).requires_grad_()
    (-ref_terms(pt, d64(img))[1]).backward()
    assert close(d1, pt.grad.numpy(), TOL)
    # fused: all-zero logits
    z, lab = np.zeros((N, C, H, W), np.float32), np.full((N, H, W), 4, np.uint8)
    lab[:, 3, 5] = 1
    dz_, dl = be.arr(z), be.arr(lab)
    out, dz, s, ds = be.zeros((8,)), be.zeros(z.shape), be.zeros(z.shape), be.zeros(z.shape)
    be.call("wsl_head_reg_fwd_bwd", be.ptr(dz_), be.ptr(dl), 4, 1.0, 4, 0.5, be.ptr(di), None, 0.0, be.ptr(out),
            be.ptr(dz), be.ptr(s), be.ptr(ds), N, C, H, W, be.ptr(ws), n, be.stream)
    o = be.np(out)
    assert o[6] == 0.0 and o[4] == -o[7] and np.all(np.isfinite(be.np(dz))) and np.all(np.isfinite(o))
    assert rel_err(be.np(ds), 0.5 * d0) < 1e-6                        # ds = 0.5 * d(inter - intra)/ds = 0.5 * d(-intra)/ds


def test_bad_arguments_are_refused_and_write_nothing(be):
    N, C, H, W = 2, 3, 6, 5
    rng = np.random.default_rng(3)
    img, p = be.arr(rng.random((N, 1, H, W)).astype(np.float32)), be.arr(rng.random((N, C, H, W)).astype(np.float32))
    ws, n = lws(be, N, 8, H * W)

    def refused(fn, outs, *args):
        rc = getattr(be.lib, fn)(*args)
        be.sync()
        assert rc == EINVAL, (fn, rc)
        from test_workspace_guards import untouched
        assert all(untouched(be, o) for o in outs), fn

    for (c, h, w) in ((1, H, W), (C, 1, 1), (9, H, W)):
        loss, dp = filled(be, (3,)), filled(be, (N, C, H, W))
        refused("wsl_class_variance_fwd_bwd", [loss, dp], be.ptr(img), be.ptr(p), be.ptr(loss), be.ptr(dp), 1.0, -1.0, N, c, h, w, be.ptr(ws), n,
                be.stream)
    lab = be.arr(np.zeros((N, H, W), np.uint8))
    for (c, h, w, im) in ((C, H, W, None), (1, H, W, img), (C, 1, 1, img)):
        outs = [filled(be, (8,)), filled(be, (N, C, H, W)), filled(be, (N, C, H, W)), filled(be, (N, C, H, W))]
        refused("wsl_head_reg_fwd_bwd", outs, be.ptr(p), be.ptr(lab), C, 1.0, 4, 0.1, be.ptr(im) if im is not None else None, None, 0.0,
                be.ptr(outs[0]), be.ptr(outs[1]), be.ptr(outs[2]), be.ptr(outs[3]), N, c, h, w, be.ptr(ws), n, be.stream)


# ------------------------------------------------------------------------------------------------ fused == chain
@pytest.mark.parametrize("teacher", [False, True], ids=["plain", "teacher"])
@pytest.mark.parametrize("shape", [(3, 4, 40, 44), (2, 5, 64, 80)], ids=lambda s: "x".join(map(str, s)))
def test_fused_class_variance_head_equals_the_chain_of_calls(be, shape, teacher):
    """wsl_head_reg_fwd_bwd(kind 4) == wsl_head_fwd_bwd + wsl_softmax_fwd + wsl_class_variance_fwd_bwd + wsl_softmax_bwd + wsl_axpy
    (+ wsl_softmax_mse_fwd_bwd + wsl_axpy) to the criteria tests/test_ops_loss.py applies to kinds 1-3"""
    N, C, H, W = shape
    rng = np.random.default_rng([44, N, C])
    w, cw = 0.1, 0.07
    z, zt = biased_logits(rng, shape), biased_logits(rng, shape)
    lab = np.full((N, H, W), C, np.uint8)
    lab[rng.random((N, H, W)) < 0.1] = rng.integers(0, C)
    img = rng.random((N, 1, H, W)).astype(np.float32)
    d = {k: be.arr(v) for k, v in dict(z=z, zt=zt, lab=lab, img=img).items()}
    ws, n = lws(be, N, C, H * W)
    o1, a, s1, ds1, dzx = be.zeros((8,)), be.zeros(shape), be.zeros(shape), be.zeros(shape), be.zeros(shape)
    be.call("wsl_head_fwd_bwd", be.ptr(d["z"]), None, be.ptr(d["lab"]), C, 0.0, 0.0, 1.0, be.ptr(o1), None, be.ptr(a), None, N, C, H * W,
            be.ptr(ws), n, be.stream)
    be.call("wsl_softmax_fwd", be.ptr(d["z"]), be.ptr(s1), N, C, H * W, be.stream)
    reg = be.zeros((3,))
    be.call("wsl_class_variance_fwd_bwd", be.ptr(d["img"]), be.ptr(s1), be.ptr(reg), be.ptr(ds1), w, -w, N, C, H, W, be.ptr(ws), n, be.stream)
    be.call("wsl_softmax_bwd", be.ptr(s1), be.ptr(ds1), be.ptr(dzx), N, C, H * W, be.stream)
    be.call("wsl_axpy", be.ptr(a), be.ptr(dzx), 1.0, N * C * H * W, be.stream)
    cons = be.zeros((1,))
    if teacher:
        be.call("wsl_softmax_mse_fwd_bwd", be.ptr(d["z"]), be.ptr(d["zt"]), be.ptr(cons), be.ptr(dzx), cw, N, C, H * W, be.ptr(ws), n, be.stream)
        be.call("wsl_axpy", be.ptr(a), be.ptr(dzx), 1.0, N * C * H * W, be.stream)
    o2, b, s2, ds2 = be.arr(np.full((8,), 7.0, np.float32)), be.zeros(shape), be.zeros(shape), be.zeros(shape)
    be.call("wsl_head_reg_fwd_bwd", be.ptr(d["z"]), be.ptr(d["lab"]), C, 1.0, 4, w, be.ptr(d["img"]), be.ptr(d["zt"]) if teacher else None,
            cw, be.ptr(o2), be.ptr(b), be.ptr(s2), be.ptr(ds2), N, C, H, W, be.ptr(ws), n, be.stream)
    r, g = be.np(reg), be.np(o2)
    assert rel_err(be.np(s2), be.np(s1)) < 5e-7
    assert rel_err(g[:4], be.np(o1)[:4]) < 1e-6
    for got, ref in ((g[4], r[0]), (g[6], r[1]), (g[7], r[2])):
        assert abs(got - ref) <= 1e-6 * abs(ref), (g, r)
    if teacher:
        assert abs(g[5] - be.np(cons)[0]) <= 1e-6 * abs(be.np(cons)[0])
    else:
        assert g[5] == 0.0
    assert rel_err(be.np(b), be.np(a)) < 2e-6, rel_err(be.np(b), be.np(a))


# ------------------------------------------------------------------------------------------------ workspace, reproducibility, golden
@pytest.mark.parametrize("case", [(4, 3, 40, 44), (8, 2, 64, 80), (8, 1, 1, 700), (5, 2, 600, 3)], ids=_id)
def test_workspace_guards(be, case):
    """both entry points inside guard words at exactly wsl_loss_ws_bytes; one byte less returns WSL_EWORKSPACE and writes nothing"""
    C, N, H, W = case
    z, p, img = _inputs(case, 51)
    lab = np.full((N, H, W), C, np.uint8)
    lab[:, 0, 0] = 1
    d = {k: be.arr(v) for k, v in dict(z=z, p=p, img=img, lab=lab).items()}
    nbytes = be.lib.wsl_loss_ws_bytes(N, C, H * W)

    def run_a(ws, n, outs):
        be.call("wsl_class_variance_fwd_bwd", be.ptr(d["img"]), be.ptr(d["p"]), be.ptr(outs[0]), be.ptr(outs[1]), 1.0, -1.0, N, C, H, W, ws, n,
                be.stream)

    def run_b(ws, n, outs):
        be.call("wsl_head_reg_fwd_bwd", be.ptr(d["z"]), be.ptr(d["lab"]), C, 1.0, 4, 0.1, be.ptr(d["img"]), None, 0.0, be.ptr(outs[0]),
                be.ptr(outs[1]), be.ptr(outs[2]), be.ptr(outs[3]), N, C, H, W, ws, n, be.stream)

    guard_check(be, nbytes, lambda: [filled(be, (3,)), filled(be, (N, C, H, W))], run_a)
    guard_check(be, nbytes, lambda: [filled(be, (8,))] + [filled(be, (N, C, H, W)) for _ in range(3)], run_b)


def test_two_runs_are_bit_equal(be):
    case = (4, 2, 64, 80)
    _, p, img = _inputs(case, 61)
    C, N, H, W = case
    runs, di, dp_ = [], be.arr(img), be.arr(p)
    for _ in range(2):
        loss, dp = be.zeros((3,)), be.zeros(p.shape)
        ws, n = lws(be, N, C, H * W)
        be.call("wsl_class_variance_fwd_bwd", be.ptr(di), be.ptr(dp_), be.ptr(loss), be.ptr(dp), 1.0, -1.0, N, C, H, W, be.ptr(ws),
                n, be.stream)
        runs.append((be.np(loss).copy(), be.np(dp).copy()))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32)) and np.any(runs[0][1] != 0)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_values_and_gradient(be, tag):
    """g14_interintra (tests/golden/make_golden_interintra.py): the reference's own functions.  Against their float64 run at the sweep's
    criteria; against their float32 run at 1e-4 (two float32 evaluations of the same expression)"""
    g = golden("g14_interintra")
    p, img = g[f"{tag}_p"], g[f"{tag}_img"]
    N, C, H, W = p.shape
    loss, dp, di, dp_ = be.zeros((3,)), be.zeros(p.shape), be.arr(img), be.arr(p)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_class_variance_fwd_bwd", be.ptr(di), be.ptr(dp_), be.ptr(loss), be.ptr(dp), 1.0, -1.0, N, C, H, W, be.ptr(ws), n,
            be.stream)
    o = be.np(loss)
    v64, v32 = g[f"{tag}_f64_values"], g[f"{tag}_f32_values"]
    check_s("wsl_class_variance_fwd_bwd(golden)", be, o[1], v64[0], tag + " inter")
    check_s("wsl_class_variance_fwd_bwd(golden)", be, o[2], v64[1], tag + " intra")
    check_s("wsl_class_variance_fwd_bwd(golden)", be, o[0], v64[0] - v64[1], tag + " inter-intra")
    check_t("wsl_class_variance_fwd_bwd(golden)", be, be.np(dp), g[f"{tag}_f64_dp"], tag + " dp")
    assert rel_err(o[1:], v32) < TOL and close(be.np(dp), g[f"{tag}_f32_dp"], TOL)
