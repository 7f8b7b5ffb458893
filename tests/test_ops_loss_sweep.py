"""Every loss entry point of the C ABI against a float64 reference, over class counts, sizes, label forms and edges.

Reference: oracle/torch_ref.py evaluated on .double() tensors with autograd.  Inputs are generated as float32 and converted EXACTLY to
float64, so selections (TV's erosion / dilation arg-extrema, Mumford-Shah's signs) are decided on identical values on both sides.  The
fused entry points are compared with the reference COMPOSITION (not with the chain of calls: tests/test_ops_loss.py does that).

Grid: C in {1, 2, 3, 4, 5, 8} (the generic class-count instantiations <0> of the head / mixprob kernels run for every C != 4), ignore index
= C (the scribble convention) and, for C = 5 and 8, also ignore = 4 (a real class is ignored); (N, H, W) from one pixel to 9600 pixels = 38
workgroups, which reaches the unrolled loop and the tail of head_finalize_kernel; on the GPU also the sizes whose grid-stride loops run
more than once (N * HW > 1024 * 256; HW > 262144 for the pDice kernels, which grid over HW alone).

Decisions that rounding could flip are handled explicitly, never by a tolerance:
  * pseudo labels of the heads: the pDice part of the reference uses the label map the kernel returned; separately that map must equal
    the float64 arg-max on every pixel whose float64 top-2 margin is >= 1e-5, and at most 0.1 % of the pixels may lie below the margin;
  * the fused regulariser head: the regulariser's selections are taken on the softmax the kernel returned (itself compared with the
    float64 softmax), its gradient is propagated through the float64 softmax backward;
  * the USTM certainty mask: pmean is bimodal, the threshold lies between the modes and no pixel's float64 uncertainty may be within
    1e-3 of it; the mask count must then match exactly.
  * ignore = 4 with C > 4: the cross-entropy ignores class 4; the head's pDice term masks nothing (its pseudo labels are never the ignore
    index by construction of the trainers: include/wsl_hip.h), so the reference's pDice runs with ignore = C there.

Tolerances are the project's own: tensors pass close(got, ref, 1e-4) (both criteria of conftest.py), loss scalars agree to 1e-5
(rel_err, as tests/test_ops_loss.py).  The worst measured errors per entry point and backend reach the terminal summary."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import close, get_backend, mixed_err, rel_err, summary_line
from oracle import torch_ref as R

TOL = 1e-4
LTOL = 1e-5
MARGIN = 1e-5

CLASSES = (1, 2, 3, 4, 5, 8)
SMALL = [(1, 1, 1), (2, 7, 9), (3, 17, 23), (2, 40, 44), (5, 48, 40)]
LARGE = [(5, 256, 256), (3, 300, 308)]                      # N * HW > 262144: the grid-stride loops iterate; the second has HW % 4 != 0
# (C, ignore, N, H, W)
CASES = [(c, c) + s for c in CLASSES for s in SMALL] + [(c, 4) + s for c in (5, 8) for s in SMALL]
CASES_NOLABEL = [(c, c) + s for c in CLASSES for s in SMALL]
LARGE_CASES = [(3, 3) + LARGE[0], (8, 8) + LARGE[1], (8, 4) + LARGE[0]]


def _id(c):
    if not isinstance(c, tuple):
        return str(c)
    return "C{}_ign{}_{}x{}x{}".format(*c) if len(c) == 5 else "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------ measured margins
_WORST = {}


def _note(entry, be, kind, err, what):
    rec = _WORST.setdefault((entry, be.name), {})
    if err >= rec.get(kind, (-1.0, ""))[0]:
        rec[kind] = (err, what)


def check_t(entry, be, got, ref, what):
    """a tensor: both criteria of conftest.close at 1e-4"""
    got, ref = np.asarray(got), np.asarray(ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{entry} {what}: non-finite output"
    r, m = rel_err(got, ref), mixed_err(got, ref, TOL)
    print(f"SWEEP {entry} [{be.name}] {what}: rel_err {r:.3e} mixed_err {m:.3e}")
    _note(entry, be, "rel_err", r, what)
    _note(entry, be, "mixed_err", m, what)
    assert close(got, ref, TOL), (entry, what, r, m)


def check_s(entry, be, got, ref, what):
    """a loss scalar: 1e-5 relative (rel_err of conftest, as tests/test_ops_loss.py)"""
    got, ref = float(got), float(ref)
    assert np.isfinite(got), f"{entry} {what}: {got}"
    e = rel_err(got, ref)
    print(f"SWEEP {entry} [{be.name}] {what}: {got!r} vs {ref!r} ({e:.3e})")
    _note(entry, be, "loss", e, what)
    assert e < LTOL, (entry, what, got, ref, e)


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    for (entry, name), rec in sorted(_WORST.items()):
        summary_line(f"LOSS-SWEEP {entry} [{name}]: " + "; ".join(
            f"worst {k} {v[0]:.2e} (bound {'1e-5' if k == 'loss' else ('1e-4' if k == 'rel_err' else '1')}) at {v[1]}" for k, v in sorted(rec.items())))
    _WORST.clear()


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case, salt=0):
    return np.random.default_rng([salt] + [int(v) + 1 for v in case if not isinstance(v, str)])


def logits(rng, shape, big=False):
    if not big:
        return (rng.standard_normal(shape) * 2).astype(np.float32)
    z = (rng.standard_normal(shape) * 30).astype(np.float32)
    zf = z.reshape(shape[0], shape[1], -1)
    for k in range(min(6, zf.shape[2])):                       # a few pixels at +-80: exp(-160) underflows, the max-subtracted form must not
        zf[k % shape[0], :, (k * 7919) % zf.shape[2]] = 80.0 * np.where(rng.random(shape[1]) < 0.5, -1.0, 1.0) + 0.37 * np.arange(shape[1])
        # (+ 0.37 c: classes at the same extreme do not tie exactly, so the arg-max decisions stay clear)
    return z


def labels(rng, N, H, W, C, ignore, mode="sparse"):
    if mode == "none":
        return np.full((N, H, W), ignore, np.uint8)
    if mode == "one":
        lab = np.full((N, H, W), ignore, np.uint8)
        lab.reshape(-1)[(N * H * W) // 2] = 0 if ignore != 0 else 1
        return lab
    if ignore == C:
        lab = np.full((N, H, W), C, np.uint8)
        m = rng.random((N, H, W)) < 0.25
        lab[m] = rng.integers(0, C, int(m.sum()))
    else:
        lab = rng.integers(0, C, (N, H, W)).astype(np.uint8)   # a real class is the ignored one
    lab.reshape(-1)[0] = 0
    return lab


def probs(rng, shape):
    return torch.softmax(torch.from_numpy(logits(rng, shape)), 1).numpy()


def d64(a):
    return torch.from_numpy(np.asarray(a)).double()


def lws(be, N, C, HW):
    n = be.lib.wsl_loss_ws_bytes(N, C, HW)
    return be.ws(n), n


def ce_ref(z, lab, ignore):
    return F.cross_entropy(z, torch.from_numpy(lab.astype(np.int64)), ignore_index=ignore)


def check_pseudo(entry, be, got, s1, s2, beta, what):
    """the returned label map against the float64 arg-max wherever the float64 decision is clear"""
    mix = float(np.float32(beta)) * s1 + float(np.float32(1.0 - beta)) * s2
    top = torch.topk(mix, 2, dim=1).values if mix.shape[1] > 1 else None
    clear = (top[:, 0] - top[:, 1] >= MARGIN) if top is not None else torch.ones_like(mix[:, 0], dtype=torch.bool)
    n_unclear = int((~clear).sum())
    assert n_unclear <= 1e-3 * clear.numel(), (entry, what, n_unclear, clear.numel())
    ref = torch.argmax(mix, 1)
    bad = int(((torch.from_numpy(got) != ref) & clear).sum())
    assert bad == 0, f"{entry} {what}: {bad} pseudo labels differ from the float64 arg-max at a margin >= {MARGIN}"
    assert got.min() >= 0 and got.max() < mix.shape[1]


# ------------------------------------------------------------------------------------------------ softmax / CE / argmax / pDice
def _run_softmax(be, case, big=False):
    C, _, N, H, W = case
    rng = _rng(case, 1)
    shape = (N, C, H, W)
    z, ds = logits(rng, shape, big), rng.standard_normal(shape).astype(np.float32)
    zt = d64(z).requires_grad_()
    st = torch.softmax(zt, 1)
    dz, ds_, s, dzo = be.arr(z), be.arr(ds), be.zeros(shape), be.zeros(shape)
    be.call("wsl_softmax_fwd", be.ptr(dz), be.ptr(s), N, C, H * W, be.stream)
    check_t("wsl_softmax_fwd", be, be.np(s), st, _id(case) + (" big" if big else ""))
    # backward from the kernel's own softmax, against the float64 backward
    (st * d64(ds)).sum().backward()
    be.call("wsl_softmax_bwd", be.ptr(s), be.ptr(ds_), be.ptr(dzo), N, C, H * W, be.stream)
    check_t("wsl_softmax_bwd", be, be.np(dzo), zt.grad, _id(case) + (" big" if big else ""))


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_softmax_sweep(be, case):
    _run_softmax(be, case)


def _run_ce(be, case, i64=False, mode="sparse", big=False):
    C, ignore, N, H, W = case
    rng = _rng(case, 2)
    shape, gs = (N, C, H, W), 0.7
    z, lab = logits(rng, shape, big), labels(rng, N, H, W, C, ignore, mode)
    dz_, dl = be.arr(z), be.arr(lab.astype(np.int64) if i64 else lab)
    loss, dz = be.zeros((1,)), be.arr(np.full(shape, 7.0, np.float32))
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_ce_fwd_bwd", be.ptr(dz_), be.ptr(dl), int(i64), ignore, be.ptr(loss), be.ptr(dz), gs, N, C, H * W, be.ptr(ws), n, be.stream)
    what = f"{_id(case)} i64={int(i64)} {mode}" + (" big" if big else "")
    if mode == "none":
        assert np.isnan(be.np(loss)[0]) and np.all(be.np(dz) == 0), what
        return
    zt = d64(z).requires_grad_()
    ref = ce_ref(zt, lab, ignore)
    (gs * ref).backward()
    check_s("wsl_ce_fwd_bwd", be, be.np(loss)[0], ref, what)
    check_t("wsl_ce_fwd_bwd", be, be.np(dz), zt.grad, what)


@pytest.mark.parametrize("i64", [False, True], ids=["u8", "i64"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ce_sweep(be, case, i64):
    _run_ce(be, case, i64)


@pytest.mark.parametrize("mode", ["none", "one"])
@pytest.mark.parametrize("case", [(1, 1, 2, 7, 9), (3, 3, 3, 17, 23), (4, 4, 2, 40, 44), (8, 4, 5, 48, 40)], ids=_id)
def test_ce_all_ignored_and_one_valid_pixel(be, case, mode):
    _run_ce(be, case, False, mode)
    _run_ce(be, case, True, mode)


def _run_mix_argmax(be, case):
    C, _, N, H, W = case
    rng = _rng(case, 3)
    s1, s2 = probs(rng, (N, C, H, W)), probs(rng, (N, C, H, W))
    d1, d2, out = be.arr(s1), be.arr(s2), be.zeros((N, H, W), np.int64)
    for beta in (0.37, 0.0, 1.0, 0.5):
        be.call("wsl_mix_argmax", be.ptr(d1), be.ptr(d2), beta, be.ptr(out), N, C, H * W, be.stream)
        # bit-exact with torch's float32 expression (the header's promise) ...
        assert np.array_equal(be.np(out), R.mix_argmax(torch.from_numpy(s1), torch.from_numpy(s2), beta).numpy()), (_id(case), beta)
        # ... and equal to the float64 decision wherever that is clear
        check_pseudo("wsl_mix_argmax", be, be.np(out), d64(s1), d64(s2), beta, f"{_id(case)} beta {beta}")


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_mix_argmax_sweep(be, case):
    _run_mix_argmax(be, case)


def _run_pdice(be, case, i64, dice, gout):
    """pDLoss (ignore >= 0) / DiceLoss (ignore = -1), uint8 and int64 targets, gout a device scalar or NULL"""
    C, ignore, N, H, W = case
    rng = _rng(case, 4)
    shape = (N, C, H, W)
    s = probs(rng, shape)
    tgt = rng.integers(0, C, (N, H, W)).astype(np.uint8)
    if not dice and ignore == C:
        tgt[rng.random((N, H, W)) < 0.3] = C
    ign = -1 if dice else ignore
    ds_, dt = be.arr(s), be.arr(tgt.astype(np.int64) if i64 else tgt)
    loss, sums, ds = be.zeros((1,)), be.zeros((3 * C,)), be.zeros(shape)
    go = be.arr(np.array([0.6], np.float32)) if gout else None
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_pdice_fwd", be.ptr(ds_), be.ptr(dt), int(i64), ign, be.ptr(loss), be.ptr(sums), N, C, H * W, be.ptr(ws), n, be.stream)
    be.call("wsl_pdice_bwd", be.ptr(ds_), be.ptr(dt), int(i64), ign, be.ptr(sums), be.ptr(go) if gout else None, be.ptr(ds), N, C, H * W,
            be.stream)
    st = d64(s).requires_grad_()
    t = torch.from_numpy(tgt.astype(np.int64))[:, None]
    ref = R.dice(st, t, C) if dice else R.pdice(st, t, C, ignore)
    ((0.6 if gout else 1.0) * ref).backward()
    what = f"{_id(case)} {'dice' if dice else 'pdice'} i64={int(i64)} gout={int(gout)}"
    check_s("wsl_pdice_fwd", be, be.np(loss)[0], ref, what)
    check_t("wsl_pdice_bwd", be, be.np(ds), st.grad, what)


@pytest.mark.parametrize("i64,dice,gout", [(False, False, True), (True, False, False), (False, True, False), (True, True, True)],
                         ids=["pdice_u8_gout", "pdice_i64", "dice_u8", "dice_i64_gout"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pdice_sweep(be, case, i64, dice, gout):
    _run_pdice(be, case, i64, dice, gout)


# ------------------------------------------------------------------------------------------------ the fused heads
def _run_head(be, case, dual=True, mode="sparse", with_pseudo=True, with_dz=True, big=False):
    C, ignore, N, H, W = case
    rng = _rng(case, 5)
    shape, beta, w_pse, gs = (N, C, H, W), 0.37, 0.5, 0.7
    z1, z2, lab = logits(rng, shape, big), logits(rng, shape, big), labels(rng, N, H, W, C, ignore, mode)
    d1, d2, dl = be.arr(z1), be.arr(z2), be.arr(lab)
    out, pseudo = be.zeros((4,)), be.zeros((N, H, W), np.int64)
    dz1, dz2 = be.arr(np.full(shape, 7.0, np.float32)), be.arr(np.full(shape, 7.0, np.float32))
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_head_fwd_bwd", be.ptr(d1), be.ptr(d2) if dual else None, be.ptr(dl), ignore, beta, w_pse, gs, be.ptr(out),
            be.ptr(pseudo) if (dual and with_pseudo) else None, be.ptr(dz1) if with_dz else None, be.ptr(dz2) if (dual and with_dz) else None,
            N, C, H * W, be.ptr(ws), n, be.stream)
    what = f"{_id(case)} dual={int(dual)} {mode} pseudo={int(with_pseudo)} dz={int(with_dz)}" + (" big" if big else "")
    o = be.np(out)
    t1, t2 = d64(z1).requires_grad_(), d64(z2).requires_grad_()
    s1, s2 = torch.softmax(t1, 1), torch.softmax(t2, 1)
    n_valid = int(np.sum((lab != ignore) & (lab < C)))
    assert o[3] == n_valid, what
    pse = None
    if dual:
        if with_pseudo:
            pl = be.np(pseudo)
            check_pseudo("wsl_head_fwd_bwd", be, pl, s1.detach(), s2.detach(), beta, what)
        else:                                                   # no map returned: the float64 one (its margins are asserted where it is returned)
            pl = torch.argmax(float(np.float32(beta)) * s1.detach() + float(np.float32(1.0 - beta)) * s2.detach(), 1).numpy()
        plt = torch.from_numpy(pl)[:, None]
        pse = 0.5 * (R.pdice(s1, plt, C, C) + R.pdice(s2, plt, C, C))
        check_s("wsl_head_fwd_bwd", be, o[2], pse, what + " pse")
    else:
        assert o[2] == 0.0, what
    if mode == "none":
        # every pixel ignored: loss NaN like torch, n_valid 0, the CE part of every logit gradient exactly 0
        assert np.isnan(o[0]) and np.isnan(o[1]), what
        if not with_dz:
            return
        if dual:
            (gs * w_pse * pse).backward()
            check_t("wsl_head_fwd_bwd", be, be.np(dz1), t1.grad, what + " dz1")
            check_t("wsl_head_fwd_bwd", be, be.np(dz2), t2.grad, what + " dz2")
        else:
            assert np.all(be.np(dz1) == 0), what
        return
    ce = 0.5 * (ce_ref(t1, lab, ignore) + ce_ref(t2, lab, ignore)) if dual else ce_ref(t1, lab, ignore)
    loss = ce + w_pse * pse if dual else ce
    check_s("wsl_head_fwd_bwd", be, o[0], loss, what + " loss")
    check_s("wsl_head_fwd_bwd", be, o[1], ce, what + " ce")
    if with_dz:
        (gs * loss).backward()
        check_t("wsl_head_fwd_bwd", be, be.np(dz1), t1.grad, what + " dz1")
        if dual:
            check_t("wsl_head_fwd_bwd", be, be.np(dz2), t2.grad, what + " dz2")
        else:
            assert np.all(be.np(dz2) == 7.0)                    # untouched


@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_head_sweep(be, case, dual):
    _run_head(be, case, dual)


@pytest.mark.parametrize("kw", [dict(mode="none"), dict(mode="none", dual=False), dict(mode="one"), dict(with_pseudo=False),
                                dict(with_dz=False), dict(big=True), dict(big=True, dual=False)],
                         ids=["all_ignored", "all_ignored_single", "one_valid", "no_pseudo", "no_dz", "big", "big_single"])
@pytest.mark.parametrize("case", [(2, 2, 2, 7, 9), (3, 3, 3, 17, 23), (4, 4, 2, 40, 44), (8, 4, 5, 48, 40)], ids=_id)
def test_head_edges(be, case, kw):
    _run_head(be, case, **kw)


def _run_head_gatedcrf(be, case, radius, dual=True, mode="sparse", big=False):
    C, ignore, N, H, W = case
    rng = _rng(case, 6 + radius)
    shape, beta, cw = (N, C, H, W), 0.37, 0.1
    desc = (1.0, 6.0, 0.1)                                      # weight, sigma_xy, sigma_rgb
    z1, z2, lab = logits(rng, shape, big), logits(rng, shape, big), labels(rng, N, H, W, C, ignore, mode)
    img = rng.random((N, 1, H, W)).astype(np.float32)
    img[:, :, : H // 2] = img[:, :, : H // 2] * 0.05 + 0.4      # a smooth half: many taps with k close to the maximum
    d = {k: be.arr(v) for k, v in dict(z1=z1, z2=z2, lab=lab, img=img).items()}
    out, dz1, dz2, y, msg = be.zeros((5,)), be.zeros(shape), be.zeros(shape), be.zeros(shape), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_head_gatedcrf_fwd_bwd", be.ptr(d["z1"]), be.ptr(d["z2"]) if dual else None, be.ptr(d["lab"]), ignore, beta, be.ptr(d["img"]),
            radius, desc[1], desc[2], desc[0], cw, be.ptr(out), be.ptr(dz1), be.ptr(dz2) if dual else None, be.ptr(y), be.ptr(msg), N, C, H, W,
            be.ptr(ws), n, be.stream)
    what = f"{_id(case)} r{radius} dual={int(dual)} {mode}" + (" big" if big else "")
    o = be.np(out)
    t1, t2 = d64(z1).requires_grad_(), d64(z2).requires_grad_()
    yt = R.mixprob(t1, t2 if dual else None, beta)
    crf, mref = R.gatedcrf(yt, d64(img), radius, desc[1], desc[2], desc[0])
    check_t("wsl_head_gatedcrf_fwd_bwd", be, be.np(y), yt, what + " y")
    check_t("wsl_head_gatedcrf_fwd_bwd", be, be.np(msg), mref, what + " msg")
    if C > 1:
        check_s("wsl_head_gatedcrf_fwd_bwd", be, o[4], crf, what + " crf")
    else:
        # One class: y is the constant 1, every in-image pair cancels between sum K and sum y msg, and the loss is the small remainder
        # (the kernel mass that falls outside the image) of two sums orders of magnitude larger.  A bound relative to the remainder is
        # not defined for fp32 sums; the bound is on the scale of the two sums.  The generic kernel adds the T = (2 r + 1)^2 - 1 taps of
        # a pixel in fp32 (|error| <= (T - 1) u of the sum, u = 2^-24, any order), then the 256 pixels of a workgroup in fp32 (<= 255 u),
        # then merges in fp64: each sum carries at most (T + 254) u (1 + O(u)) of itself.  (The rounding of a tap's k enters both sums
        # alike and cancels; on the out-of-image taps it is relative to the remainder: the 1e-5 term.)
        NHW = float(N * H * W)
        prod = float((mref * yt).sum())
        ksum = float(crf) * NHW + prod
        T = (2 * radius + 1) ** 2 - 1
        bound = LTOL * abs(float(crf)) + (T + 254) * 2.0 ** -24 * 1.001 * (ksum + prod) / NHW
        err = abs(float(o[4]) - float(crf))
        print(f"SWEEP wsl_head_gatedcrf_fwd_bwd [{be.name}] {what} crf (C = 1): {float(o[4])!r} vs {float(crf)!r}, |error| {err:.3e}, "
              f"bound {bound:.3e} (sums {ksum / NHW:.4g} and {prod / NHW:.4g} per pixel)")
        _note("wsl_head_gatedcrf_fwd_bwd", be, "C=1 crf error / derived bound", err / bound, what)
        assert np.isfinite(o[4]) and err <= bound, (what, float(o[4]), float(crf), err, bound)
    assert o[3] == int(np.sum((lab != ignore) & (lab < C))), what
    if dual:
        # out[2] is the (unweighted: w_pse = 0) pseudo-label Dice of the head; this entry point returns no label map, so the float64 arg-max
        # stands in wherever every pixel's decision is clear (wsl_head_fwd_bwd's cases check the map itself)
        s1, s2 = torch.softmax(t1, 1).detach(), torch.softmax(t2, 1).detach()
        mix = float(np.float32(beta)) * s1 + float(np.float32(1.0 - beta)) * s2
        top = torch.topk(mix, 2, dim=1).values if C > 1 else None
        n_unclear = int((top[:, 0] - top[:, 1] < MARGIN).sum()) if top is not None else 0
        assert n_unclear <= 1e-3 * mix[:, 0].numel(), (what, n_unclear)          # the condition check_pseudo asserts
        if n_unclear == 0:
            plt = torch.argmax(mix, 1)[:, None]
            check_s("wsl_head_gatedcrf_fwd_bwd", be, o[2], 0.5 * (R.pdice(s1, plt, C, C) + R.pdice(s2, plt, C, C)), what + " pse")
        else:                                                   # visible in the terminal summary: this case did not check out[2]
            summary_line(f"LOSS-SWEEP wsl_head_gatedcrf_fwd_bwd [{be.name}] {what}: out[2] (pse) NOT checked, {n_unclear} of "
                         f"{mix[:, 0].numel()} pixels have a float64 top-2 margin below {MARGIN}")
    else:
        assert o[2] == 0.0, what
    if mode == "none":
        assert np.isnan(o[0]) and np.isnan(o[1]), what
        (cw * crf).backward()                                   # the CE part of the gradient is exactly 0: the CRF part alone remains
    else:
        ce = 0.5 * (ce_ref(t1, lab, ignore) + ce_ref(t2, lab, ignore)) if dual else ce_ref(t1, lab, ignore)
        check_s("wsl_head_gatedcrf_fwd_bwd", be, o[0], ce, what + " loss")
        check_s("wsl_head_gatedcrf_fwd_bwd", be, o[1], ce, what + " ce")
        (ce + cw * crf).backward()
    check_t("wsl_head_gatedcrf_fwd_bwd", be, be.np(dz1), t1.grad, what + " dz1")
    if dual:
        check_t("wsl_head_gatedcrf_fwd_bwd", be, be.np(dz2), t2.grad, what + " dz2")


# the radii rotate over the cases: 5 and 2 take the 4-class fast kernel at C = 4 and W % 4 == 0, everything else the generic one
@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_head_gatedcrf_sweep(be, case, dual):
    _run_head_gatedcrf(be, case, (5, 2, 3, 1)[(CASES.index(case) + int(dual)) % 4], dual)


@pytest.mark.parametrize("kw", [dict(mode="none"), dict(mode="none", dual=False), dict(mode="one"), dict(big=True)],
                         ids=["all_ignored", "all_ignored_single", "one_valid", "big"])
@pytest.mark.parametrize("case,radius", [((3, 3, 3, 17, 23), 3), ((4, 4, 2, 40, 44), 5), ((8, 4, 2, 40, 44), 2)], ids=_id)
def test_head_gatedcrf_edges(be, case, radius, kw):
    _run_head_gatedcrf(be, case, radius, **kw)


def _reg_value(kind, s, img, C):
    return {1: lambda: R.tv_loss(s[1:]), 2: lambda: R.mumford_shah(img, s), 3: lambda: R.entropy_loss(s, C)}[kind]()


def _run_head_reg(be, case, kind, teacher, mode="sparse", big=False):
    C, ignore, N, H, W = case
    rng = _rng(case, 20 + kind)
    shape = (N, C, H, W)
    w_ce, cw = 0.8, 0.07
    rw = {1: 1.0, 2: 1.0 / (N * H * W), 3: 0.5}[kind]           # Mumford-Shah is a SUM over pixels
    z, zt, lab = logits(rng, shape, big), logits(rng, shape, big), labels(rng, N, H, W, C, ignore, mode)
    img = rng.random((N, 1, H, W)).astype(np.float32) + 0.05
    d = {k: be.arr(v) for k, v in dict(z=z, zt=zt, lab=lab, img=img).items()}
    out, dz, s, ds = be.arr(np.full((6,), 7.0, np.float32)), be.zeros(shape), be.zeros(shape), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_head_reg_fwd_bwd", be.ptr(d["z"]), be.ptr(d["lab"]), ignore, w_ce, kind, rw, be.ptr(d["img"]),
            be.ptr(d["zt"]) if teacher else None, cw, be.ptr(out), be.ptr(dz), be.ptr(s), be.ptr(ds), N, C, H, W, be.ptr(ws), n, be.stream)
    what = f"{_id(case)} kind{kind} teacher={int(teacher)} {mode}" + (" big" if big else "")
    o = be.np(out)
    t = d64(z).requires_grad_()
    st = torch.softmax(t, 1)
    check_t("wsl_head_reg_fwd_bwd", be, be.np(s), st, what + " s")
    # the regulariser's selections (arg-extrema, signs) on the softmax the kernel returned -- compared with the float64 one just above
    sk = d64(be.np(s)).requires_grad_()
    reg = _reg_value(kind, sk, d64(img), C)
    cons = torch.mean((sk - torch.softmax(d64(zt), 1)) ** 2) if teacher else None
    check_s("wsl_head_reg_fwd_bwd", be, o[4], reg, what + " reg")
    if teacher:
        check_s("wsl_head_reg_fwd_bwd", be, o[5], cons, what + " cons")
    else:
        assert o[5] == 0.0, what
    (rw * reg + (cw * cons if teacher else 0.0)).backward()
    st.backward(sk.grad, retain_graph=True)                     # ... propagated through the float64 softmax backward
    assert o[3] == int(np.sum((lab != ignore) & (lab < C))) and o[2] == 0.0, what
    if mode == "none":
        assert np.isnan(o[0]) and np.isnan(o[1]), what
    else:
        ce = ce_ref(t, lab, ignore)
        check_s("wsl_head_reg_fwd_bwd", be, o[0], ce, what + " loss")
        check_s("wsl_head_reg_fwd_bwd", be, o[1], ce, what + " ce")
        (w_ce * ce).backward()
    check_t("wsl_head_reg_fwd_bwd", be, be.np(dz), t.grad, what + " dz")


def _reg_ok(case, kind):
    C, _, N = case[:3]
    return not ((kind == 1 and N < 2) or (kind == 3 and C < 2))   # tv_loss(outputs_soft[1:]) needs N >= 2, entropy a log(C) > 0


_REG = [(1, False, "tv"), (2, True, "ms_teacher"), (3, False, "entropy"), (1, True, "tv_teacher"), (2, False, "ms"), (3, True, "entropy_teacher")]


@pytest.mark.parametrize("case,kind,teacher", [(c, k, t) for k, t, _ in _REG for c in CASES if _reg_ok(c, k)],
                         ids=[f"{n}-{_id(c)}" for k, t, n in _REG for c in CASES if _reg_ok(c, k)])
def test_head_reg_sweep(be, case, kind, teacher):
    _run_head_reg(be, case, kind, teacher)


@pytest.mark.parametrize("kw", [dict(mode="none"), dict(mode="one"), dict(big=True)], ids=["all_ignored", "one_valid", "big"])
@pytest.mark.parametrize("kind", [1, 2, 3], ids=["tv", "ms", "entropy"])
@pytest.mark.parametrize("case", [(3, 3, 3, 17, 23), (8, 4, 2, 40, 44)], ids=_id)
def test_head_reg_edges(be, case, kind, kw):
    _run_head_reg(be, case, kind, True, **kw)


# ------------------------------------------------------------------------------------------------ mixed probabilities, GatedCRF
def _run_mixprob(be, case, dual=True, big=False):
    C, _, N, H, W = case
    rng = _rng(case, 7)
    shape, beta, k = (N, C, H, W), 0.37, -0.3
    z1, z2, dy = logits(rng, shape, big), logits(rng, shape, big), rng.standard_normal(shape).astype(np.float32)
    a0, b0 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    d = {k_: be.arr(v) for k_, v in dict(z1=z1, z2=z2, dy=dy).items()}
    p2 = be.ptr(d["z2"]) if dual else None
    y = be.zeros(shape)
    be.call("wsl_mixprob_fwd", be.ptr(d["z1"]), p2, beta, be.ptr(y), N, C, H * W, be.stream)
    t1, t2 = d64(z1).requires_grad_(), d64(z2).requires_grad_()
    yt = R.mixprob(t1, t2 if dual else None, beta)
    what = f"{_id(case)} dual={int(dual)}" + (" big" if big else "")
    check_t("wsl_mixprob_fwd", be, be.np(y), yt, what)
    (k * (yt * d64(dy)).sum()).backward()
    for acc in (0, 1):                                          # overwrite, then accumulate onto a non-zero tensor
        g1, g2 = be.arr(a0), be.arr(b0)
        be.call("wsl_mixprob_bwd", be.ptr(d["z1"]), p2, beta, be.ptr(d["dy"]), k, be.ptr(g1), be.ptr(g2) if dual else None, acc, N, C, H * W,
                be.stream)
        check_t("wsl_mixprob_bwd", be, be.np(g1), t1.grad + (d64(a0) if acc else 0.0), what + f" acc={acc} dz1")
        if dual:
            check_t("wsl_mixprob_bwd", be, be.np(g2), t2.grad + (d64(b0) if acc else 0.0), what + f" acc={acc} dz2")


@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_mixprob_sweep(be, case, dual):
    _run_mixprob(be, case, dual)


def _run_gatedcrf(be, case, radius, gout):
    """y does NOT sum to one over the classes (nothing may assume a softmax)"""
    C, _, N, H, W = case
    rng = _rng(case, 8 + radius)
    shape, gs = (N, C, H, W), 0.7
    w, sxy, srgb = (0.7, 4.0, 0.25) if radius == 3 else (1.0, 6.0, 0.1)
    y = (rng.random(shape) * 1.5).astype(np.float32)
    img = rng.random((N, 1, H, W)).astype(np.float32)
    img[:, :, : H // 2] = img[:, :, : H // 2] * 0.05 + 0.4
    dy_, di = be.arr(y), be.arr(img)
    msg, loss, dy = be.zeros(shape), be.zeros((1,)), be.zeros(shape)
    go = be.arr(np.array([0.6], np.float32)) if gout else None
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_gatedcrf_fwd", be.ptr(dy_), be.ptr(di), be.ptr(msg), be.ptr(loss), N, C, H, W, radius, sxy, srgb, w, be.ptr(ws), n, be.stream)
    be.call("wsl_gatedcrf_bwd", be.ptr(msg), be.ptr(go) if gout else None, gs, be.ptr(dy), N, C, H, W, be.stream)
    yt = d64(y).requires_grad_()
    ref, mref = R.gatedcrf(yt, d64(img), radius, sxy, srgb, w)
    (gs * (0.6 if gout else 1.0) * ref).backward()
    what = f"{_id(case)} r{radius} gout={int(gout)}"
    check_t("wsl_gatedcrf_fwd", be, be.np(msg), mref, what + " msg")
    check_s("wsl_gatedcrf_fwd", be, be.np(loss)[0], ref, what)
    check_t("wsl_gatedcrf_bwd", be, be.np(dy), yt.grad, what)


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_gatedcrf_sweep(be, case):
    i = CASES_NOLABEL.index(case)
    _run_gatedcrf(be, case, (5, 2, 3, 1, 8)[i % 5], gout=bool(i % 2))


# ------------------------------------------------------------------------------------------------ regularisers on probabilities
def _run_tv(be, case, n0):
    C, _, N, H, W = case
    rng = _rng(case, 9)
    shape, gs = (N, C, H, W), 0.7
    p = probs(rng, shape)
    dp_, loss, dp = be.arr(p), be.zeros((1,)), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_tv_fwd_bwd", be.ptr(dp_), n0, be.ptr(loss), be.ptr(dp), gs, N, C, H, W, be.ptr(ws), n, be.stream)
    pt = d64(p).requires_grad_()
    ref = R.tv_loss(pt[n0:])
    (gs * ref).backward()
    check_s("wsl_tv_fwd_bwd", be, be.np(loss)[0], ref, f"{_id(case)} n0={n0}")
    check_t("wsl_tv_fwd_bwd", be, be.np(dp), pt.grad, f"{_id(case)} n0={n0}")


@pytest.mark.parametrize("case,n0", [(c, n0) for n0 in (0, 1) for c in CASES_NOLABEL if n0 < c[2]],       # tv_loss(p[1:]) needs N >= 2
                         ids=[f"n0={n0}-{_id(c)}" for n0 in (0, 1) for c in CASES_NOLABEL if n0 < c[2]])
def test_tv_sweep(be, case, n0):
    _run_tv(be, case, n0)


def _run_ms(be, case):
    C, _, N, H, W = case
    rng = _rng(case, 10)
    shape, gs = (N, C, H, W), 0.7
    p, img = probs(rng, shape), rng.random((N, 1, H, W)).astype(np.float32) + 0.05
    di, dp_, loss, dp = be.arr(img), be.arr(p), be.zeros((1,)), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_mumford_shah_fwd_bwd", be.ptr(di), be.ptr(dp_), be.ptr(loss), be.ptr(dp), gs, N, C, H, W, be.ptr(ws), n, be.stream)
    pt = d64(p).requires_grad_()
    ref = R.mumford_shah(d64(img), pt)
    (gs * ref).backward()
    check_s("wsl_mumford_shah_fwd_bwd", be, be.np(loss)[0], ref, _id(case))
    if H * W == 1:
        # one pixel: the centroid IS the pixel, the gradient is identically zero and no relative criterion is defined against it.  fp32 forms
        # the centroid as fl(fl(p I) / I) = p (1 + e1)(1 + e2), |e| <= u = 2^-24, so |p - centroid| <= 2 u |p| (+ O(u^2)) and the gradient
        # 2 (p - centroid) I gscale is at most 4 u |p| I gscale in magnitude (times 1 + 2 u for the two products)
        assert not pt.grad.any()
        bound = 4.0 * 2.0 ** -24 * float(np.abs(p).max()) * float(img.max()) * gs * (1 + 1e-6)
        assert np.abs(be.np(dp)).max() <= bound, (np.abs(be.np(dp)).max(), bound)
        return
    check_t("wsl_mumford_shah_fwd_bwd", be, be.np(dp), pt.grad, _id(case))


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_mumford_shah_sweep(be, case):
    _run_ms(be, case)


def _run_mse(be, case, big=False):
    C, _, N, H, W = case
    rng = _rng(case, 11)
    shape, gs = (N, C, H, W), 0.7
    a, b = logits(rng, shape, big), logits(rng, shape, big)
    da_, db_, loss, da = be.arr(a), be.arr(b), be.zeros((1,)), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_softmax_mse_fwd_bwd", be.ptr(da_), be.ptr(db_), be.ptr(loss), be.ptr(da), gs, N, C, H * W, be.ptr(ws), n, be.stream)
    at = d64(a).requires_grad_()
    ref = torch.mean(R.softmax_mse(at, d64(b)))
    (gs * ref).backward()
    what = _id(case) + (" big" if big else "")
    check_s("wsl_softmax_mse_fwd_bwd", be, be.np(loss)[0], ref, what)
    check_t("wsl_softmax_mse_fwd_bwd", be, be.np(da), at.grad, what)


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_softmax_mse_sweep(be, case):
    _run_mse(be, case)


def _run_entropy(be, case, big=False, norm=None):
    C, _, N, H, W = case
    rng = _rng(case, 12)
    shape, gs = (N, C, H, W), 0.7
    norm = norm or C
    # big: the softmax of large logits -- probabilities that are exactly 0 and exactly 1
    p = torch.softmax(torch.from_numpy(logits(rng, shape, True)), 1).numpy() if big else probs(rng, shape)
    if big:
        assert (p == 0).any() or C == 1
    dp_, loss, dp = be.arr(p), be.zeros((1,)), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_entropy_fwd_bwd", be.ptr(dp_), be.ptr(loss), be.ptr(dp), gs, N, C, H * W, norm, be.ptr(ws), n, be.stream)
    pt = d64(p).requires_grad_()
    ref = R.entropy_loss(pt, norm)
    (gs * ref).backward()
    what = f"{_id(case)} norm={norm}" + (" big" if big else "")
    check_s("wsl_entropy_fwd_bwd", be, be.np(loss)[0], ref, what)
    check_t("wsl_entropy_fwd_bwd", be, be.np(dp), pt.grad, what)


# (C = 1 is not a case: p is the constant 1 and the loss is -log(1 + 1e-6) / log(norm), whose fp32 value is the rounding of 1 + 1e-6 to
#  1 + 2^-20 -- 5 % off in ANY fp32 evaluation, torch's included; probabilities that are exactly 1 occur in the large-logit cases)
@pytest.mark.parametrize("case", [c for c in CASES_NOLABEL if c[0] > 1], ids=_id)
def test_entropy_sweep(be, case):
    _run_entropy(be, case)


# ------------------------------------------------------------------------------------------------ uncertainty-aware mean teacher
def _run_softmax_accum(be, case, big=False):
    C, _, N, H, W = case
    rng = _rng(case, 13)
    shape, T = (N, C, H, W), 8
    zs = [logits(rng, shape, big) for _ in range(T)]
    acc = be.arr(np.full(shape, np.nan, np.float32))            # init = 1 must overwrite, not accumulate
    for i, z in enumerate(zs):
        dz = be.arr(z)
        be.call("wsl_softmax_accum", be.ptr(dz), be.ptr(acc), 1.0 / T, int(i == 0), N, C, H * W, be.stream)
        if i == 0:
            assert not np.isnan(be.np(acc)).any(), "init = 1 left a NaN of the old buffer"
            check_t("wsl_softmax_accum", be, be.np(acc), torch.softmax(d64(z), 1) / T, _id(case) + " init")
    ref = torch.stack([torch.softmax(d64(z), 1) for z in zs]).mean(0)
    check_t("wsl_softmax_accum", be, be.np(acc), ref, _id(case) + f" T={T}" + (" big" if big else ""))


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_softmax_accum_sweep(be, case):
    _run_softmax_accum(be, case)


def bimodal_pmean(rng, shape, big=False):
    """about half the pixels sharply peaked (uncertainty ~ 0.03), half near uniform (uncertainty ~ log C): the certainty threshold goes
    between the modes.  big: the peaked half holds probabilities that are exactly 0 and 1."""
    N, C, H, W = shape
    peaked = rng.random((N, 1, H, W)) < 0.5
    z = rng.standard_normal(shape) * 0.05
    cls = rng.integers(0, C, (N, 1, H, W))
    z = np.where(peaked & (np.arange(C).reshape(1, C, 1, 1) == cls), z + (200.0 if big else 8.0), z)
    return torch.softmax(torch.from_numpy(z.astype(np.float32)), 1).numpy()


def _run_ustm(be, case, big=False):
    C, _, N, H, W = case
    rng = _rng(case, 14)
    shape, gs = (N, C, H, W), 0.7
    a, b, pm = logits(rng, shape, big), logits(rng, shape, big), bimodal_pmean(rng, shape, big)
    unc = -(d64(pm) * torch.log(d64(pm) + 1e-6)).sum(1, keepdim=True)
    thr = 0.5 * float(np.log(C)) if C > 1 else 0.5 * float(unc.min() + unc.max()) + 0.01
    assert float((unc - thr).abs().min()) > 1e-3, "a pixel's uncertainty lies on the threshold: the mask is not decided"
    d = {k: be.arr(v) for k, v in dict(a=a, b=b, pm=pm).items()}
    loss, da = be.zeros((3,)), be.zeros(shape)
    ws, n = lws(be, N, C, H * W)
    be.call("wsl_ustm_consistency_fwd_bwd", be.ptr(d["a"]), be.ptr(d["b"]), be.ptr(d["pm"]), thr, be.ptr(loss), be.ptr(da), gs, N, C, H * W,
            be.ptr(ws), n, be.stream)
    at = d64(a).requires_grad_()
    ref, cnt = R.ustm_consistency(at, d64(b), d64(pm), thr)
    (gs * ref).backward()
    what = _id(case) + (" big" if big else "")
    o = be.np(loss)
    assert o[1] == float(cnt), (what, o[1], float(cnt))          # the mask count, exactly
    check_s("wsl_ustm_consistency_fwd_bwd", be, o[0], ref, what)
    check_s("wsl_ustm_consistency_fwd_bwd", be, o[2], 1.0 / (2.0 * float(cnt) + 1e-16) if cnt > 0 else o[2], what + " factor")
    check_t("wsl_ustm_consistency_fwd_bwd", be, be.np(da), at.grad, what)


@pytest.mark.parametrize("case", CASES_NOLABEL, ids=_id)
def test_ustm_consistency_sweep(be, case):
    _run_ustm(be, case)


@pytest.mark.parametrize("k", [-1, 0, 1, 2, 3, 5])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 9), (2, 40, 44), (5, 33, 70), (1, 1, 50), (2, 50, 1)], ids=_id)
def test_rot90_non_square_bit_exact(be, shape, k):
    """planes of H * W below and above one 1024-element block, several planes, every k the engine can pass -- bit-exact against
    torch.rot90, and rot90(rot90(x, k), 4 - k) == x (what the engine relies on for the gradient)"""
    planes, H, W = shape
    x = np.random.default_rng(H * W + k + 10).standard_normal(shape).astype(np.float32)
    ref = torch.rot90(torch.from_numpy(x), k, [1, 2]).contiguous().numpy()
    dx, y, back = be.arr(x), be.arr(np.full(ref.shape, np.nan, np.float32)), be.arr(np.full(shape, np.nan, np.float32))
    be.call("wsl_rot90", be.ptr(dx), be.ptr(y), planes, H, W, k, be.stream)
    assert np.array_equal(be.np(y).view(np.uint32), ref.view(np.uint32)), (shape, k)
    Ho, Wo = ref.shape[1:]
    be.call("wsl_rot90", be.ptr(y), be.ptr(back), planes, Ho, Wo, 4 - k, be.stream)
    assert np.array_equal(be.np(back).view(np.uint32), x.view(np.uint32)), (shape, k)


@pytest.mark.parametrize("n", [1, 3, 1023, 1024, 1025, 4099, 40 * 44 * 8 + 1])
def test_axpy_sweep(be, n):
    rng = np.random.default_rng(n)
    dst, src, k = rng.standard_normal(n + 2).astype(np.float32), rng.standard_normal(n + 2).astype(np.float32), -0.37
    dd, ds = be.arr(dst), be.arr(src)
    be.call("wsl_axpy", be.ptr(dd) + 4, be.ptr(ds) + 4, k, n, be.stream)               # (an unaligned start, the ends untouched)
    got = be.np(dd)
    assert got[0] == dst[0] and got[-1] == dst[-1]
    check_t("wsl_axpy", be, got[1:-1], d64(dst)[1:-1] + float(np.float32(k)) * d64(src)[1:-1], f"n={n}")


# ------------------------------------------------------------------------------------------------ large logits
@pytest.mark.parametrize("case", [(3, 3, 3, 17, 23), (4, 4, 2, 40, 44), (8, 8, 2, 40, 44)], ids=_id)
def test_large_logits_do_not_overflow(be, case):
    """z = 30 * randn with a few pixels at +-80: every softmax-bearing entry point stays finite and within tolerance of float64 (the
    heads' cases are in test_head_edges / test_head_gatedcrf_edges / test_head_reg_edges); entropy and USTM see probabilities that are
    exactly 0"""
    _run_softmax(be, case, big=True)
    _run_ce(be, case, big=True)
    _run_mixprob(be, case, True, big=True)
    _run_mse(be, case, big=True)
    _run_softmax_accum(be, case, big=True)
    _run_entropy(be, case, big=True)
    _run_ustm(be, case, big=True)


# ------------------------------------------------------------------------------------------------ GPU-only sizes
_LARGE_RUNS = {
    "softmax": lambda be, c: _run_softmax(be, c),
    "ce_u8": lambda be, c: _run_ce(be, c, False),
    "ce_i64": lambda be, c: _run_ce(be, c, True),
    "mix_argmax": lambda be, c: _run_mix_argmax(be, c),
    "pdice": lambda be, c: _run_pdice(be, c, False, False, True),
    "head_dual": lambda be, c: _run_head(be, c, True),
    "head_single": lambda be, c: _run_head(be, c, False),
    "head_gatedcrf_dual": lambda be, c: _run_head_gatedcrf(be, c, 2, True),          # (radius 2: the float64 reference runs on the host)
    "head_gatedcrf_single": lambda be, c: _run_head_gatedcrf(be, c, 2, False),
    "head_reg_tv": lambda be, c: _run_head_reg(be, c, 1, True),
    "head_reg_ms": lambda be, c: _run_head_reg(be, c, 2, False),
    "head_reg_entropy": lambda be, c: _run_head_reg(be, c, 3, False),
    "mixprob": lambda be, c: _run_mixprob(be, c, True),
    "gatedcrf": lambda be, c: _run_gatedcrf(be, c, 2, True),
    "tv": lambda be, c: _run_tv(be, c, 1),
    "mumford_shah": lambda be, c: _run_ms(be, c),
    "softmax_mse": lambda be, c: _run_mse(be, c),
    "entropy": lambda be, c: _run_entropy(be, c),
    "softmax_accum": lambda be, c: _run_softmax_accum(be, c),
    "ustm": lambda be, c: _run_ustm(be, c),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE_CASES, ids=_id)
@pytest.mark.parametrize("entry", list(_LARGE_RUNS))
def test_grid_stride_sizes_gpu(entry, case):
    """N * HW > 1024 workgroups * 256 threads: every pixel kernel's grid-stride loop runs more than once"""
    _LARGE_RUNS[entry](get_backend("hip"), case)


@pytest.mark.gpu
@pytest.mark.parametrize("i64,dice", [(False, False), (True, False), (True, True)], ids=["pdice_u8", "pdice_i64", "dice_i64"])
@pytest.mark.parametrize("C", [3, 8])
def test_pdice_grid_stride_size_gpu(C, i64, dice):
    """the pDice kernels grid over HW alone: their stride loop needs HW > 262144"""
    _run_pdice(get_backend("hip"), (C, C, 2, 520, 512), i64, dice, True)


@pytest.mark.gpu
@pytest.mark.parametrize("C,radius,dual", [(4, 5, True), (3, 5, False), (8, 3, True), (4, 2, False)])
def test_gatedcrf_radius5_mid_size_gpu(C, radius, dual):
    """(2, 96, 264): interior and border workgroups of both CRF kernels at the radii the trainers use, standalone and fused"""
    be = get_backend("hip")
    _run_gatedcrf(be, (C, C, 2, 96, 264), radius, True)
    _run_head_gatedcrf(be, (C, C, 2, 96, 264), radius, dual)
