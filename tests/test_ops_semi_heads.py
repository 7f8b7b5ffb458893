"""wsl_sup_head_fwd_bwd and wsl_entropy_logits_fwd_bwd (include/wsl_hip.h, csrc/wsl_semi.hip) through the C ABI against float64.

Reference: float64 torch on the EXACT float32 inputs -- F.cross_entropy(ignore_index), the lines of DiceLoss (utils/losses.py:156-192:
one-hot over range(C), 1 - (2 I + 1e-5) / (Z + Y + 1e-5) averaged over the classes) and of entropy_loss (utils/losses.py:30-36) restated, with
autograd for dz.  Criteria: those of tests/test_ops_loss_sweep.py -- tensors close(., ., 1e-4) (both criteria of conftest.py), loss scalars
1e-5 relative.  The fused heads are also compared with the chains of existing entry points they replace, the no-valid-pixel convention
with wsl_head_fwd_bwd.

Sizes: C in 1 .. 8 (one instantiation each), N in {1, 3}, HW in {1, 63, 64, 65, 24 * 20, 2052, 2053}: HW % 4 == 0 takes the 128-bit form, the rest
the one-pixel-per-lane form; a workgroup walks chunks of 2048 pixels, which 2053 crosses by 5 pixels and 2052 by one group of four (N = 3
crosses two more boundaries inside samples).  The worst measured errors reach the terminal summary (recorded in profiles/semi_margins.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import close, mixed_err, rel_err, summary_line
from test_workspace_guards import filled, guard_check, untouched

TOL, LTOL = 1e-4, 1e-5
EINVAL = -1
HWS = (1, 63, 64, 65, 24 * 20, 2052, 2053)
CASES = [(c, n) for c in range(1, 9) for n in (1, 3)]

_WORST = {}


def _note(entry, be, kind, err, what):
    rec = _WORST.setdefault((entry, be.name), {})
    if err >= rec.get(kind, (-1.0, ""))[0]:
        rec[kind] = (err, what)


def check_t(entry, be, got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (entry, what)
    r, m = rel_err(got, ref), mixed_err(got, ref, TOL)
    _note(entry, be, "rel_err", r, what)
    _note(entry, be, "mixed_err", m, what)
    assert close(got, ref, TOL), (entry, what, r, m)


def check_s(entry, be, got, ref, what):
    got, ref = float(got), float(ref.detach() if isinstance(ref, torch.Tensor) else ref)
    assert np.isfinite(got), (entry, what, got)
    e = rel_err(got, ref)
    _note(entry, be, "loss", e, what)
    assert e < LTOL, (entry, what, got, ref, e)


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    for (entry, name), rec in sorted(_WORST.items()):
        summary_line(f"SEMI-HEADS {entry} [{name}]: " + "; ".join(
            f"worst {k} {v[0]:.2e} (bound {'1e-5' if k == 'loss' else ('1e-4' if k == 'rel_err' else '1')}) at {v[1]}" for k, v in sorted(rec.items())))
    _WORST.clear()


# ------------------------------------------------------------------------------------------------ inputs and the float64 reference
def _inputs(C, N, HW, salt=0, sharp=None, absent=None, all_ignored=False):
    rng = np.random.default_rng([salt, C, N, HW])
    if sharp is None:
        z = (2.0 * rng.standard_normal((N, C, HW)) + np.arange(C).reshape(1, -1, 1)).astype(np.float32)
    else:
        z = (sharp * np.where(rng.random((N, C, HW)) < 0.5, -1.0, 1.0)).astype(np.float32)
    ignore = C                                            # the ignore value: one past the classes, as 4 is for the four ACDC classes
    lab = rng.integers(0, C, (N, HW)).astype(np.uint8)
    if absent is not None:
        lab[lab == absent] = (absent + 1) % C
    lab[rng.random((N, HW)) < 0.25] = ignore
    lab.reshape(-1)[0] = 0                                 # at least one valid pixel
    if all_ignored:
        lab[:] = ignore
    return z, lab, ignore


def ref_sup(z, lab, ignore, w_ce, w_dice, gscale):
    """(loss, ce, dice, n_valid, dz) in float64: CrossEntropyLoss(ignore_index) + DiceLoss(C) of losses.py:156-192 restated"""
    C = z.shape[1]
    zd = torch.from_numpy(z).double().requires_grad_()
    t = torch.from_numpy(lab).long()
    ce = F.cross_entropy(zd, t, ignore_index=ignore)
    s = torch.softmax(zd, 1)
    dice = 0.0
    for c in range(C):                                     # _one_hot_encoder over range(C): an ignored label is zero in every class
        tc = (t == c).double()
        sc = s[:, c]
        dice = dice + (1 - (2 * torch.sum(sc * tc) + 1e-5) / (torch.sum(sc * sc) + torch.sum(tc * tc) + 1e-5))
    dice = dice / C
    n_valid = int((t != ignore).sum())
    # float32-rounded weights, as the entry point receives them
    w_ce, w_dice, gscale = float(np.float32(w_ce)), float(np.float32(w_dice)), float(np.float32(gscale))
    loss = (w_ce * ce if n_valid else 0.0) + w_dice * dice       # (no valid pixel: CE is NaN and its gradient 0 -- the Dice part remains)
    (gscale * loss).backward()
    return (w_ce * ce + w_dice * dice), ce, dice, n_valid, zd.grad


def ref_ent(z, norm, gscale):
    zd = torch.from_numpy(z).double().requires_grad_()
    p = torch.softmax(zd, 1)
    loss = torch.mean(-1 * torch.sum(p * torch.log(p + 1e-6), dim=1) / torch.tensor(np.log(norm)))     # losses.py:30-36
    (float(np.float32(gscale)) * loss).backward()
    return loss, zd.grad


def lws(be, N, C, HW):
    n = be.lib.wsl_loss_ws_bytes(N, C, HW)
    return be.ws(n), n


def run_sup(be, z, lab, ignore, w_ce, w_dice, gscale, ws=None, n=None, out=None, dz=None):
    N, C, HW = z.shape
    if ws is None:
        wsb, n = lws(be, N, C, HW)
        ws = be.ptr(wsb)
    dzd, ld = be.arr(z), be.arr(lab)
    out = be.arr(np.full(4, 7.0, np.float32)) if out is None else out
    dz = be.arr(np.full(z.shape, 7.0, np.float32)) if dz is None else dz
    be.call("wsl_sup_head_fwd_bwd", be.ptr(dzd), be.ptr(ld), ignore, w_ce, w_dice, gscale, be.ptr(out), be.ptr(dz), N, C, HW, ws, n, be.stream)
    be.sync()
    return be.np(out).copy(), be.np(dz).copy()


def run_ent(be, z, norm, gscale, ws=None, n=None, out=None, dz=None):
    N, C, HW = z.shape
    if ws is None:
        wsb, n = lws(be, N, C, HW)
        ws = be.ptr(wsb)
    zd = be.arr(z)
    out = be.arr(np.full(1, 7.0, np.float32)) if out is None else out
    dz = be.arr(np.full(z.shape, 7.0, np.float32)) if dz is None else dz
    be.call("wsl_entropy_logits_fwd_bwd", be.ptr(zd), be.ptr(out), be.ptr(dz), gscale, N, C, HW, norm, ws, n, be.stream)
    be.sync()
    return be.np(out).copy(), be.np(dz).copy()


def chain_sup(be, z, lab, ignore, w_ce, w_dice):
    """what loss='ce_dice' launches today: head (w_ce * CE), softmax, DiceLoss forward / backward, softmax backward, axpy"""
    N, C, HW = z.shape
    zd, ld = be.arr(z), be.arr(lab)
    out, dz, s, ds, dzx = be.arr(np.zeros(8, np.float32)), be.zeros(z.shape), be.zeros(z.shape), be.zeros(z.shape), be.zeros(z.shape)
    sums, gout, dice = be.zeros((3 * C,)), be.arr(np.full(1, w_dice, np.float32)), be.zeros((1,))
    ws, n = lws(be, N, C, HW)
    be.call("wsl_head_fwd_bwd", be.ptr(zd), None, be.ptr(ld), ignore, 0.0, 0.0, w_ce, be.ptr(out), None, be.ptr(dz), None, N, C, HW, be.ptr(ws), n, be.stream)
    be.call("wsl_softmax_fwd", be.ptr(zd), be.ptr(s), N, C, HW, be.stream)
    be.call("wsl_pdice_fwd", be.ptr(s), be.ptr(ld), 0, -1, be.ptr(dice), be.ptr(sums), N, C, HW, be.ptr(ws), n, be.stream)
    be.call("wsl_pdice_bwd", be.ptr(s), be.ptr(ld), 0, -1, be.ptr(sums), be.ptr(gout), be.ptr(ds), N, C, HW, be.stream)
    be.call("wsl_softmax_bwd", be.ptr(s), be.ptr(ds), be.ptr(dzx), N, C, HW, be.stream)
    be.call("wsl_axpy", be.ptr(dz), be.ptr(dzx), 1.0, N * C * HW, be.stream)
    be.sync()
    o = be.np(out)
    return float(o[1]), float(be.np(dice)[0]), float(o[3]), be.np(dz).copy()


def chain_ent(be, z, norm, gscale):
    N, C, HW = z.shape
    zd = be.arr(z)
    out, dz, s, ds = be.zeros((1,)), be.zeros(z.shape), be.zeros(z.shape), be.zeros(z.shape)
    ws, n = lws(be, N, C, HW)
    be.call("wsl_softmax_fwd", be.ptr(zd), be.ptr(s), N, C, HW, be.stream)
    be.call("wsl_entropy_fwd_bwd", be.ptr(s), be.ptr(out), be.ptr(ds), gscale, N, C, HW, norm, be.ptr(ws), n, be.stream)
    be.call("wsl_softmax_bwd", be.ptr(s), be.ptr(ds), be.ptr(dz), N, C, HW, be.stream)
    be.sync()
    return float(be.np(out)[0]), be.np(dz).copy()


def _check_sup(be, z, lab, ignore, what, w_ce=0.5, w_dice=0.5, gscale=1.0):
    o, dz = run_sup(be, z, lab, ignore, w_ce, w_dice, gscale)
    loss, ce, dice, n_valid, g = ref_sup(z, lab, ignore, w_ce, w_dice, gscale)
    e = "wsl_sup_head_fwd_bwd"
    check_s(e, be, o[0], loss, what + " loss")
    check_s(e, be, o[1], ce, what + " ce")
    check_s(e, be, o[2], dice, what + " dice")
    assert o[3] == n_valid, (what, o[3], n_valid)
    check_t(e, be, dz, g, what + " dz")
    return o, dz


def _check_ent(be, z, norm, what, gscale=1.0):
    o, dz = run_ent(be, z, norm, gscale)
    loss, g = ref_ent(z, norm, gscale)
    e = "wsl_entropy_logits_fwd_bwd"
    check_s(e, be, o[0], loss, what + " loss")
    check_t(e, be, dz, g, what + " dz")
    return o, dz


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("case", CASES, ids=lambda c: "C{}_N{}".format(*c))
def test_sup_head_against_float64(be, case):
    C, N = case
    for HW in HWS:
        z, lab, ignore = _inputs(C, N, HW, salt=1)
        _check_sup(be, z, lab, ignore, f"C{C} N{N} HW{HW}")
    z, lab, ignore = _inputs(C, N, 65, salt=2)
    _check_sup(be, z, lab, ignore, f"C{C} N{N} HW65 weights", w_ce=0.3, w_dice=0.9, gscale=0.37)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "C{}_N{}".format(*c))
def test_entropy_head_against_float64(be, case):
    C, N = case
    for HW in HWS:
        z, _, _ = _inputs(C, N, HW, salt=3)
        _check_ent(be, z, 4, f"C{C} N{N} HW{HW}")
    z, _, _ = _inputs(C, N, 65, salt=4)
    _check_ent(be, z, max(C, 2), f"C{C} N{N} HW65 norm/gscale", gscale=0.1)


@pytest.mark.parametrize("HW", [63, 64])
def test_saturated_logits_stay_finite(be, HW):
    """logits of +-80: exp(-160) underflows, a confident pixel's entropy term is -log(1 + 1e-6); every output stays finite and still meets
    the float64 reference"""
    for C in (2, 4, 8):
        z, lab, ignore = _inputs(C, 3, HW, salt=5, sharp=80.0)
        o, dz = _check_sup(be, z, lab, ignore, f"+-80 C{C} HW{HW}")
        assert np.all(np.isfinite(o)) and np.all(np.isfinite(dz))
        # the entropy gradient of a saturated pixel is ZERO to 1e-19 (p is one-hot, or uniform over the classes tied at +80), so there is no
        # reference scale for close(): the value is checked as usual, the gradient against what float32 can cancel -- dz_c = k p_c (e_c -
        # sum_j e_j p_j) with |e| <= |log 1e-6| + 1 < 14.9 and the sum over C terms rounded to 2^-23 each: |dz - ref| <= k * C * 2^-23 * 14.9
        o, dz = run_ent(be, z, 4, 1.0)
        loss, g = ref_ent(z, 4, 1.0)
        assert np.all(np.isfinite(o)) and np.all(np.isfinite(dz))
        check_s("wsl_entropy_logits_fwd_bwd", be, o[0], loss, f"+-80 C{C} HW{HW} loss")
        bound = 1.0 / (3 * HW * np.log(4.0)) * C * 2.0 ** -23 * 14.9
        err = float(np.max(np.abs(dz - g.numpy())))
        _note("wsl_entropy_logits_fwd_bwd", be, "saturated dz abs err / bound", err / bound, f"+-80 C{C} HW{HW}")
        assert err <= bound, (C, HW, err, bound)


def test_a_class_absent_from_the_labels(be):
    """Y_c = I_c = 0 for the absent class: its Dice term is 1 - 1e-5 / (Z_c + 1e-5), gradient through Z_c alone"""
    for HW in (65, 24 * 20):
        z, lab, ignore = _inputs(4, 3, HW, salt=6, absent=2)
        assert not np.any(lab == 2)
        _check_sup(be, z, lab, ignore, f"class 2 absent HW{HW}")


# ------------------------------------------------------------------------------------------------ against the chains they replace
@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_fused_heads_against_the_chains(be, C):
    """(C = 1 is left to the float64 sweeps above: softmax is 1 there and the chain's wsl_entropy_fwd_bwd forms 1 + 1e-6 in float32, whose
    rounding is 5 % of the whole -log(1 + 1e-6) term; the fused head takes log p from the logits and meets float64)"""
    for N, HW in ((3, 65), (1, 24 * 20), (3, 2053)):
        z, lab, ignore = _inputs(C, N, HW, salt=7)
        o, dz = run_sup(be, z, lab, ignore, 0.5, 0.5, 1.0)
        ce, dice, n_valid, dzc = chain_sup(be, z, lab, ignore, 0.5, 0.5)
        assert rel_err([o[1], o[2], o[0]], [ce, dice, 0.5 * (ce + dice)]) < LTOL and o[3] == n_valid
        assert close(dz, dzc, TOL), (C, N, HW, rel_err(dz, dzc), mixed_err(dz, dzc, TOL))
        oe, dze = run_ent(be, z, 4, 0.1)
        le, dzec = chain_ent(be, z, 4, 0.1)
        assert rel_err(oe[0], le) < LTOL, (oe, le)
        assert close(dze, dzec, TOL), (C, N, HW, rel_err(dze, dzec), mixed_err(dze, dzec, TOL))


def test_no_valid_pixel_follows_the_head(be):
    """every label ignored: ce (and the loss) NaN, n_valid 0, the CE gradient exactly 0 -- what wsl_head_fwd_bwd writes for that batch;
    the Dice part stays finite and keeps its gradient"""
    for HW in (63, 64):
        z, lab, ignore = _inputs(4, 2, HW, salt=8, all_ignored=True)
        N, C = 2, 4
        zd, ld = be.arr(z), be.arr(lab)
        out, dzh = be.arr(np.full(4, 7.0, np.float32)), be.arr(np.full(z.shape, 7.0, np.float32))
        ws, n = lws(be, N, C, HW)
        be.call("wsl_head_fwd_bwd", be.ptr(zd), None, be.ptr(ld), ignore, 0.0, 0.0, 0.5, be.ptr(out), None, be.ptr(dzh), None, N, C, HW, be.ptr(ws), n, be.stream)
        be.sync()
        oh, dzh = be.np(out).copy(), be.np(dzh).copy()
        assert np.isnan(oh[1]) and oh[3] == 0 and not np.any(dzh)
        o, dz = run_sup(be, z, lab, ignore, 0.5, 0.0, 1.0)            # CE alone: the head's numbers
        assert np.isnan(o[0]) and np.isnan(o[1]) and o[3] == oh[3] and np.array_equal(dz, dzh)
        o, dz = run_sup(be, z, lab, ignore, 0.5, 0.5, 1.0)
        _, _, dice, _, g = ref_sup(z, lab, ignore, 0.5, 0.5, 1.0)
        assert np.isnan(o[0]) and np.isnan(o[1]) and o[3] == 0
        check_s("wsl_sup_head_fwd_bwd", be, o[2], dice, f"all ignored HW{HW} dice")
        check_t("wsl_sup_head_fwd_bwd", be, dz, g, f"all ignored HW{HW} dz")


# ------------------------------------------------------------------------------------------------ refusals, workspace, reproducibility
def test_nine_classes_are_refused_with_nothing_written(be):
    from wsl4mis_amd import _lib
    N, C, HW = 2, 9, 64
    z, lab = be.arr(np.zeros((N, C, HW), np.float32)), be.arr(np.zeros((N, HW), np.uint8))
    ws = filled(be, (be.lib.wsl_loss_ws_bytes(N, 8, HW) // 4 + 64,))
    out, dz = filled(be, (4,)), filled(be, (N, C, HW))
    with pytest.raises(_lib.WslError, match="-> -1:"):
        be.call("wsl_sup_head_fwd_bwd", be.ptr(z), be.ptr(lab), 9, 0.5, 0.5, 1.0, be.ptr(out), be.ptr(dz), N, C, HW, be.ptr(ws), 4 * int(np.prod(be.shape(ws))), be.stream)
    with pytest.raises(_lib.WslError, match="-> -1:"):
        be.call("wsl_entropy_logits_fwd_bwd", be.ptr(z), be.ptr(out), be.ptr(dz), 1.0, N, C, HW, 4, be.ptr(ws), 4 * int(np.prod(be.shape(ws))), be.stream)
    with pytest.raises(_lib.WslError, match="-> -1:"):                 # log(1) = 0 normaliser
        be.call("wsl_entropy_logits_fwd_bwd", be.ptr(z), be.ptr(out), be.ptr(dz), 1.0, N, 4, HW, 1, be.ptr(ws), 4 * int(np.prod(be.shape(ws))), be.stream)
    be.sync()
    assert untouched(be, out) and untouched(be, dz) and untouched(be, ws)


@pytest.mark.parametrize("shape", [(3, 4, 65), (1, 8, 2052), (2, 1, 24 * 20)], ids=lambda s: "x".join(map(str, s)))
def test_workspace_of_exactly_the_queried_size(be, shape):
    """guard words around a workspace of wsl_loss_ws_bytes(): nothing in front, nothing behind, the same bits with slack, and
    WSL_EWORKSPACE with nothing written when it is one byte short"""
    N, C, HW = shape
    z, lab, ignore = _inputs(C, N, HW, salt=9)
    nbytes = be.lib.wsl_loss_ws_bytes(N, C, HW)
    guard_check(be, nbytes, lambda: [filled(be, (4,)), filled(be, z.shape)],
                lambda ws, n, outs: run_sup(be, z, lab, ignore, 0.5, 0.5, 1.0, ws=ws, n=n, out=outs[0], dz=outs[1]))
    guard_check(be, nbytes, lambda: [filled(be, (1,)), filled(be, z.shape)],
                lambda ws, n, outs: run_ent(be, z, 4, 0.1, ws=ws, n=n, out=outs[0], dz=outs[1]))


def test_two_runs_are_bit_identical(be):
    for N, C, HW in ((3, 4, 2053), (3, 4, 2052), (1, 7, 65)):
        z, lab, ignore = _inputs(C, N, HW, salt=10)
        a, b = run_sup(be, z, lab, ignore, 0.5, 0.5, 1.0), run_sup(be, z, lab, ignore, 0.5, 0.5, 1.0)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        a, b = run_ent(be, z, 4, 0.1), run_ent(be, z, 4, 0.1)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
