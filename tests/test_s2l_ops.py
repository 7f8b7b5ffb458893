"""The three Scribble2Label entry points of the C ABI (csrc/wsl_s2l.hip) against the reference's own results (fixtures g13_s2l_*,
tests/golden/make_golden_s2l.py), a float64 restatement and scipy:

  wsl_augment_batch_s2l    bit for bit equal to RandomGenerator_s2l in all four arrays, same draws from both generators
  wsl_s2l_head_fwd_bwd     pseudo labels and both counts exact (the fp32 threshold compare at float32(thr) and one ulp either side,
                           the highest qualifying class, the NaN of a CE without valid pixels), losses and dz by close() at 1e-4;
                           class counts 2, 3, 4, 8 against float64; guard words around exactly the queried workspace
  wsl_s2l_ensemble_update  two successive updates against the reference's lines by close(); its index map EXACTLY against
                           scipy.ndimage.zoom(order=0), read out of the store through saturated logits with alpha = 1"""
import os
import random

import numpy as np
import pytest
from scipy.ndimage import zoom

from conftest import GOLDEN, close, get_backend, golden, rel_err
from test_workspace_guards import filled, guard_check
from wsl4mis_amd import _lib
from wsl4mis_amd.dataloaders import h5lite

TOL = 1e-4
ACDC = os.path.join(GOLDEN, "acdc", "ACDC_training_slices")


def weight_map(h, w, seed):
    """the fixture's random [h, w, 4] store, rebuilt from its seed (make_golden_s2l.py::weight_map)"""
    return (np.random.default_rng([seed, 13]).integers(0, 256, (h, w, 4)).astype(np.float32) / np.float32(255)).astype(np.float32)


# ================================================================================================ augmentation
def aug_call(be, img, mask, scr, w, p, size):
    from wsl4mis_amd.dataloaders.dataset import _rotate_matrix
    d = {k: be.arr(v) for k, v in dict(img=img.astype(np.float32), mask=mask.astype(np.uint8), scr=scr.astype(np.uint8), w=w).items()}
    s = _lib.WslAugSampleS2l()
    s.img, s.mask, s.scr, s.weight, s.h, s.w = be.ptr(d["img"]), be.ptr(d["mask"]), be.ptr(d["scr"]), be.ptr(d["w"]), img.shape[0], img.shape[1]
    s.op, s.k, s.axis = p["op"], p.get("k", 0), p.get("axis", 0)
    if p["op"] == 2:
        m, off = _rotate_matrix(p["angle"], img.shape)
        s.m00, s.m01, s.m10, s.m11, s.off0, s.off1 = m[0, 0], m[0, 1], m[1, 0], m[1, 1], off[0], off[1]
    Ho, Wo = size
    o = [be.zeros((1, 1, Ho, Wo)), be.zeros((1, Ho, Wo), np.uint8), be.zeros((1, Ho, Wo), np.uint8), be.zeros((1, Ho, Wo, w.shape[2]))]
    arr = (_lib.WslAugSampleS2l * 1)(s)
    be.call("wsl_augment_batch_s2l", arr, 1, w.shape[2], be.ptr(o[0]), be.ptr(o[1]), be.ptr(o[2]), be.ptr(o[3]), Ho, Wo, be.stream)
    be.sync()
    return [be.np(a)[0] for a in o]


def test_augmentation_equals_the_reference_bit_for_bit(be):
    from wsl4mis_amd.dataloaders.dataset_s2l import _draw
    g = golden("g13_s2l_aug")
    seen = set()
    for i in range(int(g["meta_n"])):
        t = f"c{i:02d}"
        with h5lite.File(os.path.join(ACDC, str(g["meta_files"][int(g[f"{t}_file"])]))) as f:
            img, mask, scr = f["image"][:], f["label"][:], f["scribble"][:]
        seed, size = int(g[f"{t}_seed"]), tuple(int(v) for v in g[f"{t}_size"])
        if be.name == "emul" and size[0] * size[1] > 64 * 48 and i % 2:
            continue                                            # (one of the two 256 x 256 cases is enough for the host emulator)
        random.seed(seed), np.random.seed(seed)
        p = _draw()
        # the draw order, by the decisions taken and by the state of both generators afterwards
        assert [p["op"]] + [p[k] for k in ("k", "axis", "angle") if k in p] == [int(v) for v in g[f"{t}_draw"]], (t, p)
        assert [random.random(), float(np.random.randint(0, 1 << 30))] == list(g[f"{t}_next"]), t
        seen.add((p["op"], p.get("k"), p.get("axis"), p.get("angle")))
        oi, om, osc, ow = aug_call(be, img, mask, scr, weight_map(img.shape[0], img.shape[1], seed), p, size)
        assert np.array_equal(oi[0].view(np.uint32), g[f"{t}_image"][0].view(np.uint32)), t
        assert np.array_equal(om, g[f"{t}_mask"]) and np.array_equal(osc, g[f"{t}_scribble"]), t
        assert np.array_equal(ow.view(np.uint32), g[f"{t}_weight"].view(np.uint32)), t
    assert {(1, k, a, None) for k in range(4) for a in range(2)} <= seen and (0, None, None, None) in seen
    assert len({s[3] for s in seen if s[0] == 2}) >= 5


def test_augmentation_without_mask_and_in_chunks(be):
    """mask NULL, C = 3 (the scalar weight gather), 40 samples (two descriptor tables): against numpy's own index maps (op 0 and 1)"""
    rng = np.random.default_rng(5)
    n, C_, Ho, Wo = 40, 3, 16, 12
    keep, arr, exp = [], (_lib.WslAugSampleS2l * n)(), []
    for i in range(n):
        h, w = int(rng.integers(9, 30)), int(rng.integers(9, 30))
        img, scr, wt = rng.random((h, w), dtype=np.float32), rng.integers(0, 5, (h, w)).astype(np.uint8), rng.random((h, w, C_), dtype=np.float32)
        d = [be.arr(img), be.arr(scr), be.arr(wt)]
        keep.append(d)
        s = arr[i]
        s.img, s.mask, s.scr, s.weight, s.h, s.w = be.ptr(d[0]), None, be.ptr(d[1]), be.ptr(d[2]), h, w
        s.op, s.k, s.axis = i % 2, i % 4, (i // 4) % 2
        f = (lambda a: np.flip(np.rot90(a, s.k), axis=s.axis)) if s.op else (lambda a: a)
        exp.append([zoom(f(a), (Ho / f(a).shape[0], Wo / f(a).shape[1]) + (1,) * (a.ndim - 2), order=0) for a in (img, scr, wt)])
    o = [be.zeros((n, 1, Ho, Wo)), be.zeros((n, Ho, Wo), np.uint8), be.zeros((n, Ho, Wo, C_))]
    be.call("wsl_augment_batch_s2l", arr, n, C_, be.ptr(o[0]), None, be.ptr(o[1]), be.ptr(o[2]), Ho, Wo, be.stream)
    be.sync()
    for i in range(n):
        assert np.array_equal(be.np(o[0])[i, 0], exp[i][0]) and np.array_equal(be.np(o[1])[i], exp[i][1]), i
        assert np.array_equal(be.np(o[2])[i], exp[i][2]), i


# ================================================================================================ loss head
def head_call(be, z, scr, w, thr, w_u=0.5, ignore=4, gscale=1.0, want_u=True, want_dz=True):
    N, C_, H, W = z.shape
    d = [be.arr(z), be.arr(scr), be.arr(w)]
    out, u, dz = be.zeros((8,)), be.zeros((N, H, W), np.uint8), be.zeros(z.shape)
    n = be.lib.wsl_s2l_head_ws_bytes(N, C_, H * W)
    ws = be.ws(n)
    be.call("wsl_s2l_head_fwd_bwd", be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), ignore, thr, w_u, gscale, be.ptr(out),
            be.ptr(u) if want_u else None, be.ptr(dz) if want_dz else None, N, C_, H * W, be.ptr(ws), n, be.stream)
    be.sync()
    return be.np(out)[:5].copy(), be.np(u).copy(), be.np(dz).copy()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_head_matches_the_reference(be, tag):
    """a: thr 0.8 with weights planted at float32(0.8) and one ulp either side; b: thr 0.3, two classes over the threshold (the highest
    wins); c: no confident pixel -- the second CE and the loss are NaN, the gradient of the scribble CE is still there"""
    g = golden("g13_s2l_head")
    out, u, dz = head_call(be, g[f"{tag}_z"], g[f"{tag}_scribble"], g[f"{tag}_weight"], float(g[f"{tag}_thr"]))
    assert np.array_equal(u, g[f"{tag}_u"])
    assert [int(out[3]), int(out[4])] == [int(v) for v in g[f"{tag}_counts"]]
    ref = g[f"{tag}_losses"]
    if tag == "c":
        assert np.isnan(ref[0]) and np.isnan(ref[2])
        assert np.isnan(out[0]) and np.isnan(out[2]) and close(out[1], ref[1], TOL)
    else:
        assert close(out[:3], ref, TOL), (out, ref)
    assert np.all(np.isfinite(dz)) and close(dz, g[f"{tag}_dz"], TOL), rel_err(dz, g[f"{tag}_dz"])


def test_head_threshold_compare_is_fp32(be):
    """float32(0.8) > 0.8 is False in torch (the scalar is rounded to the tensor's type); a compare in double would say True"""
    g = golden("g13_s2l_head")
    w, u = g["a_weight"], g["a_u"]
    t32 = np.float32(0.8)
    assert float(t32) > 0.8
    assert w[0, 0, 0, 1] == t32 and u[0, 0, 0] == 4                       # at the threshold: not confident
    assert w[0, 0, 1, 2] == np.nextafter(t32, np.float32(1)) and u[0, 0, 1] == 2      # one ulp above
    assert w[0, 0, 2, 3] == np.nextafter(t32, np.float32(0)) and u[0, 0, 2] == 4      # one ulp below
    _, got, _ = head_call(be, g["a_z"], g["a_scribble"], w, 0.8, want_dz=False)
    assert [int(v) for v in got[0, 0, :5]] == [4, 2, 4, 0, 4]


def head_f64(z, scr, w, thr, w_u, ignore):
    N, C_, H, W = z.shape
    zd = z.astype(np.float64)
    m = zd.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(zd - m).sum(1))
    s = np.exp(zd - lse[:, None])
    conf = (w > np.float32(thr)) & (scr == ignore)[..., None]            # decided on the fp32 values, like the kernel and torch
    u = np.full((N, H, W), ignore, np.int64)
    for c in range(C_):
        u[conf[..., c]] = c
    res, dz = [], np.zeros_like(zd)
    for lab, k in ((scr.astype(np.int64), 1.0), (u, w_u)):
        valid = (lab != ignore) & (lab < C_)
        n = int(valid.sum())
        oh = (np.arange(C_)[None, :, None, None] == np.where(valid, lab, -1)[:, None]).astype(np.float64)
        nll = (lse - (zd * oh).sum(1))[valid].sum()
        res += [nll / n if n else np.nan, n]
        if n:
            dz += k * (s - oh) * valid[:, None] / n
    return np.array([res[0] + w_u * res[2], res[0], res[2], res[1], res[3]]), u.astype(np.uint8), dz


SWEEP = [(2, 2, 7, 9), (3, 3, 17, 23), (4, 2, 40, 44), (4, 3, 7, 9), (8, 2, 24, 20), (8, 1, 1, 1), (4, 1, 1, 4)]
SWEEP_GPU = [(4, 5, 256, 256), (3, 3, 300, 308), (4, 2, 301, 303)]      # grid-stride loops iterate; the last: C = 4 on the scalar path


def _sweep_case(be, case):
    C_, N, H, W = case
    rng = np.random.default_rng(list(case))
    ignore = C_ if C_ != 8 else 4                                          # C = 8: a real class is the ignore index
    z = (rng.standard_normal((N, C_, H, W)) * 2).astype(np.float32)
    scr = np.full((N, H, W), ignore, np.uint8)
    m = rng.random((N, H, W)) < 0.2
    scr[m] = rng.integers(0, C_, int(m.sum()))
    scr.reshape(-1)[0] = 0 if ignore != 0 else 1
    w = rng.random((N, H, W, C_)).astype(np.float32)
    w.reshape(-1, C_)[-1] = 0.99                                           # at least one confident pixel (every class qualifies) ...
    scr.reshape(-1)[-1] = ignore if N * H * W > 1 else scr.reshape(-1)[-1]    # ... unless the only pixel is the scribble's
    thr, w_u = 0.45, 0.5
    ref, u_ref, dz_ref = head_f64(z, scr, w, thr, w_u, ignore)
    out, u, dz = head_call(be, z, scr, w, thr, w_u, ignore, gscale=0.5)
    assert np.array_equal(u, u_ref) and [int(out[3]), int(out[4])] == [int(ref[3]), int(ref[4])], case
    for k in range(3):
        if np.isnan(ref[k]):
            assert np.isnan(out[k]), (case, k, out, ref)
        else:
            assert rel_err(out[k], ref[k]) < 1e-5, (case, k, out, ref)
    assert close(dz, 0.5 * dz_ref, TOL), (case, rel_err(dz, 0.5 * dz_ref))


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "C{}_{}x{}x{}".format(*c))
def test_head_class_count_sweep_against_float64(be, case):
    _sweep_case(be, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SWEEP_GPU, ids=lambda c: "C{}_{}x{}x{}".format(*c))
def test_head_large_sizes_against_float64_gpu(case):
    _sweep_case(get_backend("hip"), case)


def test_head_is_bit_reproducible(be):
    g = golden("g13_s2l_head")
    a = head_call(be, g["b_z"], g["b_scribble"], g["b_weight"], 0.3)
    b = head_call(be, g["b_z"], g["b_scribble"], g["b_weight"], 0.3)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", [(2, 4, 40, 44), (3, 3, 17, 23), (1, 4, 7, 9), (1, 4, 1, 700), (1, 8, 600, 3), (1, 4, 1, 1)],
                         ids=lambda s: "-".join(str(v) for v in s))
def test_head_stays_inside_its_workspace(be, shape):
    N, C_, H, W = shape
    rng = np.random.default_rng(H * 7 + W + C_)
    z = be.arr((rng.standard_normal(shape) * 2).astype(np.float32))
    scr = np.full((N, H, W), C_, np.uint8)
    scr[rng.random((N, H, W)) < 0.2] = 0
    scr.reshape(-1)[0] = 0
    scr, w = be.arr(scr), be.arr(rng.random((N, H, W, C_)).astype(np.float32))
    P = be.ptr
    guard_check(be, be.lib.wsl_s2l_head_ws_bytes(N, C_, H * W), lambda: [filled(be, (8,)), filled(be, (N, H, W), np.uint8), filled(be, shape)],
                lambda ws, n, o: be.call("wsl_s2l_head_fwd_bwd", P(z), P(scr), P(w), C_, 0.5, 0.5, 1.0, P(o[0]), P(o[1]), P(o[2]), N, C_,
                                         H * W, ws, n, be.stream))


# ================================================================================================ ensemble update
def update_call(be, z, stores, alpha):
    n, C_, Hn, Wn = z.shape
    slots = (_lib.WslS2lSlot * n)()
    for i, s in enumerate(stores):
        slots[i].weight, slots[i].h, slots[i].w = be.ptr(s), be.shape(s)[0], be.shape(s)[1]
    zd = be.arr(z)
    be.call("wsl_s2l_ensemble_update", be.ptr(zd), slots, n, C_, Hn, Wn, alpha, be.stream)
    be.sync()


def test_update_matches_the_reference(be):
    g = golden("g13_s2l_update")
    sizes = [tuple(int(v) for v in s) for s in g["meta_sizes"]]
    stores = [be.zeros(s + (4,)) for s in sizes]
    for r in range(2):
        update_call(be, g[f"z{r}"], stores, float(g["meta_alpha"]))
        for i, s in enumerate(stores):
            assert close(be.np(s), g[f"w{r}_{i}"], TOL), (r, i, rel_err(be.np(s), g[f"w{r}_{i}"]))


def test_update_ema_arithmetic_is_contraction_free_fp32(be):
    """alpha * pred + (1 - alpha) * weight with alpha and 1 - alpha (subtracted in double) rounded to fp32, two multiplies and an add:
    with saturated logits pred is exactly 1 on one class, so the expected store is exact"""
    alpha = 0.2
    a, oma = np.float32(alpha), np.float32(1.0 - alpha)
    rng = np.random.default_rng(3)
    old = rng.random((9, 7, 4)).astype(np.float32)
    hot = rng.integers(0, 4, (1, 8, 8))
    z = np.where(np.arange(4)[None, :, None, None] == hot[:, None], 40.0, -40.0).astype(np.float32)
    st = be.arr(old)
    update_call(be, z, [st], alpha)
    src = zoom(hot[0], (9 / 8, 7 / 8), order=0)
    pred = (np.arange(4)[None, None, :] == src[..., None]).astype(np.float32)
    exp = (a * pred).astype(np.float32) + (oma * old).astype(np.float32)
    got = be.np(st)
    on = pred == 1
    assert np.array_equal(got[on].view(np.uint32), exp[on].view(np.uint32))
    assert np.max(np.abs(got[~on] - (oma * old)[~on])) <= 1e-30                # pred = exp(-80) there, not 0


def index_map_through_the_store(be, Hn, Wn, sizes):
    """1 + the source pixel index of every native pixel (0: scipy's fill -- no class is hot there), two bits per call: class = bits
    (2k, 2k+1) of the index, alpha = 1"""
    idx = np.arange(Hn * Wn).reshape(Hn, Wn)
    got = [np.zeros(s, np.int64) for s in sizes]
    fill = [None] * len(sizes)
    stores = [be.zeros(s + (4,)) for s in sizes]
    for k in range(0, max(1, int(np.ceil(np.log2(Hn * Wn)))), 2):
        hot = (idx >> k) & 3
        z = np.where(np.arange(4)[:, None, None] == hot[None], 40.0, -40.0).astype(np.float32)
        update_call(be, np.broadcast_to(z, (len(sizes),) + z.shape).copy(), stores, 1.0)
        for i, s in enumerate(stores):
            w = be.np(s)
            nhot = (w > 0.5).sum(-1)
            assert np.all(nhot <= 1) and np.all(w[nhot == 0] == 0)          # a fill pixel is exactly 0 in every class
            assert fill[i] is None or np.array_equal(fill[i], nhot == 0)
            fill[i] = nhot == 0
            got[i] |= np.argmax(w, -1).astype(np.int64) << k
    return [np.where(f, 0, g + 1) for f, g in zip(fill, got)]


def check_index_map(be, Hn, Wn, sizes):
    """scipy.ndimage.zoom(order=0) exactly, its mode='constant' fill included: for some (in, out) the last coordinate (out - 1) *
    ((in - 1) / (out - 1)) lands one ulp above in - 1 and scipy writes cval = 0 into the last row / column (33 <- 32 is one)"""
    got = index_map_through_the_store(be, Hn, Wn, sizes)
    for (h, w), gi in zip(sizes, got):
        ref = zoom(np.arange(1, Hn * Wn + 1, dtype=np.float64).reshape(Hn, Wn), (h / Hn, w / Wn), order=0)
        assert ref.shape == (h, w)
        assert np.array_equal(gi, ref.astype(np.int64)), (h, w, int((gi != ref).sum()))


def test_update_index_map_is_scipy_zoom_order0(be):
    check_index_map(be, 32, 32, [(45, 38), (20, 25), (50, 17), (32, 32), (33, 31), (2, 64)])
    check_index_map(be, 16, 24, [(31, 9), (16, 24), (7, 50)])


@pytest.mark.gpu
def test_update_index_map_at_the_acdc_sizes_gpu():
    be = get_backend("hip")
    check_index_map(be, 256, 256, [(100, 430), (216, 256), (430, 100), (300, 301), (256, 256), (154, 154), (428, 512)])


def test_update_generic_class_count_and_many_slices(be):
    """C = 3 (scalar store path) and 70 slices (two slot tables) against the float64 softmax"""
    rng = np.random.default_rng(8)
    n, C_, Hn, Wn, alpha = 70, 3, 8, 8, 0.3
    z = (rng.standard_normal((n, C_, Hn, Wn)) * 2).astype(np.float32)
    sizes = [(int(rng.integers(3, 14)), int(rng.integers(3, 14))) for _ in range(n)]
    old = [rng.random(s + (C_,)).astype(np.float32) for s in sizes]
    stores = [be.arr(o) for o in old]
    update_call(be, z, stores, alpha)
    e = np.exp(z.astype(np.float64) - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    for i, (h, w) in enumerate(sizes):
        pz = zoom(p[i], (1, h / Hn, w / Wn), order=0).transpose(1, 2, 0)
        assert close(be.np(stores[i]), alpha * pz + (1 - alpha) * old[i], TOL), i


# ================================================================================================ arguments
def test_bad_arguments_return_einval(be):
    z, scr, w = be.zeros((1, 4, 4, 4)), be.zeros((1, 4, 4), np.uint8), be.zeros((1, 4, 4, 4))
    out, dz = be.zeros((8,)), be.zeros((1, 4, 4, 4))
    n = be.lib.wsl_s2l_head_ws_bytes(1, 4, 16)
    ws = be.ws(n)
    P = be.ptr

    def head(zp=P(z), sp=P(scr), wp=P(w), ignore=4, C_=4, HW=16, N=1):
        return be.lib.wsl_s2l_head_fwd_bwd(zp, sp, wp, ignore, 0.8, 0.5, 1.0, P(out), None, P(dz), N, C_, HW, P(ws), n, be.stream)

    assert head() == 0
    for kw in (dict(zp=None), dict(sp=None), dict(wp=None), dict(C_=9), dict(C_=0), dict(HW=0), dict(N=0), dict(ignore=-1), dict(ignore=300)):
        assert head(**kw) == -1, kw                                            # WSL_EINVAL
    assert b"s2l_head_fwd_bwd" in be.lib.wsl_last_error()
    assert be.lib.wsl_s2l_head_ws_bytes(0, 4, 16) == 0
    st = be.zeros((5, 5, 4))
    slot = (_lib.WslS2lSlot * 1)()
    slot[0].weight, slot[0].h, slot[0].w = P(st), 5, 5
    upd = lambda zp=P(z), sl=slot, n_=1, C_=4, Hn=4: be.lib.wsl_s2l_ensemble_update(zp, sl, n_, C_, Hn, 4, 0.2, be.stream)  # noqa: E731
    assert upd() == 0
    bad = (_lib.WslS2lSlot * 1)()
    bad[0].weight, bad[0].h, bad[0].w = P(st), 0, 5
    null = (_lib.WslS2lSlot * 1)()
    null[0].h, null[0].w = 5, 5
    for kw in (dict(zp=None), dict(sl=None), dict(n_=0), dict(C_=9), dict(Hn=0), dict(sl=bad), dict(sl=null)):
        assert upd(**kw) == -1, kw
    s = (_lib.WslAugSampleS2l * 1)()
    img, sc = be.zeros((5, 5)), be.zeros((5, 5), np.uint8)
    s[0].img, s[0].scr, s[0].weight, s[0].h, s[0].w = P(img), P(sc), P(st), 5, 5
    o = [be.zeros((1, 1, 4, 4)), be.zeros((1, 4, 4), np.uint8), be.zeros((1, 4, 4, 4))]
    aug = lambda sm=s, C_=4, oi=P(o[0]), Ho=4: be.lib.wsl_augment_batch_s2l(sm, 1, C_, oi, None, P(o[1]), P(o[2]), Ho, 4, be.stream)  # noqa: E731
    assert aug() == 0
    s3 = (_lib.WslAugSampleS2l * 1)()
    s3[0].img, s3[0].scr, s3[0].weight, s3[0].h, s3[0].w, s3[0].op = P(img), P(sc), P(st), 5, 5, 3
    s4 = (_lib.WslAugSampleS2l * 1)()
    s4[0].img, s4[0].scr, s4[0].h, s4[0].w = P(img), P(sc), 5, 5
    for kw in (dict(sm=None), dict(C_=9), dict(oi=None), dict(Ho=0), dict(sm=s3), dict(sm=s4)):
        assert aug(**kw) == -1, kw
    be.sync()
