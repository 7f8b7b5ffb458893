"""The two kernel families of on-device validation at the C ABI (csrc/wsl_val.hip), against scipy / numpy restated here:
  wsl_val_zoom_in    == scipy.ndimage.zoom(slice, (Ho / h, Wo / w), order=0), bit for bit, scipy's fill of the last row / column included
  wsl_val_labelmap   == zoom(np.argmax(z, 1).astype(np.uint8)[k], (h / Hn, w / Wn), order=0), and the per-(group, class) counts
                        |pred == c|, |label == c|, |pred == c & label == c| == np.count_nonzero
Every comparison is exact: the index rule is integer-valued and the counts are integers."""
import numpy as np
import pytest
from scipy.ndimage import zoom

from wsl4mis_amd import _lib

GUARD = 0xAB


def _zoom_in(be, imgs, Ho, Wo):
    dev = [be.arr(a, np.float32) for a in imgs]
    n = len(imgs)
    src = (_lib.WslValSrc * n)()
    for k, (a, d) in enumerate(zip(imgs, dev)):
        src[k].img, src[k].h, src[k].w = be.ptr(d), a.shape[0], a.shape[1]
    out = be.arr(np.full((n, 1, Ho, Wo), -7.0, np.float32))
    be.call("wsl_val_zoom_in", src, n, be.ptr(out), Ho, Wo, be.stream)
    be.sync()
    return be.np(out)


# (Ho, Wo) of the call -> the native sizes mixed in it; the FIRST is the pair the issue lists, with what scipy does there
ZOOM_IN = [
    ((8, 16), [(30, 32), (9, 11)], "fill"),       # scipy fills the last row and the last column
    ((12, 20), [(26, 22), (7, 33)], "fill"),
    ((16, 16), [(20, 27), (5, 7)], "edge"),       # edge pixel kept on both axes; (5, 7): upsampling
    ((7, 10), [(13, 9), (30, 32)], None),         # a width that is no multiple of 4: the one-sample-per-lane kernel
]


@pytest.mark.parametrize("target,sizes,kind", ZOOM_IN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_zoom_in_equals_scipy_bit_for_bit(be, target, sizes, kind):
    rng = np.random.default_rng(11)
    Ho, Wo = target
    n = 70                                                        # more than one table of 64
    imgs = [(1.0 + rng.random(sizes[k % len(sizes)])).astype(np.float32) for k in range(n)]      # >= 1: a fill of 0 is visible
    ref = [zoom(a, (Ho / a.shape[0], Wo / a.shape[1]), order=0) for a in imgs]
    assert all(r.shape == (Ho, Wo) for r in ref)
    first = ref[0]
    if kind == "fill":                                            # ... so the fill rule cannot go untested silently
        assert (first[-1] == 0).all() and (first[:, -1] == 0).all() and (first[:-1, :-1] >= 1).all()
    if kind == "edge":
        assert np.array_equal(first[-1, -1], imgs[0][-1, -1]) and (first >= 1).all()
        assert (ref[1] >= 1).all() and ref[1].shape > imgs[1].shape                    # the upsampled one
    got = _zoom_in(be, imgs, Ho, Wo)
    for k in range(n):
        assert np.array_equal(got[k, 0].view(np.uint32), ref[k].view(np.uint32)), (k, imgs[k].shape)


def _packed(shapes, lead=5):
    """byte offsets of slices packed into one buffer behind `lead` guard bytes, with 0 / 1 / 2 guard bytes between them: every
    alignment of a start and of an end occurs"""
    offs, o = [], lead
    for k, (h, w) in enumerate(shapes):
        offs.append(o)
        o += h * w + k % 3
    return offs, o + 7


def _labelmap(be, z, shapes, labels=None, groups=None, counts=None, n_groups=0, buf=None):
    """-> (list of predictions, the whole buffer): the slices packed by _packed into a buffer of guard bytes"""
    n, C_, Hn, Wn = z.shape
    offs, total = _packed(shapes)
    buf = be.arr(np.full((total,), GUARD, np.uint8)) if buf is None else buf
    zd = be.arr(z, np.float32)
    labs = [None if labels is None or labels[k] is None else be.arr(labels[k], np.uint8) for k in range(n)]
    dst = (_lib.WslValDst * n)()
    for k, (h, w) in enumerate(shapes):
        dst[k].pred, dst[k].h, dst[k].w = be.ptr(buf) + offs[k], h, w
        dst[k].label = None if labs[k] is None else be.ptr(labs[k])
        dst[k].group = 0 if groups is None else groups[k]
    be.call("wsl_val_labelmap", be.ptr(zd), dst, n, C_, Hn, Wn, None if counts is None else be.ptr(counts), n_groups, be.stream)
    be.sync()
    raw = be.np(buf)
    return [raw[o:o + h * w].reshape(h, w) for o, (h, w) in zip(offs, shapes)], raw


def _guards_intact(raw, shapes):
    offs, total = _packed(shapes)
    keep = np.ones(total, bool)
    for o, (h, w) in zip(offs, shapes):
        keep[o:o + h * w] = False
    return bool((raw[keep] == GUARD).all()) and int(keep.sum()) >= 12


def _ref_labelmap(z, shapes):
    lab = np.argmax(z, 1).astype(np.uint8)
    out = [zoom(lab[k], (h / z.shape[2], w / z.shape[3]), order=0) for k, (h, w) in enumerate(shapes)]
    assert all(o.shape == s for o, s in zip(out, shapes))
    return out


def _tied_logits(rng, shape):
    """three logit values only: most pixels have their maximum in two classes or in all of them"""
    z = rng.integers(0, 3, shape).astype(np.float32)
    z[:, :, ::5, ::3] = 1.0                                       # ... and a lattice where every class is equal
    return z


# (Hn, Wn) of the logits -> native sizes mixed in the call (the issue's pairs; (15, 13): an odd h * w), fill or not, slices
LABELMAP = [
    ((16, 32), [(30, 31)], True, 5),
    ((8, 15), [(26, 26)], True, 5),
    ((32, 22), [(16, 39)], True, 5),
    ((16, 16), [(20, 24), (16, 16), (15, 13)], False, 66),        # no fill; more than one table
]


@pytest.mark.parametrize("C_", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("net,sizes,fill,n", LABELMAP, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_labelmap_equals_zoom_of_argmax(be, C_, net, sizes, fill, n):
    rng = np.random.default_rng(100 + C_)
    Hn, Wn = net
    shapes = [sizes[k % len(sizes)] for k in range(n)]
    z = _tied_logits(rng, (n, C_, Hn, Wn))
    if C_ > 1:
        srt = np.sort(z.reshape(n, C_, -1), axis=1)
        assert (srt[:, -1] == srt[:, -2]).mean() > 0.2 and (srt[:, -1] == srt[:, 0]).any()      # ties in two classes / in all
    for h, w in sizes:                                            # the fill occurs where the table says, and only there
        ones = zoom(np.ones((Hn, Wn), np.uint8), (h / Hn, w / Wn), order=0)
        assert bool((ones == 0).any()) == fill, (net, h, w)
    ref = _ref_labelmap(z, shapes)
    got, raw = _labelmap(be, z, shapes)
    for k in range(n):
        assert np.array_equal(got[k], ref[k]), (k, shapes[k])
    assert _guards_intact(raw, shapes)


def _ref_counts(preds, labels, groups, n_groups, C_):
    cnt = np.zeros((n_groups, C_, 3), np.int64)
    for p, l, g in zip(preds, labels, groups):
        if l is None:
            continue
        for c in range(C_):
            cnt[g, c] += (np.count_nonzero(p == c), np.count_nonzero(l == c), np.count_nonzero((p == c) & (l == c)))
    return cnt


@pytest.mark.parametrize("C_", [3, 4])                            # the generic and the 4-class instantiation
def test_counts_equal_count_nonzero(be, C_):
    rng = np.random.default_rng(5 + C_)
    Hn, Wn = 16, 16
    shapes = [(33, 47), (20, 24), (33, 47), (15, 13), (20, 24), (33, 47), (15, 13)]      # (33, 47): two workgroups per slice
    groups = [0, 1, 1, 1, 1, 2, 2]                                # three groups, uneven
    n = len(shapes)
    z = _tied_logits(rng, (n, C_, Hn, Wn))
    labels = [rng.integers(0, C_ + 1, s).astype(np.uint8) for s in shapes]                # the value C counts nowhere
    assert any((l == C_).any() for l in labels)
    ref_pred = _ref_labelmap(z, shapes)
    ref = _ref_counts(ref_pred, labels, groups, 3, C_)
    assert (ref[:, :, 2] > 0).any() and ref[:, :, 1].sum() < sum(h * w for h, w in shapes)
    counts = be.zeros((3, C_, 3), np.int64)
    got, raw = _labelmap(be, z, shapes, labels, groups, counts, 3)
    first = be.np(counts).copy()
    assert np.array_equal(first, ref)
    assert all(np.array_equal(g, r) for g, r in zip(got, ref_pred)) and _guards_intact(raw, shapes)
    # a second call ADDS; a slice without a label counts nowhere
    labels2 = [None if k in (1, 5) else l for k, l in enumerate(labels)]
    _labelmap(be, z, shapes, labels2, groups, counts, 3)
    assert np.array_equal(be.np(counts), ref + _ref_counts(ref_pred, labels2, groups, 3, C_))
    # counts = NULL (labels given) and label = NULL: predictions only
    got3, raw3 = _labelmap(be, z, shapes, labels, groups, None, 0)
    assert raw3.tobytes() == raw.tobytes()
    # two runs: identical bytes
    again = be.zeros((3, C_, 3), np.int64)
    _, raw4 = _labelmap(be, z, shapes, labels, groups, again, 3)
    assert be.np(again).tobytes() == first.tobytes() and raw4.tobytes() == raw.tobytes()


def test_refusals_launch_nothing(be):
    Hn = Wn = 8
    h, w = 9, 7
    z = be.zeros((2, 4, Hn, Wn))
    pred = be.arr(np.full((2 * h * w,), GUARD, np.uint8))
    lab = be.zeros((2 * h * w,), np.uint8)
    counts = be.arr(np.full((2, 4, 3), 17, np.int64))
    P = be.ptr

    def table(null_pred=False, group=1):
        d = (_lib.WslValDst * 2)()
        for k in range(2):
            d[k].pred, d[k].label, d[k].h, d[k].w, d[k].group = P(pred) + k * h * w, P(lab) + k * h * w, h, w, k
        if null_pred:
            d[1].pred = None
        d[1].group = group
        return d

    def call(C_=4, n=2, d=None, zp=P(z)):
        return be.lib.wsl_val_labelmap(zp, d or table(), n, C_, Hn, Wn, P(counts), 2, be.stream)

    for kw in (dict(C_=0), dict(C_=9), dict(n=0), dict(d=table(null_pred=True)), dict(d=table(group=2)), dict(d=table(group=-1)),
               dict(zp=None)):
        assert call(**kw) == -1, kw                               # WSL_EINVAL
        assert b"val_labelmap" in be.lib.wsl_last_error(), kw
    be.sync()
    assert (be.np(pred) == GUARD).all() and (be.np(counts) == 17).all()
    assert call() == 0                                            # the same arguments, well-formed: accepted
    be.sync()
    assert (be.np(pred) == 0).all() and be.np(counts)[:, 0].tolist() == [[17 + h * w] * 3] * 2

    img, out = be.zeros((h, w)), be.arr(np.full((1, 1, 4, 4), -7.0, np.float32))
    s = (_lib.WslValSrc * 1)()
    s[0].img, s[0].h, s[0].w = P(img), h, w
    bad = (_lib.WslValSrc * 1)()
    bad[0].img, bad[0].h, bad[0].w = P(img), 0, w
    zin = lambda sl=s, n=1, op=P(out), Ho=4: be.lib.wsl_val_zoom_in(sl, n, op, Ho, 4, be.stream)  # noqa: E731
    for kw in (dict(sl=None), dict(n=0), dict(op=None), dict(Ho=0), dict(sl=bad)):
        assert zin(**kw) == -1, kw
        assert b"val_zoom_in" in be.lib.wsl_last_error(), kw
    be.sync()
    assert (be.np(out) == -7.0).all()
    assert zin() == 0
    be.sync()
    assert (be.np(out) == 0.0).all()
