"""The two backward routes that recompute instead of going through memory, against the routes they replace -- bit for bit:

  * classifier data gradient (4 -> 16 channels) in two passes of the narrow-K kernel with the BatchNorm-backward finalize between them
    (wsl_conv2d_dgrad_bn_dy, route 2) == wsl_conv2d_dgrad_bn followed by wsl_bnact_bwd_finish;
  * first convolution's weight gradient from a virtual dy (wsl_bnact_bwd_coef + wsl_conv2d_wgrad_bnd_partial) == wsl_bnact_bwd_finish_d_amax
    followed by wsl_conv2d_wgrad_partial on the materialised dy.

`be` runs every case on the host emulator (CPU) and, with -m gpu, on the MI355X; `be_route` where a number of workgroups is forced."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from wsl4mis_amd import _lib

TOL = 1e-4
# (N, H, W), 16 channels, 3x3, 8 x 64 tiles: one tile with all four image borders in it; eight tiles (tile edges in both directions, batch
# stride); 576 tiles = more than 2 x 256 persistent workgroups, so some workgroups walk two tiles (LDS tile and prefetch registers reused)
SHAPES = [(1, 8, 64), (2, 16, 128), (9, 64, 512)]
CH = 16


def _bn_table(rng, N, H, W):
    """raw conv output y and a BatchNorm table whose z = y * scale + shift takes both signs, every |z| clear of the LeakyReLU kink by far
    more than fp32 rounding (the float64 restatement must take the same side)"""
    y = rng.standard_normal((N, CH, H, W)).astype(np.float32)
    gamma, beta = (rng.random(CH) + 0.5).astype(np.float32), (rng.standard_normal(CH) * 0.3).astype(np.float32)
    mean = y.mean((0, 2, 3)).astype(np.float32)
    invstd = (1.0 / np.sqrt(y.var((0, 2, 3)) + 1e-5)).astype(np.float32)
    scale = (gamma * invstd).astype(np.float32)
    shift = (beta - mean * scale).astype(np.float32)
    for _ in range(4):
        z = y.astype(np.float64) * scale[None, :, None, None] + shift[None, :, None, None]
        near = np.abs(z) < 1e-4
        if not near.any():
            break
        y[near] += np.float32(0.01)
    assert (z > 0).any() and (z < 0).any() and not near.any()
    st = np.concatenate([mean, invstd, scale, shift]).astype(np.float32)
    return y, gamma, beta, mean, invstd, st


def _dy64(g, y, gamma, mean, invstd, st, leaky):
    """float64 restatement of the BatchNorm (+ LeakyReLU) backward: dy = gamma * invstd * (d - mean(d) - xhat * mean(d * xhat))"""
    g, y = g.astype(np.float64), y.astype(np.float64)
    b = lambda v: v.astype(np.float64)[None, :, None, None]
    d = g
    if leaky:
        z = y * b(st[2 * CH:3 * CH]) + b(st[3 * CH:])
        d = g * np.where(z > 0, 1.0, 0.01)
    xh = (y - b(mean)) * b(invstd)
    c1, c2 = d.mean((0, 2, 3), keepdims=True), (d * xh).mean((0, 2, 3), keepdims=True)
    return b(gamma) * b(invstd) * (d - c1 - xh * c2), d.sum((0, 2, 3)), (d * xh).sum((0, 2, 3))


# ------------------------------------------------------------------------------------------------ classifier data gradient
def _cls_setup(be, rng, N, H, W):
    dlog = (rng.standard_normal((N, 4, H, W)) * 0.1).astype(np.float32)
    w = (rng.standard_normal((4, CH, 3, 3)) * 0.2).astype(np.float32)          # the classifier 16 -> 4: its data gradient maps 4 -> 16
    y, gamma, beta, mean, invstd, st = _bn_table(rng, N, H, W)
    host = dict(dlog=dlog, w=w, y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, st=st)
    d = {k: be.arr(v) for k, v in host.items()}
    wp = be.zeros((9 * 4 * CH,))
    be.call("wsl_conv2d_pack_weights", be.ptr(d["w"]), be.ptr(wp), 4, CH, 3, 1, be.stream)
    return host, d, wp


def _cls_today(be, d, wp, N, H, W, amax=None):
    """wsl_conv2d_dgrad_bn_d (the net's call; the narrow-K kernel writes the plain gradient: wsl_conv2d_dgrad_bn's launch) + finish"""
    nws = be.lib.wsl_bnact_bwd_ws_bytes(N, CH, H, W)
    ncoef = be.lib.wsl_bnact_bwd_finish_ws_bytes(N, CH, H, W, 1)
    g, dy, dg, db, part, coef = be.zeros((N, CH, H, W)), be.zeros((N, CH, H, W)), be.zeros((CH,)), be.zeros((CH,)), be.ws(nws), be.ws(ncoef)
    fused = C.c_int(-1)
    src = be.src(d["dlog"], 4)
    be.call("wsl_conv2d_dgrad_bn_d", src, be.ptr(wp), be.ptr(g), CH * H * W, N, H, W, CH, 3, 3, be.ptr(d["y"]), be.ptr(d["st"]), None, 1.0,
            be.ptr(part), C.byref(fused), be.stream)
    bn = [be.ptr(g), CH * H * W, be.ptr(d["y"]), be.ptr(d["mean"]), be.ptr(d["invstd"]), be.ptr(d["gamma"]), be.ptr(d["beta"])]
    out = [be.ptr(dy), be.ptr(dg), be.ptr(db), N, CH, H, W]
    if fused.value == 2:
        nblk = be.lib.wsl_conv2d_stat_blocks(N, H, W, 4, CH, 3)
        be.call("wsl_bnact_bwd_finish_d_amax", *bn, *out, be.ptr(part), nblk, 1, be.ptr(coef), ncoef, amax, be.stream)
    elif fused.value == 1:
        nblk = be.lib.wsl_conv2d_stat_blocks(N, H, W, 4, CH, 3)
        be.call("wsl_bnact_bwd_finish_amax", *bn, None, 1.0, *out, be.ptr(part), nblk, 1, be.ptr(coef), ncoef, amax, be.stream)
    else:
        nblk = 0
        be.call("wsl_bnact_bwd_amax", *bn, None, 1.0, *out, be.ptr(part), nws, amax, be.stream)
    return fused.value, nblk, [be.np(t).copy() for t in (g, dy, dg, db, part)]


def _cls_new(be, d, wp, N, H, W, amax=None):
    nws = be.lib.wsl_bnact_bwd_ws_bytes(N, CH, H, W)
    ncoef = be.lib.wsl_bnact_bwd_finish_ws_bytes(N, CH, H, W, 1)
    g, dy, dg, db, part, coef = be.zeros((N, CH, H, W)), be.zeros((N, CH, H, W)), be.zeros((CH,)), be.zeros((CH,)), be.ws(nws), be.ws(ncoef)
    route = C.c_int(-1)
    be.call("wsl_conv2d_dgrad_bn_dy", be.src(d["dlog"], 4), be.ptr(wp), be.ptr(g), N, H, W, CH, 3, 3, be.ptr(d["y"]), be.ptr(d["st"]),
            be.ptr(d["gamma"]), be.ptr(d["beta"]), be.ptr(part), nws, be.ptr(dy), be.ptr(dg), be.ptr(db), be.ptr(coef), ncoef, amax,
            C.byref(route), be.stream)
    return route.value, [be.np(t).copy() for t in (g, dy, dg, db, part)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_classifier_dgrad_two_pass_equals_todays_route(be, shape):
    N, H, W = shape
    host, d, wp = _cls_setup(be, np.random.default_rng(N * 1000 + H + W), N, H, W)
    # today's route through its plain entry points: wsl_conv2d_dgrad_bn followed by wsl_bnact_bwd_finish
    nws = be.lib.wsl_bnact_bwd_ws_bytes(N, CH, H, W)
    g, dy, dg, db, part, coef = be.zeros((N, CH, H, W)), be.zeros((N, CH, H, W)), be.zeros((CH,)), be.zeros((CH,)), be.ws(nws), be.zeros((2 * CH,))
    fused = C.c_int(-1)
    be.call("wsl_conv2d_dgrad_bn", be.src(d["dlog"], 4), be.ptr(wp), be.ptr(g), CH * H * W, N, H, W, CH, 3, 3, be.ptr(d["y"]),
            be.ptr(d["st"]), None, 1.0, be.ptr(part), C.byref(fused), be.stream)
    assert fused.value == 1
    nblk = be.lib.wsl_conv2d_stat_blocks(N, H, W, 4, CH, 3)
    assert nblk == N * (H // 8) * (W // 64)
    be.call("wsl_bnact_bwd_finish", be.ptr(g), CH * H * W, be.ptr(d["y"]), be.ptr(d["mean"]), be.ptr(d["invstd"]), be.ptr(d["gamma"]),
            be.ptr(d["beta"]), None, 1.0, be.ptr(dy), be.ptr(dg), be.ptr(db), N, CH, H, W, be.ptr(part), nblk, 1, be.ptr(coef), 8 * CH,
            be.stream)
    route, (g2, dy2, dg2, db2, part2) = _cls_new(be, d, wp, N, H, W)
    assert route == 2
    assert not g2.any()                                                        # the gradient itself is never written
    assert np.array_equal(part2[:nblk * CH * 2], be.np(part)[:nblk * CH * 2])  # statistics partials [C][tiles][2]
    assert np.array_equal(dg2, be.np(dg)) and np.array_equal(db2, be.np(db))
    assert np.array_equal(dy2, be.np(dy))
    # ... and the float64 restatement
    g64 = F.conv_transpose2d(torch.from_numpy(host["dlog"]).double(), torch.from_numpy(host["w"]).double(), padding=1).numpy()
    dy64, s1, s2 = _dy64(g64, host["y"], host["gamma"], host["mean"], host["invstd"], host["st"], True)
    e = rel_err(dy2, dy64)
    print(f"classifier {shape}: dy vs float64 {e:.2e}")
    assert e < TOL
    assert rel_err(db2, s1) < TOL and rel_err(dg2, s2) < TOL


def test_classifier_dgrad_ineligible_width_takes_todays_route(be):
    N, H, W = 1, 16, 48
    host, d, wp = _cls_setup(be, np.random.default_rng(48), N, H, W)
    fused, nblk, ref = _cls_today(be, d, wp, N, H, W)
    route, got = _cls_new(be, d, wp, N, H, W)
    assert route == (1 if fused else 0)
    for a, b in zip(got[:4], ref[:4]):                                         # g, dy, dgamma, dbeta
        assert np.array_equal(a, b)
    g64 = F.conv_transpose2d(torch.from_numpy(host["dlog"]).double(), torch.from_numpy(host["w"]).double(), padding=1).numpy()
    assert rel_err(got[1], _dy64(g64, host["y"], host["gamma"], host["mean"], host["invstd"], host["st"], True)[0]) < TOL


def test_classifier_dgrad_split_precision_takes_todays_route(be):
    """the split-precision net wants max |dy| of every BatchNorm layer (the operand scale of dy's consumers): the apply pass of today's
    route leaves it, so a call that asks for it takes today's route at a shape the two-pass route would take otherwise"""
    N, H, W = 2, 16, 128
    host, d, wp = _cls_setup(be, np.random.default_rng(7), N, H, W)
    am_ref, am = be.arr(np.zeros(64, np.int32)), be.arr(np.zeros(64, np.int32))   # bit patterns of non-negative floats
    fused, nblk, ref = _cls_today(be, d, wp, N, H, W, be.ptr(am_ref))
    assert fused == 1
    route, got = _cls_new(be, d, wp, N, H, W, be.ptr(am))
    assert route == 1
    for a, b in zip(got[:4], ref[:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(be.np(am), be.np(am_ref))
    assert be.np(am).max() == np.abs(got[1]).max().view(np.int32)
    route2, got2 = _cls_new(be, d, wp, N, H, W)                                # without the maximum: two passes, the same dy
    assert route2 == 2 and np.array_equal(got2[1], got[1])


# ------------------------------------------------------------------------------------------------ first convolution's weight gradient
def _first_setup(be, rng, N, H, W):
    x = rng.standard_normal((N, 1, H, W)).astype(np.float32)
    dz = (rng.standard_normal((N, CH, H, W)) * 0.1).astype(np.float32)         # the gradient in front of the BatchNorm output (d form)
    y, gamma, beta, mean, invstd, st = _bn_table(rng, N, H, W)
    # the producer's partial sums, one per 8 x 64 tile and channel: [C][tiles][2] = (sum dz, sum dz * xhat)
    xh = (y - mean[None, :, None, None]) * invstd[None, :, None, None]
    t = lambda v: v.reshape(N, CH, H // 8, 8, W // 64, 64).sum((3, 5), dtype=np.float32).transpose(1, 0, 2, 3).reshape(CH, -1)
    part = np.stack([t(dz), t(dz * xh)], -1).astype(np.float32)
    host = dict(x=x, dz=dz, y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, part=part)
    return host, {k: be.arr(v) for k, v in host.items()}, part.shape[1]


def _first_today(be, d, nblk, N, H, W):
    dy, dg, db, coef = be.zeros((N, CH, H, W)), be.zeros((CH,)), be.zeros((CH,)), be.zeros((2 * CH,))
    be.call("wsl_bnact_bwd_finish_d_amax", be.ptr(d["dz"]), CH * H * W, be.ptr(d["y"]), be.ptr(d["mean"]), be.ptr(d["invstd"]),
            be.ptr(d["gamma"]), be.ptr(d["beta"]), be.ptr(dy), be.ptr(dg), be.ptr(db), N, CH, H, W, be.ptr(d["part"]), nblk, 1, be.ptr(coef),
            8 * CH, None, be.stream)
    nws = be.lib.wsl_conv2d_wgrad_ws_bytes(N, H, W, 1, CH, 3)
    ws, dw, dbias = be.ws(nws), be.zeros((CH, 1, 3, 3)), be.zeros((CH,))
    pend = _lib.WslWgradPending()
    be.call("wsl_conv2d_wgrad_partial", be.src(d["x"], 1), be.src(), be.ptr(dy), CH * H * W, be.ptr(dw), be.ptr(dbias), N, H, W, CH, 3,
            be.ptr(ws), nws, C.byref(pend), be.stream)
    be.call("wsl_wgrad_reduce_batch", C.byref(pend), 1, be.stream)
    return [be.np(t).copy() for t in (dw, dbias, dg, db, coef, dy)], pend.nsplit


def _first_new(be, d, nblk, N, H, W):
    dg, db, coef = be.zeros((CH,)), be.zeros((CH,)), be.zeros((2 * CH,))
    sx = be.src(d["x"], 1)
    assert be.lib.wsl_conv2d_wgrad_bnd_ok(sx, be.src(), be.ptr(d["dz"]), CH * H * W, be.ptr(d["y"]), CH * H * W, H, W, CH, 3) == 1
    be.call("wsl_bnact_bwd_coef", be.ptr(d["part"]), nblk, 1, N, CH, H, W, be.ptr(dg), be.ptr(db), be.ptr(coef), be.stream)
    nws = be.lib.wsl_conv2d_wgrad_ws_bytes(N, H, W, 1, CH, 3)
    ws, dw, dbias = be.ws(nws), be.zeros((CH, 1, 3, 3)), be.zeros((CH,))
    pend = _lib.WslWgradPending()
    be.call("wsl_conv2d_wgrad_bnd_partial", sx, be.ptr(d["dz"]), CH * H * W, be.ptr(d["y"]), CH * H * W, be.ptr(d["mean"]),
            be.ptr(d["invstd"]), be.ptr(d["gamma"]), be.ptr(coef), be.ptr(dw), be.ptr(dbias), N, H, W, CH, 3, be.ptr(ws), nws,
            C.byref(pend), be.stream)
    be.call("wsl_wgrad_reduce_batch", C.byref(pend), 1, be.stream)
    return [be.np(t).copy() for t in (dw, dbias, dg, db, coef)], pend.nsplit


def _first_check(be, shape, seed):
    N, H, W = shape
    host, d, nblk = _first_setup(be, np.random.default_rng(seed), N, H, W)
    ref, ns_ref = _first_today(be, d, nblk, N, H, W)
    got, ns = _first_new(be, d, nblk, N, H, W)
    assert ns == ns_ref                                                        # the same plan: the same splits, partials and sums
    for name, a, b in zip(("dw", "db", "dgamma", "dbeta", "coef"), got, ref):
        assert np.array_equal(a, b), name
    # float64 restatement of the whole pair (BatchNorm backward in its d form + weight gradient)
    dy64, _, _ = _dy64(host["dz"], host["y"], host["gamma"], host["mean"], host["invstd"], None, False)
    wt = torch.zeros(CH, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(CH, dtype=torch.float64, requires_grad=True)
    (F.conv2d(torch.from_numpy(host["x"]).double(), wt, bt, padding=1) * torch.from_numpy(dy64)).sum().backward()
    e = rel_err(got[0], wt.grad.numpy())
    print(f"first conv {shape}: dw vs float64 {e:.2e}")
    assert e < TOL
    # (db is mathematically zero -- dy sums to zero per channel: round-off on both sides, compared with the materialised route above only)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_conv_wgrad_from_virtual_dy_equals_materialised_dy(be, shape):
    _first_check(be, shape, shape[0] * 100 + shape[1])


@pytest.mark.parametrize("wgs", [8, 5])
def test_first_conv_virtual_dy_tile_walks(be_route, wgs):
    """few persistent workgroups: every split walks several tiles, in the interleaved (splits % 8 == 0) and in the contiguous order"""
    be = be_route
    be.call("wsl_debug_wgrad_workgroups", wgs)
    try:
        _first_check(be, (3, 24, 128), wgs)
    finally:
        be.call("wsl_debug_wgrad_workgroups", 0)


def test_first_conv_virtual_dy_is_refused_where_the_kernel_does_not_fit(be):
    """no quiet fall-back inside the entry point: the caller asks wsl_conv2d_wgrad_bnd_ok() and takes the two-launch route otherwise"""
    N, H, W = 1, 16, 48
    rng = np.random.default_rng(5)
    x, x4 = be.arr(rng.standard_normal((N, 1, H, W)).astype(np.float32)), be.arr(rng.standard_normal((N, 4, H, W)).astype(np.float32))
    dz, y = be.zeros((N, CH, H, W)), be.zeros((N, CH, H, W))
    v = be.arr(np.ones(2 * CH, np.float32))
    ok = lambda s, co=CH, ks=3, h=H, w=W, off=0: be.lib.wsl_conv2d_wgrad_bnd_ok(s, be.src(), be.ptr(dz) + off, CH * h * w, be.ptr(y), CH * h * w,
                                                                              h, w, co, ks)
    assert ok(be.src(x, 1)) == 0                                               # W = 48: no full 8 x 64 tiles
    assert ok(be.src(x, 1), h=8, w=64) == 1                                    # (the same buffers hold one 8 x 64 tile)
    assert ok(be.src(x, 1), h=8, w=64, off=4) == 0                             # dz not float4-aligned
    assert ok(be.src(x, 1), h=8, w=64, ks=1) == 0
    assert ok(be.src(x4, 4), h=8, w=64) == 0                                   # more than one input channel
    assert ok(be.src(x, 1, scale=v, shift=v), h=8, w=64) == 0                  # a source with a loader transform
    nws = be.lib.wsl_conv2d_wgrad_ws_bytes(N, H, W, 1, CH, 3)
    ws, dw, dbias, pend = be.ws(nws), be.zeros((CH, 1, 3, 3)), be.zeros((CH,)), _lib.WslWgradPending()
    with pytest.raises(_lib.WslError, match="wgrad_bnd"):
        be.call("wsl_conv2d_wgrad_bnd_partial", be.src(x, 1), be.ptr(dz), CH * H * W, be.ptr(y), CH * H * W, be.ptr(v), be.ptr(v), be.ptr(v),
                be.ptr(v), be.ptr(dw), be.ptr(dbias), N, H, W, CH, 3, be.ptr(ws), nws, C.byref(pend), be.stream)
