"""The (ws, ws_bytes) entry points of csrc/wsl_dan.hip -- wsl_conv4s2_wgrad, wsl_dan_head_fwd_bwd, wsl_dan_forward, wsl_dan_backward --
called with EXACTLY the bytes their own query returns, inside guard words, as tests/test_workspace_guards.py does for the rest of the C
ABI (its guard_check: both guard zones untouched, results independent of the workspace's slack, one byte less returns WSL_EWORKSPACE and
writes nothing); and the WSL_EINVAL refusals the header documents, with every output untouched."""
import ctypes as C

import numpy as np
import pytest

from netutil import ptr_array
from test_workspace_guards import filled, guard_check, untouched
from wsl4mis_amd import _lib


def _id(case):
    return "-".join(str(v) for v in case)


# (N, Ci, Co, H, W): ordinary, odd, narrow, tall, one output column / row
WGRAD = [(2, 5, 16, 6, 10), (1, 3, 7, 7, 9), (2, 16, 32, 34, 18), (1, 6, 20, 36, 4), (1, 4, 8, 600, 2), (1, 2, 5, 3, 700), (1, 20, 40, 2, 2)]


@pytest.mark.parametrize("case", WGRAD, ids=_id)
def test_conv4s2_wgrad_inside_its_workspace(be, case):
    N, Ci, Co, H, W = case
    rng = np.random.default_rng(sum(case))
    x = be.arr(rng.standard_normal((N, Ci, H, W)).astype(np.float32))
    g = be.arr(rng.standard_normal((N, Co, H // 2, W // 2)).astype(np.float32))
    z = be.arr((rng.standard_normal((N, Co, H // 2, W // 2)) + 0.01).astype(np.float32))
    cm = be.arr(((rng.random((N, Co)) > 0.5) * 2.0).astype(np.float32))
    nb = be.lib.wsl_conv4s2_wgrad_ws_bytes(N, H, W, Ci, Co)

    def run(ws, n, outs):
        be.call("wsl_conv4s2_wgrad", be.ptr(x), 1, None, be.ptr(g), be.ptr(z), be.ptr(cm), be.ptr(outs[0]), be.ptr(outs[1]), N, Ci, H, W, Co,
                ws, n, be.stream)
    dw, db = guard_check(be, nb, lambda: [filled(be, (Co, Ci, 4, 4)), filled(be, (Co,))], run)
    assert np.all(np.isfinite(dw)) and np.all(np.isfinite(db))


# (N, C, H, W, pool): 2 x 2, 2 x 2 with rows / columns the floor drops, 1 x 4, 4 x 1
HEAD = [(3, 8, 2, 2, 1), (2, 16, 14, 14, 7), (2, 4, 15, 17, 7), (1, 5, 7, 28, 7), (2, 3, 12, 3, 3)]


@pytest.mark.parametrize("case", HEAD, ids=_id)
def test_dan_head_inside_its_workspace(be, case):
    N, Cc, H, W, pool = case
    rng = np.random.default_rng(sum(case))
    z = be.arr(rng.standard_normal((N, Cc, H, W)).astype(np.float32))
    Wc, bc = be.arr((rng.standard_normal((2, 4 * Cc)) * 0.3).astype(np.float32)), be.arr(rng.standard_normal(2).astype(np.float32))
    t = be.arr(rng.integers(0, 2, N).astype(np.int32))
    nb = be.lib.wsl_dan_head_ws_bytes(N, Cc)

    def run(ws, n, outs):
        be.call("wsl_dan_head_fwd_bwd", be.ptr(z), be.ptr(t), be.ptr(Wc), be.ptr(bc), pool, 1.0, be.ptr(outs[0]), be.ptr(outs[1]), be.ptr(outs[2]),
                be.ptr(outs[3]), be.ptr(outs[4]), N, Cc, H, W, ws, n, be.stream)
    loss, logits, dz, dW, db = guard_check(be, nb, lambda: [filled(be, (1,)), filled(be, (N, 2)), filled(be, (N, Cc, H, W)),
                                                            filled(be, (2, 4 * Cc)), filled(be, (2,))], run)
    assert np.isfinite(loss[0]) and loss[0] > 0 and np.all(np.isfinite(dz)) and np.all(np.isfinite(dW))
    assert abs(float(db.sum())) < 1e-6                       # softmax - onehot sums to zero over the two classes


# (num_classes, n_channel, ndf, pool, N, H, W)
NETS = [(3, 2, 4, 1, 2, 32, 32), (4, 1, 3, 1, 1, 16, 64), (2, 1, 2, 2, 1, 64, 70)]


@pytest.mark.parametrize("case", NETS, ids=_id)
def test_dan_network_inside_its_workspace(be, case):
    nc, ch, ndf, pool, N, H, W = case
    d = _lib.WslDanDesc(nc, ch, ndf, pool, N, H, W, 0)
    rng = np.random.default_rng(sum(case))
    n_param = be.lib.wsl_dan_param_count(C.byref(d))
    assert n_param == ndf * 16 * (nc + ch) + 2 * ndf + 16 * ndf * ndf * (2 + 8 + 32) + 14 * ndf + 64 * ndf + 2
    assert be.lib.wsl_dan_buffer_count(C.byref(d)) == 0 and be.lib.wsl_dan_num_entries(C.byref(d)) == 12
    params = be.arr((rng.standard_normal(n_param) * 0.2).astype(np.float32))
    map_, feat = be.arr(rng.random((N, nc, H, W)).astype(np.float32)), be.arr(rng.random((N, ch, H, W)).astype(np.float32))
    cms = [be.arr(((rng.random((N, k * ndf)) > 0.5) * 2.0).astype(np.float32)) for k in (2, 4)]
    t = be.arr(rng.integers(0, 2, N).astype(np.int32))
    nb = be.lib.wsl_dan_ws_bytes(C.byref(d))

    def run(ws, n, outs):
        be.call("wsl_dan_forward", C.byref(d), be.ptr(params), be.ptr(map_), be.ptr(feat), ptr_array(be, cms), 1, be.ptr(t), 1.0, be.ptr(outs[0]),
                be.ptr(outs[1]), ws, n, be.stream)
        be.call("wsl_dan_backward", C.byref(d), be.ptr(params), be.ptr(map_), be.ptr(feat), ptr_array(be, cms), None, 3, be.ptr(outs[2]),
                be.ptr(outs[3]), ws, n, be.stream)
    logits, loss, dmap, grads = guard_check(be, nb, lambda: [filled(be, (N, 2)), filled(be, (1,)), filled(be, (N, nc, H, W)), filled(be, (n_param,))], run)
    assert np.all(np.isfinite(logits)) and np.isfinite(loss[0]) and np.all(np.isfinite(dmap)) and np.all(np.isfinite(grads))


def test_refusals_write_nothing(be):
    """WSL_EINVAL: a pooled map that does not have 4 positions, a level with H or W < 2, a null required pointer"""
    L, rng = be.lib, np.random.default_rng(0)
    # ---- the head
    N, Cc = 2, 4
    z = be.arr(rng.standard_normal((N, Cc, 9, 9)).astype(np.float32))
    Wc, bc, t = be.arr(np.ones((2, 4 * Cc), np.float32)), be.arr(np.zeros(2, np.float32)), be.arr(np.zeros(N, np.int32))
    outs = [filled(be, (1,)), filled(be, (N, 2)), filled(be, (N, Cc, 9, 9)), filled(be, (2, 4 * Cc)), filled(be, (2,))]
    ws = filled(be, (4096,))
    head = lambda zz, tt, pool, lo: L.wsl_dan_head_fwd_bwd(zz, tt, be.ptr(Wc), be.ptr(bc), pool, 1.0, lo, be.ptr(outs[1]), be.ptr(outs[2]),  # noqa: E731
                                                           be.ptr(outs[3]), be.ptr(outs[4]), N, Cc, 9, 9, be.ptr(ws), 4096 * 4, be.stream)
    assert head(be.ptr(z), be.ptr(t), 3, be.ptr(outs[0])) == -1 and b"4 positions" in L.wsl_last_error()       # 3 x 3
    assert head(be.ptr(z), be.ptr(t), 7, be.ptr(outs[0])) == -1                                                # 1 x 1
    assert head(be.ptr(z), be.ptr(t), 0, be.ptr(outs[0])) == -1
    assert head(None, be.ptr(t), 4, be.ptr(outs[0])) == -1 and head(be.ptr(z), None, 4, be.ptr(outs[0])) == -1 and head(be.ptr(z), be.ptr(t), 4, None) == -1
    assert L.wsl_dan_head_fwd_bwd(be.ptr(z), be.ptr(t), be.ptr(Wc), be.ptr(bc), 4, 1.0, be.ptr(outs[0]), be.ptr(outs[1]), be.ptr(outs[2]),
                                  be.ptr(outs[3]), None, N, Cc, 9, 9, be.ptr(ws), 4096 * 4, be.stream) == -1          # dW without db
    be.sync()
    assert all(untouched(be, o) for o in outs) and untouched(be, ws)
    # ---- the network
    d_bad = _lib.WslDanDesc(4, 1, 2, 1, 1, 16, 16, 0)         # pools to 1 x 1
    d_small = _lib.WslDanDesc(4, 1, 2, 1, 1, 8, 64, 0)        # the third level would be 1 x 8
    d_ok = _lib.WslDanDesc(4, 1, 2, 1, 1, 32, 32, 0)
    assert L.wsl_dan_ws_bytes(C.byref(d_bad)) == 0 and b"4 positions" in L.wsl_last_error()
    assert L.wsl_dan_ws_bytes(C.byref(d_small)) == 0 and L.wsl_dan_ws_bytes(C.byref(d_ok)) > 0
    assert L.wsl_dan_num_entries(C.byref(_lib.WslDanDesc(0, 1, 2, 1, 1, 32, 32, 0))) == -1
    n_param = L.wsl_dan_param_count(C.byref(d_ok))
    params, map_, feat = be.arr(np.ones(n_param, np.float32)), be.arr(np.ones((1, 4, 32, 32), np.float32)), be.arr(np.ones((1, 1, 32, 32), np.float32))
    nb = L.wsl_dan_ws_bytes(C.byref(d_ok))
    ws2, logits, dmap, grads = filled(be, (nb // 4 + 1,)), filled(be, (1, 2)), filled(be, (1, 4, 32, 32)), filled(be, (n_param,))
    fwd = lambda dd, p, m, f, cm, tr, lg: L.wsl_dan_forward(C.byref(dd), p, m, f, cm, tr, None, 1.0, lg, None, be.ptr(ws2), nb, be.stream)  # noqa: E731
    assert fwd(d_bad, be.ptr(params), be.ptr(map_), be.ptr(feat), None, 0, be.ptr(logits)) == -1
    assert fwd(d_ok, None, be.ptr(map_), be.ptr(feat), None, 0, be.ptr(logits)) == -1
    assert fwd(d_ok, be.ptr(params), None, be.ptr(feat), None, 0, be.ptr(logits)) == -1
    assert fwd(d_ok, be.ptr(params), be.ptr(map_), None, None, 0, be.ptr(logits)) == -1
    assert fwd(d_ok, be.ptr(params), be.ptr(map_), be.ptr(feat), None, 0, None) == -1
    assert fwd(d_ok, be.ptr(params), be.ptr(map_), be.ptr(feat), None, 1, be.ptr(logits)) == -1                # training without masks
    bwd = lambda flags, dm, gr: L.wsl_dan_backward(C.byref(d_ok), be.ptr(params), be.ptr(map_), be.ptr(feat), None, be.ptr(logits), flags, dm, gr,  # noqa: E731
                                                   be.ptr(ws2), nb, be.stream)
    assert bwd(0, be.ptr(dmap), be.ptr(grads)) == -1 and bwd(1, None, be.ptr(grads)) == -1 and bwd(2, be.ptr(dmap), None) == -1 and bwd(4, be.ptr(dmap), be.ptr(grads)) == -1
    be.sync()
    assert all(untouched(be, o) for o in (ws2, logits, dmap, grads))
