"""The 4x4 stride-2 padding-1 convolution of the DAN adversary through the C ABI: forward (one and two sources, loader LeakyReLU(0.2) +
Dropout2d multiplier), data gradient (four parity phases, four borders) and weight gradient, against float64 torch (tests/dan_ref.py).
`be` runs every case on the host emulator and, with -m gpu, on the MI355X; the two cases with real channel counts run on the device only.

Criterion: conftest.close() / grad_tol at TOL = 1e-4 of each tensor's scale, as in the other op tests.  The LeakyReLU decision of the
backward is taken on the saved pre-activation z, an INPUT of these entry points: it is generated at least MARGIN away from the kink
(asserted), so both sides take the same branch whatever their rounding."""
import numpy as np
import pytest
import torch

import dan_ref as R
from conftest import close, get_backend, grad_tol

TOL = 1e-4
MARGIN = 1e-3

# (N, Ca, Cb, Co, H, W)
CASES = [
    (1, 1, 0, 16, 2, 2),      # a single output pixel, all taps but four in the padding
    (2, 4, 1, 16, 6, 10),     # two sources 4 + 1, K tail
    (1, 3, 0, 7, 7, 9),       # odd sizes, Co tail
    (2, 16, 0, 32, 34, 18),   # crosses a 16-pixel M tile in both directions, H != W
    (1, 6, 0, 20, 36, 4),     # narrow
]
DEVICE_CASES = [
    (1, 256, 0, 512, 4, 4),   # the deepest layer's channel counts at the smallest map
    (2, 64, 0, 128, 32, 32),  # real channel counts
]


@pytest.fixture
def be_hip():
    return get_backend("hip")


def run_case(be, case, act):
    N, Ca, Cb, Co, H, W = case
    Ho, Wo = H // 2, W // 2
    rng = np.random.default_rng(abs(hash((case, act))) % 2**31)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    xa = f32(rng.standard_normal((N, Ca, H, W)))
    xb = f32(rng.standard_normal((N, Cb, H, W))) if Cb else None
    wa = f32(rng.standard_normal((Co, Ca, 4, 4)) * 0.2)
    wb = f32(rng.standard_normal((Co, Cb, 4, 4)) * 0.2) if Cb else None
    ba, bb = f32(rng.standard_normal(Co)), (f32(rng.standard_normal(Co)) if Cb else None)
    g = f32(rng.standard_normal((N, Co, Ho, Wo)))
    cm_in = cm_out = z = None
    if act:
        cm_in = f32((rng.random((N, Ca)) > 0.5) * 2.0)
        cm_in[0, 0] = 0.0                                   # a dropped channel ...
        cm_in[-1, -1] = 2.0                                 # ... and a kept one, whatever the draw
        cm_out = f32((rng.random((N, Co)) > 0.5) * 2.0)
        cm_out[0, 0], cm_out[-1, -1] = 0.0, 2.0
        z = rng.standard_normal((N, Co, Ho, Wo))
        z = f32(np.where(np.abs(z) < 2 * MARGIN, 2 * MARGIN * np.sign(z + 1e-30), z))
        assert float(np.abs(z).min()) >= MARGIN             # kink margin of the backward's LeakyReLU decision
    # ---- checker (float64)
    t = lambda a: torch.from_numpy(a).double()
    va = t(xa)
    if act:
        va = torch.nn.functional.leaky_relu(va, R.SLOPE) * t(cm_in)[:, :, None, None]
    vin = (torch.cat([va, t(xb)], 1) if Cb else va).requires_grad_()
    wt = (torch.cat([t(wa), t(wb)], 1) if Cb else t(wa)).requires_grad_()
    bt = (t(ba) + t(bb) if Cb else t(ba)).requires_grad_()
    y_ref = R.conv4s2(vin, wt, bt)
    assert tuple(y_ref.shape) == (N, Co, Ho, Wo)
    dy = t(g)
    if act:
        dy = dy * t(cm_out)[:, :, None, None] * torch.where(t(z) > 0, 1.0, R.SLOPE)
    y_ref.backward(dy)
    y_ref, dx_ref, dw_ref, db_ref = y_ref.detach().numpy(), vin.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()
    # ---- device
    d = {k: (be.arr(v) if v is not None else None) for k, v in
         dict(xa=xa, xb=xb, wa=wa, wb=wb, ba=ba, bb=bb, g=g, cm_in=cm_in, cm_out=cm_out, z=z).items()}
    P = lambda k: be.ptr(d[k]) if d[k] is not None else None

    def fwd(xa_, Ca_, xb_, Cb_, wa_, wb_, ba_, bb_):
        y = be.zeros((N, Co, Ho, Wo))
        first = xa_ == P("xa")                               # activation and multiplier belong to source a
        be.call("wsl_conv4s2_fwd", xa_, Ca_, xb_, Cb_, int(act and first), P("cm_in") if first else None, wa_, wb_, ba_, bb_, be.ptr(y),
                N, H, W, Co, be.stream)
        return be.np(y)
    y = fwd(P("xa"), Ca, P("xb"), Cb, P("wa"), P("wb"), P("ba"), P("bb"))
    print(f"conv4s2 {case} act={act}: fwd max err {np.abs(y - y_ref).max():.3e} of scale {np.abs(y_ref).max():.3e}")
    assert close(y, y_ref, TOL)
    assert np.array_equal(y, fwd(P("xa"), Ca, P("xb"), Cb, P("wa"), P("wb"), P("ba"), P("bb")))          # bit-reproducible
    if Cb:   # the merged pass equals the sum of two one-source passes
        y_a = fwd(P("xa"), Ca, None, 0, P("wa"), None, P("ba"), None)
        y_b = fwd(P("xb"), Cb, None, 0, P("wb"), None, P("bb"), None)
        assert close(y, y_a.astype(np.float64) + y_b, TOL)
    # ---- data gradient with respect to source a: every parity phase and every border on its own scale
    def dgrad():
        dx = be.zeros((N, Ca, H, W))
        dx += 7.0                                            # (every element must be WRITTEN, not accumulated into)
        be.call("wsl_conv4s2_dgrad", P("g"), P("z"), P("cm_out"), P("wa"), be.ptr(dx), N, Ca, H, W, Co, be.stream)
        return be.np(dx).copy()
    dx = dgrad()
    ref = dx_ref[:, :Ca]
    assert close(dx, ref, TOL)
    for py in range(2):
        for px in range(2):
            if ref[:, :, py::2, px::2].size:
                assert close(dx[:, :, py::2, px::2], ref[:, :, py::2, px::2], TOL), ("phase", py, px)
    for name, sl in (("top", np.s_[:, :, 0]), ("bottom", np.s_[:, :, -1]), ("left", np.s_[:, :, :, 0]), ("right", np.s_[:, :, :, -1])):
        assert close(dx[sl], ref[sl], TOL), name
    assert np.array_equal(dx, dgrad())
    # ---- weight gradient, one call per source
    def wgrad(x_, Ci_, act_, cm_):
        nb = be.lib.wsl_conv4s2_wgrad_ws_bytes(N, H, W, Ci_, Co)
        assert nb > 0
        ws, dw, db = be.ws(nb), be.zeros((Co, Ci_, 4, 4)), be.zeros((Co,))
        be.call("wsl_conv4s2_wgrad", x_, int(act_), cm_, P("g"), P("z"), P("cm_out"), be.ptr(dw), be.ptr(db), N, Ci_, H, W, Co, be.ptr(ws),
                nb, be.stream)
        return be.np(dw).copy(), be.np(db).copy()
    dw, db = wgrad(P("xa"), Ca, act, P("cm_in"))
    print(f"conv4s2 {case} act={act}: dw max err {np.abs(dw - dw_ref[:, :Ca]).max():.3e} of scale {np.abs(dw_ref[:, :Ca]).max():.3e}")
    assert np.abs(dw - dw_ref[:, :Ca]).max() <= grad_tol("dw", dw_ref[:, :Ca], TOL)
    assert np.abs(db - db_ref).max() <= grad_tol("db", db_ref, TOL)
    assert close(dw, dw_ref[:, :Ca], TOL)
    dw2, db2 = wgrad(P("xa"), Ca, act, P("cm_in"))
    assert np.array_equal(dw, dw2) and np.array_equal(db, db2)
    if Cb:
        dwb, dbb = wgrad(P("xb"), Cb, False, None)
        assert np.abs(dwb - dw_ref[:, Ca:]).max() <= grad_tol("dw", dw_ref[:, Ca:], TOL)
        assert np.array_equal(dbb, db)                       # db0 = db1, bit for bit


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_conv4s2_fwd_dgrad_wgrad(be, case, act):
    run_case(be, case, act)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("case", DEVICE_CASES)
def test_conv4s2_real_channel_counts(be_hip, case, act):
    run_case(be_hip, case, act)


def test_conv4s2_refusals(be):
    """WSL_EINVAL with nothing written: H or W < 2, a null required pointer, a second source without weights"""
    x, w, y = be.arr(np.ones((1, 1, 4, 4), np.float32)), be.arr(np.ones((16, 1, 4, 4), np.float32)), be.zeros((1, 16, 2, 2))
    L = be.lib
    assert L.wsl_conv4s2_fwd(be.ptr(x), 1, None, 0, 0, None, be.ptr(w), None, None, None, be.ptr(y), 1, 1, 4, 16, be.stream) == -1
    assert L.wsl_conv4s2_fwd(be.ptr(x), 1, None, 0, 0, None, be.ptr(w), None, None, None, be.ptr(y), 1, 4, 1, 16, be.stream) == -1
    assert L.wsl_conv4s2_fwd(None, 1, None, 0, 0, None, be.ptr(w), None, None, None, be.ptr(y), 1, 4, 4, 16, be.stream) == -1
    assert L.wsl_conv4s2_fwd(be.ptr(x), 1, be.ptr(x), 1, 0, None, be.ptr(w), None, None, None, be.ptr(y), 1, 4, 4, 16, be.stream) == -1
    assert L.wsl_conv4s2_dgrad(be.ptr(y), None, None, be.ptr(w), be.ptr(x), 1, 1, 1, 4, 16, be.stream) == -1
    assert L.wsl_conv4s2_dgrad(be.ptr(y), None, None, None, be.ptr(x), 1, 1, 4, 4, 16, be.stream) == -1
    be.sync()
    assert not be.np(y).any() and np.array_equal(be.np(x), np.ones((1, 1, 4, 4), np.float32))
