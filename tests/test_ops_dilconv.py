"""Dilated 3x3 convolutions (PNet2D's blocks, ref: networks/pnet.py) through the C ABI: forward, data gradient and weight gradient
against torch-CPU F.conv2d(..., dilation=d) in fp64, with the loader transforms (BatchNorm scale / shift + LeakyReLU, channel
multiplier), batch-strided source and output (the concat slices of PNet) and the BatchNorm partials through wsl_bn_stats_finalize.
`be` runs every case on the host emulator (CPU) and, with -m gpu, on the MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import close
from wsl4mis_amd import _lib

TOL = 1e-4
DILS = (1, 2, 3, 4, 8, 16)
CHANS = ((1, 64), (16, 16), (64, 64))
SIZES = ((16, 16), (24, 40), (40, 56))


def _run(be, N, H, W, Ci, Co, d, loader, strided, seed):
    rng = np.random.default_rng(seed)
    extra = 3 if strided else 0                      # the source / output live in wider tensors (channel slices)
    xs = rng.standard_normal((N, Ci + extra, H, W)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 3, 3)) / np.sqrt(9 * Ci)).astype(np.float32)
    bias = rng.standard_normal(Co).astype(np.float32)
    r = rng.standard_normal((N, Co, H, W)).astype(np.float32)
    use_t = loader and Ci > 1
    scale = (rng.standard_normal(Ci) * 0.5 + 1).astype(np.float32) if use_t else None
    shift = (rng.standard_normal(Ci) * 0.3).astype(np.float32) if use_t else None
    cmask = ((rng.random((N, Ci)) >= 0.3) / 0.7).astype(np.float32) if use_t else None

    # fp64 checker on the CPU
    v = torch.from_numpy(xs[:, :Ci]).double()
    if use_t:
        v = F.leaky_relu(v * torch.from_numpy(scale).double()[None, :, None, None] + torch.from_numpy(shift).double()[None, :, None, None],
                         0.01)
        v = v * torch.from_numpy(cmask).double()[:, :, None, None]
    v.requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    bt = torch.from_numpy(bias).double().requires_grad_(True)
    y_ref = F.conv2d(v, wt, bt, padding=d, dilation=d)
    (y_ref * torch.from_numpy(r).double()).sum().backward()

    dx = be.arr(xs)
    dsc = be.arr(scale) if use_t else None
    dsh = be.arr(shift) if use_t else None
    dcm = be.arr(cmask) if use_t else None
    src = be.src(dx, Ci, bs=(Ci + extra) * H * W, scale=dsc, shift=dsh, cmask=dcm)
    dw, db, dr = be.arr(w), be.arr(bias), be.arr(r)
    y_bs = (Co + extra) * H * W
    ybuf = be.zeros((N, Co + extra, H, W))
    nblk = be.lib.wsl_conv2d_dil_stat_blocks(N, H, W, Ci, Co, d)
    assert nblk > 0
    sp, sc = be.zeros((Co * nblk * 2,)), be.zeros((nblk,))
    be.call("wsl_conv2d_dil_fwd", src, be.src(), be.ptr(dw), be.ptr(db), be.ptr(ybuf), y_bs, N, H, W, Co, 3, d, 0, be.ptr(sp),
            be.ptr(sc), be.stream)
    y = be.np(ybuf)[:, :Co]
    assert close(y, y_ref.detach().numpy(), TOL), ("forward", d, Ci, Co, H, W)
    # BatchNorm partials -> mean / invstd
    gamma, beta = be.arr(np.ones(Co, np.float32)), be.arr(np.zeros(Co, np.float32))
    mean, invstd, bsc, bsh = (be.zeros((Co,)) for _ in range(4))
    be.call("wsl_bn_stats_finalize", be.ptr(sp), be.ptr(sc), nblk, Co, be.ptr(gamma), be.ptr(beta), 1e-5, 0.1, None, None, None,
            be.ptr(mean), be.ptr(invstd), be.ptr(bsc), be.ptr(bsh), be.stream)
    yr = y_ref.detach()
    m_ref = yr.mean(dim=(0, 2, 3)).numpy()
    is_ref = (1.0 / torch.sqrt(yr.var(dim=(0, 2, 3), unbiased=False) + 1e-5)).numpy()
    assert close(be.np(mean), m_ref, TOL) and close(be.np(invstd), is_ref, TOL), ("bn stats", d)
    # data gradient: wmode 1 with the forward weight, source = dy (batch strided when `strided`)
    rs = np.zeros((N, Co + extra, H, W), np.float32)
    rs[:, :Co] = r
    drs = be.arr(rs)
    gsrc = be.src(drs, Co, bs=(Co + extra) * H * W)
    gbuf = be.zeros((N, Ci + extra, H, W))
    be.call("wsl_conv2d_dil_fwd", gsrc, be.src(), be.ptr(dw), None, be.ptr(gbuf), (Ci + extra) * H * W, N, H, W, Ci, 3, d, 1, None, None,
            be.stream)
    assert close(be.np(gbuf)[:, :Ci], v.grad.numpy(), TOL), ("data gradient", d, Ci, Co, H, W)
    # weight gradient (partials + the existing second stage)
    nws = be.lib.wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, Ci, Co, 3, d)
    ws, gw, gb = be.ws(nws), be.zeros((Co, Ci, 3, 3)), be.zeros((Co,))
    be.call("wsl_conv2d_dil_wgrad", src, be.src(), be.ptr(dr), Co * H * W, be.ptr(gw), be.ptr(gb), N, H, W, Co, 3, d, be.ptr(ws), nws,
            be.stream)
    assert close(be.np(gw), wt.grad.numpy(), TOL), ("weight gradient", d, Ci, Co, H, W)
    assert close(be.np(gb), bt.grad.numpy(), TOL), ("bias gradient", d)


# every dilation x channel pair, the sizes rotated over the dilations (the emulator runs each case lock-step on the CPU)
CASES = [(d, ci, co, SIZES[(i + j) % 3]) for i, d in enumerate(DILS) for j, (ci, co) in enumerate(CHANS)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"d{c[0]}_{c[1]}to{c[2]}_{c[3][0]}x{c[3][1]}")
def test_dilconv_ops(be, case):
    d, ci, co, (H, W) = case
    for loader, strided in ((True, True), (False, False)):
        _run(be, 2, H, W, ci, co, d, loader, strided, seed=d * 100 + ci + co + H)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("d", DILS)
def test_dilconv_ops_all_sizes_gpu(d, hw):
    from conftest import get_backend
    be = get_backend("hip")
    for ci, co in CHANS:
        _run(be, 2, hw[0], hw[1], ci, co, d, True, True, seed=7 * d + ci + hw[1])


@pytest.mark.gpu
@pytest.mark.parametrize("d", DILS)
def test_dilconv_ops_fullres_gpu(d):
    """PNet's layer shape: 64 -> 64 at 256 x 256, N = 2"""
    from conftest import get_backend
    _run(get_backend("hip"), 2, 256, 256, 64, 64, d, True, True, seed=d)


def test_dilconv_any_width(be):
    """W % 4 != 0 (W = 30) takes the same kernels with scalar stores: correct, not refused"""
    _run(be, 1, 12, 30, 16, 16, 4, True, True, seed=30)
    _run(be, 1, 9, 30, 1, 16, 3, False, False, seed=31)


def test_dilconv_large_dilations(be):
    """dilations beyond the tile width (the three column taps staged as separate windows) and beyond the image: forward, data
    gradient and weight gradient on both weight-gradient tilings (16- and 32-channel blocks)"""
    _run(be, 1, 12, 40, 32, 32, 33, True, True, seed=33)
    _run(be, 1, 12, 40, 32, 32, 48, True, False, seed=48)
    _run(be, 1, 10, 72, 16, 16, 70, False, True, seed=70)
    _run(be, 1, 8, 16, 4, 16, 100, True, True, seed=100)


def test_dilconv_bad_arguments_are_reported(be):
    N, H, W, Ci, Co = 1, 8, 16, 4, 16
    x, w, y = be.zeros((N, Ci, H, W)), be.zeros((Co, Ci, 3, 3)), be.zeros((N, Co, H, W))
    for d, ks in ((0, 3), (2, 1)):
        with pytest.raises(_lib.WslError):
            be.call("wsl_conv2d_dil_fwd", be.src(x, Ci), be.src(), be.ptr(w), None, be.ptr(y), Co * H * W, N, H, W, Co, ks, d, 0, None,
                    None, be.stream)
    assert be.lib.wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, Ci, Co, 3, 0) == 0
