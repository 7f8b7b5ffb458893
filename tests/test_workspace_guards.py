"""Nobody writes outside ws[0 .. ws_bytes): every entry point of the C ABI that takes (ws, ws_bytes), called with EXACTLY the bytes its
own query returns, inside a buffer whose words in front of and behind the workspace hold a fixed bit pattern.

For every case
  * both guard zones (64 Ki floats each: far more than any tile-count formula can overshoot at these shapes, so a failing case
    corrupts nothing and faults nothing, on the emulator or on the device) are untouched after the call;
  * the results are bit-identical to a run on a workspace larger than the query (an entry point that derives addresses from
    ws_bytes must not change its answer with the slack);
  * one byte less than the query returns WSL_EWORKSPACE (a WslError carrying -4 and the two sizes) and writes NOTHING: not into the
    workspace, not into the guards, not into any output.

The shapes are two ordinary ones per entry point plus the narrow / tall / tiny ones that make tile counts diverge from pixel counts:
(H, W) in {(600, 33), (1040, 16), (8, 1024), (1, 700), (700, 1), (600, 3), (1, 1)}, restricted to what an entry point admits."""
import ctypes as C

import numpy as np
import pytest

from wsl4mis_amd import _lib

GUARD = 64 * 1024          # floats on each side: keeps the workspace pointer 256-byte aligned
SLACK = 4096 + 123         # floats added for the "generously oversized" run (odd on purpose)
FILL = 0x5A                # every byte of the buffer and of every output before the call

NARROW = [(600, 33), (1040, 16), (8, 1024), (1, 700), (700, 1), (600, 3), (1, 1)]


def filled(be, shape, dtype=np.float32):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return be.arr(np.full(n, FILL, np.uint8).view(dtype).reshape(shape))


def untouched(be, a):
    return bool(np.all(be.np(a).reshape(-1).view(np.uint8) == FILL))


class Guarded:
    """[guard | ceil(nbytes / 4) floats | guard], all of it filled with the pattern"""

    def __init__(self, be, nbytes):
        self.be, self.n = be, (int(nbytes) + 3) // 4
        self.buf = filled(be, (GUARD + self.n + GUARD,))
        self.ptr = be.ptr(self.buf) + 4 * GUARD
        assert self.ptr % 256 == be.ptr(self.buf) % 256

    def stray(self):
        """(floats changed in front of the workspace, floats changed behind it, distance of the farthest one from the workspace)"""
        w = self.be.np(self.buf).view(np.uint32)
        word = np.uint32(FILL * 0x01010101)
        front, back = np.nonzero(w[:GUARD] != word)[0], np.nonzero(w[GUARD + self.n:] != word)[0]
        far = max([GUARD - int(front.min())] if front.size else [0], [int(back.max()) + 1] if back.size else [0])[0]
        return (int(front.size), int(back.size), far)

    def all_untouched(self):
        return untouched(self.be, self.buf)


def guard_check(be, nbytes, alloc, run):
    """alloc() -> list of fresh pattern-filled output arrays; run(ws_ptr, ws_bytes, outs) makes the call(s)"""
    nbytes = int(nbytes)
    assert nbytes > 0
    res = []
    for slack in (0, SLACK):
        g = Guarded(be, nbytes + 4 * slack)
        outs = alloc()
        run(g.ptr, nbytes + 4 * slack, outs)
        be.sync()
        front, back, far = g.stray()
        assert (front, back) == (0, 0), (f"{front} floats written in front of the workspace, {back} behind ws + ws_bytes (farthest: {far} "
                                         f"floats away); ws_bytes {nbytes + 4 * slack}, query {nbytes}")
        res.append([be.np(o).copy() for o in outs])
    for i, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), f"output {i} changes with the workspace's slack"
    # one byte short: WSL_EWORKSPACE with both sizes, and nothing written anywhere
    g = Guarded(be, nbytes)
    outs = alloc()
    with pytest.raises(_lib.WslError) as ei:
        run(g.ptr, nbytes - 1, outs)
    be.sync()
    msg = str(ei.value)
    assert "-> -4:" in msg and str(nbytes - 1) in msg and str(nbytes) in msg, msg
    assert g.all_untouched(), ("a call that returned WSL_EWORKSPACE wrote", g.stray())
    assert all(untouched(be, o) for o in outs), "a call that returned WSL_EWORKSPACE wrote into an output"
    return res[0]


def _id(case):
    return "-".join(str(v) for v in case)


# ================================================================================================ wsl_loss_ws_bytes
def _logits(rng, shape):
    return (rng.standard_normal(shape) * 2).astype(np.float32)


def _labels(rng, N, H, W, C):
    lab = np.full((N, H, W), C, np.uint8)                       # ignore index = C (the scribble convention)
    m = rng.random((N, H, W)) < 0.2
    lab[m] = rng.integers(0, C, int(m.sum()))
    lab.reshape(-1)[0] = 0                                      # at least one valid pixel
    return lab


def _probs(rng, shape):
    z = rng.standard_normal(shape)
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


# (N, C, H, W): two ordinary shapes, then the narrow ones with the class counts rotated
LOSS_SHAPES = [(2, 4, 40, 44), (3, 3, 17, 23)] + [((1, 2)[i % 2], (3, 4, 8)[i % 3], h, w) for i, (h, w) in enumerate(NARROW)]


def _loss_case(be, entry, N, C, H, W, rng):
    """-> (alloc, run) of one loss entry point at one shape"""
    HW, shape = H * W, (N, C, H, W)
    d = {k: be.arr(v) for k, v in dict(z1=_logits(rng, shape), z2=_logits(rng, shape), lab=_labels(rng, N, H, W, C),
                                       img=rng.random((N, 1, H, W)).astype(np.float32) + 0.05, p=_probs(rng, shape),
                                       pm=_probs(rng, shape)).items()}
    d["lab64"] = be.arr(be.np(d["lab"]).astype(np.int64))
    P = be.ptr
    if entry == "ce":
        return (lambda: [filled(be, (1,)), filled(be, shape)],
                lambda ws, n, o: be.call("wsl_ce_fwd_bwd", P(d["z1"]), P(d["lab"]), 0, C, P(o[0]), P(o[1]), 1.0, N, C, HW, ws, n, be.stream))
    if entry == "pdice":
        return (lambda: [filled(be, (1,)), filled(be, (3 * C,))],
                lambda ws, n, o: be.call("wsl_pdice_fwd", P(d["p"]), P(d["lab64"]), 1, C, P(o[0]), P(o[1]), N, C, HW, ws, n, be.stream))
    if entry in ("head_dual", "head_single"):
        dual = entry == "head_dual"
        return (lambda: [filled(be, (4,)), filled(be, (N, H, W), np.int64), filled(be, shape), filled(be, shape)][:4 if dual else 3],
                lambda ws, n, o: be.call("wsl_head_fwd_bwd", P(d["z1"]), P(d["z2"]) if dual else None, P(d["lab"]), C, 0.37, 0.5, 1.0,
                                         P(o[0]), P(o[1]) if dual else None, P(o[2]), P(o[3]) if dual else None, N, C, HW, ws, n, be.stream))
    if entry.startswith("reg"):
        kind = {"reg_tv": 1, "reg_ms": 2, "reg_entropy": 3}[entry]
        return (lambda: [filled(be, (6,))] + [filled(be, shape) for _ in range(3)],
                lambda ws, n, o: be.call("wsl_head_reg_fwd_bwd", P(d["z1"]), P(d["lab"]), C, 1.0, kind, 0.1, P(d["img"]), P(d["z2"]), 0.07,
                                         P(o[0]), P(o[1]), P(o[2]), P(o[3]), N, C, H, W, ws, n, be.stream))
    if entry == "gatedcrf":
        return (lambda: [filled(be, shape), filled(be, (1,))],
                lambda ws, n, o: be.call("wsl_gatedcrf_fwd", P(d["p"]), P(d["img"]), P(o[0]), P(o[1]), N, C, H, W, 3, 6.0, 0.1, 1.0, ws, n,
                                         be.stream))
    if entry == "tv":
        return (lambda: [filled(be, (1,)), filled(be, shape)],
                lambda ws, n, o: be.call("wsl_tv_fwd_bwd", P(d["p"]), 0, P(o[0]), P(o[1]), 1.0, N, C, H, W, ws, n, be.stream))
    if entry == "ms":
        return (lambda: [filled(be, (1,)), filled(be, shape)],
                lambda ws, n, o: be.call("wsl_mumford_shah_fwd_bwd", P(d["img"]), P(d["p"]), P(o[0]), P(o[1]), 1.0, N, C, H, W, ws, n, be.stream))
    if entry == "mse":
        return (lambda: [filled(be, (1,)), filled(be, shape)],
                lambda ws, n, o: be.call("wsl_softmax_mse_fwd_bwd", P(d["z1"]), P(d["z2"]), P(o[0]), P(o[1]), 1.0, N, C, HW, ws, n, be.stream))
    if entry == "ustm":
        return (lambda: [filled(be, (3,)), filled(be, shape)],
                lambda ws, n, o: be.call("wsl_ustm_consistency_fwd_bwd", P(d["z1"]), P(d["z2"]), P(d["pm"]), 0.8, P(o[0]), P(o[1]), 1.0, N, C,
                                         HW, ws, n, be.stream))
    assert entry == "entropy"
    return (lambda: [filled(be, (1,)), filled(be, shape)],
            lambda ws, n, o: be.call("wsl_entropy_fwd_bwd", P(d["p"]), P(o[0]), P(o[1]), 1.0, N, C, HW, C, ws, n, be.stream))


LOSS_ENTRIES = ["ce", "pdice", "head_dual", "head_single", "reg_tv", "reg_ms", "reg_entropy", "gatedcrf", "tv", "ms", "mse", "ustm", "entropy"]


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=_id)
@pytest.mark.parametrize("entry", LOSS_ENTRIES)
def test_loss_entry_points_stay_inside_their_workspace(be, entry, shape):
    N, C, H, W = shape
    if entry == "reg_tv" and N < 2:
        N = 2                                   # tv_loss(outputs_soft[1:]) needs a batch of at least two
    rng = np.random.default_rng(H * 7 + W + C)
    alloc, run = _loss_case(be, entry, N, C, H, W, rng)
    guard_check(be, be.lib.wsl_loss_ws_bytes(N, C, H * W), alloc, run)


# wsl_head_gatedcrf_fwd_bwd: (N, C, H, W, radius, dual).  Both CRF kernels: the 4-class fast kernel (C = 4, radius 5 | 2, W % 4 == 0; 32 x 32
# tiles) and the generic one (32 x 8 tiles: every other combination).  C = 1 is the class count for which the CRF term of
# wsl_loss_ws_bytes decides the query at every size.  The first block is ordinary shapes, the second the narrow ones: four times as many
# generic-kernel workgroups per pixel as a square image has.
CRF_CASES = [(2, 4, 40, 44, 5, True), (2, 4, 40, 44, 2, False), (2, 4, 40, 44, 3, True), (1, 4, 40, 42, 5, False), (1, 3, 33, 38, 3, True),
             (1, 8, 24, 40, 2, False), (1, 3, 64, 48, 5, False),
             (1, 3, 600, 33, 5, True), (1, 4, 600, 33, 5, False), (1, 8, 600, 33, 2, False), (2, 4, 1040, 16, 3, True),
             (2, 4, 1040, 16, 5, False), (1, 8, 1040, 16, 2, True), (1, 8, 8, 1024, 2, False), (1, 4, 8, 1024, 5, True),
             (1, 3, 8, 1024, 3, False), (1, 3, 1, 700, 2, True), (1, 4, 1, 700, 5, False), (1, 4, 700, 1, 5, False), (1, 8, 700, 1, 3, True),
             (2, 3, 700, 1, 2, False), (1, 1, 700, 1, 5, False), (2, 1, 1040, 16, 3, True), (1, 1, 600, 33, 2, True), (1, 4, 600, 3, 2, True), (1, 3, 600, 3, 5, False), (1, 4, 1, 1, 5, True), (1, 3, 1, 1, 2, False)]


def _crf_head(be, N, C, H, W, r, dual, seed):
    rng = np.random.default_rng(seed)
    shape = (N, C, H, W)
    d = {k: be.arr(v) for k, v in dict(z1=_logits(rng, shape), z2=_logits(rng, shape), lab=_labels(rng, N, H, W, C),
                                       img=rng.random((N, 1, H, W)).astype(np.float32)).items()}
    P = be.ptr

    def alloc():
        return [filled(be, (5,))] + [filled(be, shape) for _ in range(4 if dual else 3)]

    def run(ws, n, o):
        be.call("wsl_head_gatedcrf_fwd_bwd", P(d["z1"]), P(d["z2"]) if dual else None, P(d["lab"]), C, 0.37, P(d["img"]), r, 6.0, 0.1, 1.0,
                0.1, P(o[0]), P(o[1]), P(o[4]) if dual else None, P(o[2]), P(o[3]), N, C, H, W, ws, n, be.stream)

    return alloc, run


@pytest.mark.parametrize("case", CRF_CASES, ids=_id)
def test_fused_head_gatedcrf_stays_inside_its_workspace(be, case):
    N, C, H, W, r, dual = case
    alloc, run = _crf_head(be, N, C, H, W, r, dual, H + W + r)
    out = guard_check(be, be.lib.wsl_loss_ws_bytes(N, C, H * W), alloc, run)
    assert np.all(np.isfinite(out[0])), out[0]


def test_loss_workspace_query_holds_the_worst_aspect_ratio_of_the_crf(be):
    """what the fused head's bound rests on: 2 floats per GatedCRF workgroup (32 x 8 pixel tiles) behind the head's kMaxBlocks * kMaxK
    partials and 64 coefficients, for EVERY factorisation H x W of a pixel count -- the query only knows H * W"""
    for HW in (1, 7, 256, 700, 1024, 16640, 19800, 65536, 262144):
        for N, C in ((1, 1), (1, 4), (2, 8), (64, 4)):
            have = be.lib.wsl_loss_ws_bytes(N, C, HW) // 4 - (1024 * 48 + 64)
            worst = max(-(-w // 32) * -(-(HW // w) // 8) for w in range(1, HW + 1) if HW % w == 0)
            assert have >= 2 * N * worst, (HW, N, C, have, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["crf_dual", "crf_single", "reg_tv", "reg_ms", "reg_entropy"])
def test_full_size_batch_stays_inside_its_workspace_gpu(entry):
    """the bench shape (64 x 4 x 256 x 256, radius 5): the LARGE workspace layout of the fused heads"""
    from conftest import get_backend
    be = get_backend("hip")
    N, C, H, W = 64, 4, 256, 256
    if entry.startswith("crf"):
        alloc, run = _crf_head(be, N, C, H, W, 5, entry == "crf_dual", 5)
    else:
        alloc, run = _loss_case(be, entry, N, C, H, W, np.random.default_rng(6))
    guard_check(be, be.lib.wsl_loss_ws_bytes(N, C, H * W), alloc, run)


# ================================================================================================ convolution weight gradients
def _conv_in(be, rng, N, Ci, Co, H, W):
    x = be.arr(rng.standard_normal((N, Ci, H, W)).astype(np.float32))
    r = be.arr((rng.standard_normal((N, Co, H, W)) * 0.1).astype(np.float32))
    return x, r


# (N, H, W, Ci, Co, ks): the Winograd-eligible shapes with 16-channel blocks, the narrow-operand layers (1 -> 16, 16 -> 4), odd channel
# counts on the narrow / tall / tiny images, 1x1
WGRAD_CASES = [(2, 16, 32, 16, 16, 3), (2, 9, 30, 5, 7, 3), (1, 8, 1024, 16, 16, 3), (1, 1040, 16, 16, 16, 3), (1, 600, 33, 1, 16, 3),
               (1, 600, 33, 16, 4, 3), (1, 1, 700, 5, 7, 3), (1, 700, 1, 5, 7, 3), (2, 600, 3, 5, 7, 3), (1, 1, 1, 5, 7, 3),
               (1, 700, 1, 8, 6, 1), (2, 16, 32, 32, 16, 1), (1, 600, 33, 16, 8, 1)]


@pytest.mark.parametrize("partial", [False, True], ids=["one_call", "partial_plus_batch"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_id)
def test_conv2d_wgrad_stays_inside_its_workspace(be, case, partial):
    N, H, W, Ci, Co, ks = case
    x, r = _conv_in(be, np.random.default_rng(sum(case)), N, Ci, Co, H, W)
    sa = be.src(x, Ci)

    def run(ws, n, o):
        if partial:
            pend = _lib.WslWgradPending()
            be.call("wsl_conv2d_wgrad_partial", sa, be.src(), be.ptr(r), Co * H * W, be.ptr(o[0]), be.ptr(o[1]), N, H, W, Co, ks, ws, n,
                    C.byref(pend), be.stream)
            be.call("wsl_wgrad_reduce_batch", C.byref(pend), 1, be.stream)
        else:
            be.call("wsl_conv2d_wgrad", sa, be.src(), be.ptr(r), Co * H * W, be.ptr(o[0]), be.ptr(o[1]), N, H, W, Co, ks, ws, n, be.stream)

    guard_check(be, be.lib.wsl_conv2d_wgrad_ws_bytes(N, H, W, Ci, Co, ks), lambda: [filled(be, (Co, Ci, ks, ks)), filled(be, (Co,))], run)


# split-precision path: H % 8 == 0, W % 16 == 0, channels % 16 == 0
@pytest.mark.parametrize("case", [(2, 8, 16, 16, 16), (1, 16, 32, 32, 16), (1, 8, 1024, 16, 16), (1, 1040, 16, 16, 16)], ids=_id)
def test_sp_conv2d_wgrad_stays_inside_its_workspace(be, case):
    N, H, W, Ci, Co = case
    rng = np.random.default_rng(sum(case))
    x, r = _conv_in(be, rng, N, Ci, Co, H, W)
    sa = be.src(x, Ci)
    rmax = be.arr(np.full(64, np.abs(be.np(r)).max(), np.float32))
    assert be.lib.wsl_sp_conv2d_ok(sa, be.src(), None, 0, N, H, W, Co, 3) == 1

    def run(ws, n, o):
        pend = _lib.WslWgradPending()
        be.call("wsl_sp_conv2d_wgrad_partial", sa, be.src(), be.ptr(r), Co * H * W, be.ptr(rmax), be.ptr(o[0]), be.ptr(o[1]), N, H, W, Co, ws,
                n, C.byref(pend), be.stream)
        be.call("wsl_wgrad_reduce_batch", C.byref(pend), 1, be.stream)

    guard_check(be, be.lib.wsl_sp_conv2d_wgrad_ws_bytes(N, H, W, Ci, Co), lambda: [filled(be, (Co, Ci, 3, 3)), filled(be, (Co,))], run)


# (N, H, W, Ci, Co, dil): any H, W, dilation
DIL_CASES = [(2, 13, 21, 4, 6, 2), (2, 16, 32, 16, 16, 1), (1, 600, 33, 3, 5, 5), (1, 1040, 16, 16, 16, 2), (1, 8, 1024, 16, 16, 16),
             (1, 1, 700, 3, 5, 3), (1, 700, 1, 3, 5, 2), (2, 600, 3, 3, 5, 8), (1, 1, 1, 3, 5, 1)]


@pytest.mark.parametrize("case", DIL_CASES, ids=_id)
def test_conv2d_dil_wgrad_stays_inside_its_workspace(be, case):
    N, H, W, Ci, Co, dil = case
    x, r = _conv_in(be, np.random.default_rng(sum(case)), N, Ci, Co, H, W)
    sa = be.src(x, Ci)
    guard_check(be, be.lib.wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, Ci, Co, 3, dil), lambda: [filled(be, (Co, Ci, 3, 3)), filled(be, (Co,))],
                lambda ws, n, o: be.call("wsl_conv2d_dil_wgrad", sa, be.src(), be.ptr(r), Co * H * W, be.ptr(o[0]), be.ptr(o[1]), N, H, W, Co,
                                         3, dil, ws, n, be.stream))


# ================================================================================================ BatchNorm backward, upsampling
BN_SHAPES = [(2, 3, 8, 12), (2, 16, 16, 32)] + [((1, 2)[i % 2], (3, 5)[i % 2], h, w) for i, (h, w) in enumerate(NARROW)]


def _bn_in(be, rng, N, Cc, H, W):
    y = rng.standard_normal((N, Cc, H, W)).astype(np.float32)
    v = dict(g=rng.standard_normal((N, Cc, H, W)).astype(np.float32), y=y, mean=y.mean((0, 2, 3)).astype(np.float32),
             invstd=(1.0 / np.sqrt(y.var((0, 2, 3)) + 1e-5)).astype(np.float32), gamma=(rng.random(Cc) + 0.5).astype(np.float32),
             beta=(rng.standard_normal(Cc) * 0.3).astype(np.float32), emask=(rng.random((N, Cc, H, W)) > 0.3).astype(np.uint8))
    return {k: be.arr(a) for k, a in v.items()}


@pytest.mark.parametrize("amax", [False, True], ids=["plain", "amax"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_id)
def test_bnact_bwd_stays_inside_its_workspace(be, shape, amax):
    N, Cc, H, W = shape
    d = _bn_in(be, np.random.default_rng(H + W), N, Cc, H, W)
    P = be.ptr

    def run(ws, n, o):
        args = [P(d["g"]), Cc * H * W, P(d["y"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]), P(d["beta"]), P(d["emask"]), 1.0 / 0.7,
                P(o[0]), P(o[1]), P(o[2]), N, Cc, H, W, ws, n]
        if amax:
            be.call("wsl_bnact_bwd_amax", *args, P(o[3]), be.stream)
        else:
            be.call("wsl_bnact_bwd", *args, be.stream)

    guard_check(be, be.lib.wsl_bnact_bwd_ws_bytes(N, Cc, H, W),
                lambda: [filled(be, shape), filled(be, (Cc,)), filled(be, (Cc,))] + ([filled(be, (64,))] if amax else []), run)


@pytest.mark.parametrize("amax", [False, True], ids=["plain", "amax"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_id)
def test_bnact_bwd_finish_stays_inside_its_workspace(be, shape, amax):
    """stage 2 alone, from the partial sums the fan-in kernel leaves (block-major)"""
    N, Cc, H, W = shape
    d = _bn_in(be, np.random.default_rng(H + W + 1), N, Cc, H, W)
    P = be.ptr
    scale = be.arr(be.np(d["gamma"]) * be.np(d["invstd"]))
    shift = be.arr(be.np(d["beta"]) - be.np(d["mean"]) * be.np(scale))
    f = be.src(d["y"], Cc, scale=scale, shift=shift)
    nblk = be.lib.wsl_feat_grad_combine_blocks(N, H, W)
    part, g = be.zeros((nblk * Cc * 2,)), be.zeros(shape)
    be.call("wsl_feat_grad_combine_bn", f, P(d["g"]), Cc * H * W, None, 0, None, None, P(g), N, H, W, P(d["mean"]), P(d["invstd"]), P(part),
            be.stream)

    def run(ws, n, o):
        args = [P(g), Cc * H * W, P(d["y"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]), P(d["beta"]), None, 1.0, P(o[0]), P(o[1]), P(o[2]),
                N, Cc, H, W, P(part), nblk, 0, ws, n]
        if amax:
            be.call("wsl_bnact_bwd_finish_amax", *args, P(o[3]), be.stream)
        else:
            be.call("wsl_bnact_bwd_finish", *args, be.stream)

    guard_check(be, be.lib.wsl_bnact_bwd_finish_ws_bytes(N, Cc, H, W, int(amax)),
                lambda: [filled(be, shape), filled(be, (Cc,)), filled(be, (Cc,))] + ([filled(be, (64,))] if amax else []), run)


# (N, C, h, w) of the INPUT (the output is 2h x 2w)
# (the forms that do not carry the maximum through the upsampling kernel take it from the source as float4s: N * C * h * w % 4 == 0)
@pytest.mark.parametrize("shape", [(2, 16, 4, 16), (2, 4, 5, 7), (1, 4, 300, 17), (1, 5, 520, 8), (1, 3, 4, 128), (1, 4, 4, 512), (2, 4, 1, 350),
                                   (1, 4, 350, 1), (1, 4, 1, 1)], ids=_id)
def test_bilinear_up2_fwd_amax_stays_inside_its_workspace(be, shape):
    N, Cc, h, w = shape
    u = be.arr(np.random.default_rng(h + w).standard_normal(shape).astype(np.float32))
    slots = []                                    # the caller zeroes the 64 maximum words before the producer runs (include/wsl_hip.h)

    def run(ws, n, o):
        slots.append(be.zeros((64,)))
        be.call("wsl_bilinear_up2_fwd_amax", be.ptr(u), be.ptr(o[0]), Cc * 4 * h * w, N, Cc, h, w, ws, n, be.ptr(slots[-1]), be.stream)

    guard_check(be, be.lib.wsl_bilinear_up2_fwd_amax_ws_bytes(N, Cc, h, w), lambda: [filled(be, (N, Cc, 2 * h, 2 * w))], run)
    assert be.np(slots[0]).view(np.uint32).max() == be.np(slots[1]).view(np.uint32).max() == np.abs(be.np(u)).max().view(np.uint32)
    assert np.all(be.np(slots[2]) == 0)           # the refused call left them alone


# ================================================================================================ transposed-conv UpBlock
@pytest.mark.parametrize("case", [(2, 8, 4, 5, 6), (3, 32, 16, 8, 8), (1, 7, 10, 300, 17), (1, 8, 4, 1, 350), (1, 8, 4, 350, 1), (1, 7, 10, 1, 1)],
                         ids=_id)
def test_convt2x2_wgrad_stays_inside_its_workspace(be, case):
    N, Ci, Co, h, w = case
    rng = np.random.default_rng(sum(case))
    x = be.arr(rng.standard_normal((N, Ci, h, w)).astype(np.float32))
    r = be.arr(rng.standard_normal((N, Co, 2 * h, 2 * w)).astype(np.float32))
    guard_check(be, be.lib.wsl_convt2x2_wgrad_ws_bytes(N, Ci, Co), lambda: [filled(be, (Ci, Co, 2, 2)), filled(be, (Co,))],
                lambda ws, n, o: be.call("wsl_convt2x2_wgrad", be.ptr(x), be.ptr(r), Co * 4 * h * w, be.ptr(o[0]), be.ptr(o[1]), N, Ci, Co, h,
                                         w, ws, n, be.stream))


# (C1, C2, Co, N, h, w, dropout_p)
@pytest.mark.parametrize("case", [(32, 16, 16, 2, 4, 8, 0.0), (8, 4, 6, 1, 3, 5, 0.3), (16, 8, 8, 1, 260, 8, 0.0), (8, 4, 4, 1, 1, 1, 0.5)], ids=_id)
def test_upblock_t_stays_inside_its_workspace(be, case):
    C1, C2, Co, N, h, w, p = case
    rng = np.random.default_rng(int(sum(case[:6])))
    d = _lib.WslUpBlockDesc(C1, C2, Co, N, h, w, p)
    npar = be.lib.wsl_upblock_t_param_count(C.byref(d))
    v = {k: be.arr(a) for k, a in dict(params=(rng.standard_normal(npar) * 0.2).astype(np.float32),
                                       x1=rng.standard_normal((N, C1, h, w)).astype(np.float32),
                                       x2=rng.standard_normal((N, C2, 2 * h, 2 * w)).astype(np.float32),
                                       dout=rng.standard_normal((N, Co, 2 * h, 2 * w)).astype(np.float32),
                                       emask=(rng.random((N, Co, 2 * h, 2 * w)) >= p).astype(np.uint8)).items()}
    P = be.ptr
    pm = P(v["emask"]) if p > 0 else None

    def run(ws, n, o):
        bufs, nbt = be.arr(np.tile(np.array([0.0, 1.0], np.float32), 2 * Co)), be.zeros((2,), np.int64)
        be.call("wsl_upblock_t_forward", C.byref(d), P(v["params"]), P(bufs), P(nbt), P(v["x1"]), P(v["x2"]), pm, 1, P(o[0]), ws, n, be.stream)
        be.call("wsl_upblock_t_backward", C.byref(d), P(v["params"]), P(v["x1"]), P(v["x2"]), pm, P(v["dout"]), P(o[1]), P(o[2]), P(o[3]), ws,
                n, be.stream)
        be.sync()

    guard_check(be, be.lib.wsl_upblock_t_ws_bytes(C.byref(d)),
                lambda: [filled(be, (N, Co, 2 * h, 2 * w)), filled(be, (npar,)), filled(be, (N, C1, h, w)), filled(be, (N, C2, 2 * h, 2 * w))], run)


# ================================================================================================ whole networks
def _unet_case(be, N, H, W, precision, seed):
    from netutil import det_arenas, net_desc, ptr_array
    rng = np.random.default_rng(seed)
    d = net_desc("unet_cct", N, H, W, precision=precision)
    params, bufs, nbt, _ = det_arenas(be.lib, d, 2022)
    dp, x = be.arr(params), be.arr(rng.standard_normal((N, 1, H, W)).astype(np.float32))
    em = [be.arr((rng.random((N, 16 << l, H >> l, W >> l)) >= (0.05, 0.1, 0.2, 0.3, 0.5)[l]).astype(np.uint8)) for l in range(5)]
    cm = [be.arr(((rng.random((N, 16 << l)) >= 0.5) * 2.0).astype(np.float32)) for l in range(5)]
    g1, g2 = (be.arr((rng.standard_normal((N, 4, H, W)) * 0.01).astype(np.float32)) for _ in range(2))
    pem, pcm = ptr_array(be, em), ptr_array(be, cm)
    P = be.ptr

    def run(ws, n, o):
        db, dn = be.arr(bufs), be.arr(nbt)
        be.call("wsl_net_forward", C.byref(d), P(dp), P(db), P(dn), P(x), pem, pcm, 1, P(o[0]), P(o[1]), ws, n, be.stream)
        be.call("wsl_net_backward", C.byref(d), P(dp), P(x), pem, pcm, P(g1), P(g2), P(o[2]), ws, n, 0, be.stream)
        be.sync()

    run.keep = (em, cm)                                         # pem / pcm hold raw addresses
    return be.lib.wsl_net_ws_bytes(C.byref(d)), (lambda: [filled(be, (N, 4, H, W)), filled(be, (N, 4, H, W)), filled(be, params.shape)]), run


@pytest.mark.parametrize("precision", [0, 1], ids=["f32", "split"])
def test_unet_cct_stays_inside_its_workspace(be, precision):
    """forward + backward of unet_cct at 16 x 16 (the size tests/test_net.py runs on the emulator)"""
    guard_check(be, *_unet_case(be, 2, 16, 16, precision, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1], ids=["f32", "split"])
@pytest.mark.parametrize("hw", [(16, 48), (48, 80)], ids=_id)
def test_unet_cct_non_square_stays_inside_its_workspace_gpu(hw, precision):
    """(the emulator needs minutes per non-square forward + backward: GPU only)"""
    from conftest import get_backend
    be = get_backend("hip")
    guard_check(be, *_unet_case(be, 2, hw[0], hw[1], precision, 4))


@pytest.mark.parametrize("hw", [(13, 21), (8, 16)], ids=_id)
def test_pnet_stays_inside_its_workspace(be, hw):
    """forward + backward of the small PNet configuration (3 classes, 16 filters, odd dilations) at an odd size"""
    N, (H, W) = 2, hw
    rng = np.random.default_rng(H + W)
    d = _lib.WslPNetDesc(1, 3, 16, (C.c_int32 * 5)(1, 2, 3, 5, 8), N, H, W)
    npar, nbuf = be.lib.wsl_pnet_param_count(C.byref(d)), be.lib.wsl_pnet_buffer_count(C.byref(d))
    nnbt = 0
    for i in range(be.lib.wsl_pnet_num_entries(C.byref(d))):
        e = _lib.WslNetEntry()
        assert be.lib.wsl_pnet_entry(C.byref(d), i, C.byref(e)) == 0
        nnbt += e.kind == 2
    params = be.arr((rng.standard_normal(npar) * 0.2).astype(np.float32))
    x = be.arr(rng.standard_normal((N, 1, H, W)).astype(np.float32))
    cms = [be.arr(((rng.random((N, c)) >= 0.3) / 0.7).astype(np.float32)) for c in (32, 16)]
    pcm = (C.c_void_p * 2)(*[be.ptr(c) for c in cms])
    dl = be.arr((rng.standard_normal((N, 3, H, W)) * 0.01).astype(np.float32))
    P = be.ptr

    def run(ws, n, o):
        bufs, nbt = be.arr(np.tile(np.array([0.0, 1.0], np.float32), nbuf // 2 + 1)[:nbuf]), be.zeros((max(nnbt, 1),), np.int64)
        be.call("wsl_pnet_forward", C.byref(d), P(params), P(bufs), P(nbt), P(x), pcm, 1, P(o[0]), ws, n, be.stream)
        be.call("wsl_pnet_backward", C.byref(d), P(params), P(x), pcm, P(dl), P(o[1]), ws, n, 0, be.stream)
        be.sync()

    guard_check(be, be.lib.wsl_pnet_ws_bytes(C.byref(d)), lambda: [filled(be, (N, 3, H, W)), filled(be, (npar,))], run)
