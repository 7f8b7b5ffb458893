"""HIP-backed UNet / UNet_CCT with the reference's module interface (ref: networks/unet.py:286-303, 327-346).

Same constructor arguments, same forward return ((N,C,H,W) logits, or a pair for UNet_CCT), same state_dict keys /
shapes / order (202 entries for unet_cct) and parameters() order, so reference checkpoints load both ways and
`optim.SGD(model.parameters())`, `loss.backward()`, `model.train()/eval()` work unchanged.

MI355X-first differences of form: all parameters are views into ONE flat fp32 arena (networks/_arena.py), buffers
likewise, and a forward is ONE autograd node that enqueues the whole HIP kernel sequence through the C ABI
(wsl_net_forward / wsl_net_backward) instead of ~150 ATen ops.
"""
import ctypes as C
import math

import torch

from .. import _lib
from .. import runtime as rt
from ._arena import ArenaModule, ArenaNet, c_layout

_FT = (16, 32, 64, 128, 256)
_DROP = (0.05, 0.1, 0.2, 0.3, 0.5)


class _HipUNet(ArenaNet):
    _n_dec = 1
    PRECISIONS = {"f32": 0, "split_f16x3": 1}

    def __init__(self, in_chns, class_num, conv_precision="f32"):
        super().__init__()
        self.in_chns, self.class_num = int(in_chns), int(class_num)
        # "split_f16x3" (opt-in): the 3x3 layers with >= 16 channels on both sides run on the f16 matrix cores with f16 hi / lo
        # operands, three MFMA passes and fp32 accumulation (include/wsl_hip.h, "split-precision conv path"); "f32" is the default
        if conv_precision not in self.PRECISIONS:
            raise ValueError(f"conv_precision {conv_precision!r}: one of {sorted(self.PRECISIONS)}")
        self.conv_precision = conv_precision
        d0 = self._desc(1, 16, 16)
        self._build_arenas(*c_layout("wsl_net", d0))
        self.n_enc_param = rt.L().wsl_net_encoder_param_count(C.byref(d0))

    # ------------------------------------------------------------------ structure
    def _desc(self, N, H, W):
        return _lib.WslNetDesc(self.in_chns, self.class_num, self._n_dec, N, H, W, self.PRECISIONS[self.conv_precision], 0)

    # ------------------------------------------------------------------ masks (host-side RNG = torch's, on the device)
    def set_dropout_masks(self, emasks, cmasks=None):
        """Inject the Bernoulli masks of the next forward(s) (parity tests replay the reference's); None = draw."""
        self._forced_masks = emasks if callable(emasks) else (None if emasks is None and cmasks is None else (emasks, cmasks))

    def _draw_masks(self, N, H, W, training, slot="infer"):
        dev = self._param_arena.device
        if callable(self._forced_masks):                 # (tests) masks that depend on the batch shape of the forward
            em, cm = self._forced_masks(N, H, W)
        elif self._forced_masks is not None:
            em, cm = self._forced_masks
        else:
            em = cm = None
        want_e = training and em is None
        want_c = self._n_dec == 2 and cm is None     # F.dropout2d(x, 0.5) is active in eval mode too (unet.py:254-256,344)
        if want_e or want_c:
            ebufs, cbufs = self._mask_slot(slot, (N, H, W), lambda: (
                [torch.empty((N, _FT[l], H >> l, W >> l), dtype=torch.uint8, device=dev) for l in range(5)],
                [torch.empty((N, _FT[l]), dtype=torch.float32, device=dev) for l in range(5)]))
            outs, probs, scales, isf = [], [], [], []
            if want_e:
                em = ebufs
                outs += em
                probs += [1.0 - p for p in _DROP]
                scales += [1.0] * 5
                isf += [0] * 5
            if want_c:
                cm = cbufs
                outs += cm
                probs += [0.5] * 5
                scales += [2.0] * 5
                isf += [1] * 5
            n = len(outs)
            # the seed comes from torch's (CPU) generator: torch.manual_seed() keeps runs reproducible, no device sync
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            rt.call("wsl_draw_masks", n, rt.ptr_array(outs), (C.c_int64 * n)(*[t.numel() for t in outs]),
                    (C.c_float * n)(*probs), (C.c_float * n)(*scales), (C.c_int * n)(*isf), C.c_uint64(seed), rt.stream())
        return em, cm

    # ------------------------------------------------------------------ execution
    def _run_forward(self, x, keep_for_backward=False):
        x = rt.f32c(x, "input")
        if x.dim() != 4 or x.shape[1] != self.in_chns:
            raise _lib.WslError(f"expected input [N,{self.in_chns},H,W], got {tuple(x.shape)}")
        N, _, H, W = x.shape
        self._ensure_arena()
        d = self._desc(N, H, W)
        nws = rt.L().wsl_net_ws_bytes(C.byref(d))
        if nws == 0:
            raise _lib.WslError(rt.L().wsl_last_error().decode())
        training = self.training
        grad_mode = training and keep_for_backward      # (grad mode is off inside autograd.Function.forward)
        ws = rt.workspace(("net", id(self), "train" if grad_mode else "infer"), nws)
        em, cm = self._draw_masks(N, H, W, training, "train" if grad_mode else "infer")
        lm = torch.empty((N, self.class_num, H, W), dtype=torch.float32, device=x.device)
        la = torch.empty_like(lm) if self._n_dec == 2 else None
        rt.call("wsl_net_forward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(self._buf_arena), rt.ptr(self._nbt),
                rt.ptr(x), rt.ptr_array(em) if training else None, rt.ptr_array(cm), int(training), rt.ptr(lm), rt.ptr(la),
                rt.ptr(ws), nws, rt.stream())
        self._last_masks = (em, cm)
        if grad_mode:
            self._keep(d, ws, nws, em, cm)
        return (lm, la) if la is not None else (lm,)

    def _run_backward(self, x, gouts, phase=0):
        d, ws, nws, em, cm = self._saved
        g = [rt.f32c(t, "grad_output") if t is not None else None for t in gouts]
        if g[0] is None or (self._n_dec == 2 and g[1] is None):
            shape = (d.N, self.class_num, d.H, d.W)
            g = [t if t is not None else torch.zeros(shape, dtype=torch.float32, device=x.device) for t in
                 (g + [None])[:self._n_dec]]
        rt.call("wsl_net_backward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(x), rt.ptr_array(em), rt.ptr_array(cm),
                rt.ptr(g[0]), rt.ptr(g[1]) if self._n_dec == 2 else None, rt.ptr(self._grad_arena), rt.ptr(ws), nws, phase,
                rt.stream())
        return self._grad_views()


class UNet(_HipUNet):
    """ref: networks/unet.py:286-303 (in_chns, class_num) -> logits [N, class_num, H, W]."""
    _n_dec = 1

    def __init__(self, in_chns, class_num, conv_precision="f32"):
        super().__init__(in_chns, class_num, conv_precision)


class UNet_CCT(_HipUNet):
    """ref: networks/unet.py:327-346 (in_chns, class_num) -> (main_seg, aux_seg1); the aux decoder sees
    F.dropout2d(feature, 0.5) of all five encoder features, in train AND eval mode."""
    _n_dec = 2

    def __init__(self, in_chns, class_num, conv_precision="f32"):
        super().__init__(in_chns, class_num, conv_precision)


class _UpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x1, x2, *params):
        x1, x2 = rt.f32c(x1, "x1"), rt.f32c(x2, "x2")     # the dense tensors the kernels read are the ones saved
        out = mod._run_forward(x1, x2, keep=True)
        ctx.mod, ctx.token = mod, mod._fwd_token
        ctx.save_for_backward(x1, x2)
        ctx.need = (x1.requires_grad, x2.requires_grad)
        return out

    @staticmethod
    def backward(ctx, gout):
        mod = ctx.mod
        if ctx.token != mod._fwd_token:
            raise _lib.WslError("backward() after a newer training forward of the same UpBlock (its workspace was overwritten)")
        x1, x2 = ctx.saved_tensors
        dx1, dx2, grads = mod._run_backward(x1, x2, gout, ctx.need)
        return (None, dx1, dx2) + grads


class UpBlock(ArenaModule):
    """ref: networks/unet.py:47-68 -- `UpBlock(in_channels1, in_channels2, out_channels, dropout_p, bilinear=True)`,
    forward(x1, x2).  SURVEY 8f rank 4 (opt-in): the TRANSPOSED-CONVOLUTION branch (`bilinear=False`: ConvTranspose2d(k=2,
    s=2) -> cat([x2, x1]) -> ConvBlock) as a module of its own on the HIP kernels, with the reference's state_dict layout
    (up.weight [C1,C2,2,2], up.bias, conv.conv_conv.{0,1,4,5}.*) and default initialisation draws.  The reference's Decoder
    never selects this branch (it builds every UpBlock with the default bilinear=True -- that path lives inside UNet /
    UNet_CCT), so `bilinear=True` is not offered stand-alone."""
    _MOVED = "UpBlock parameters were moved off the GPU / cast away from float32"

    def __init__(self, in_channels1, in_channels2, out_channels, dropout_p, bilinear=True):
        super().__init__()
        if bilinear:
            raise NotImplementedError("the bilinear UpBlock is built into UNet / UNet_CCT; stand-alone only bilinear=False is")
        self.bilinear = False
        self.c1, self.c2, self.co, self.p = int(in_channels1), int(in_channels2), int(out_channels), float(dropout_p)
        n = rt.L().wsl_upblock_t_param_count(C.byref(self._desc(1, 1, 1)))
        if n <= 0:
            raise _lib.WslError(rt.L().wsl_last_error().decode())
        c1, c2, co = self.c1, self.c2, self.co
        layout = [("up.weight", (c1, c2, 2, 2)), ("up.bias", (c2,)), ("conv.conv_conv.0.weight", (co, 2 * c2, 3, 3)),
                  ("conv.conv_conv.0.bias", (co,)), ("conv.conv_conv.1.weight", (co,)), ("conv.conv_conv.1.bias", (co,)),
                  ("conv.conv_conv.4.weight", (co, co, 3, 3)), ("conv.conv_conv.4.bias", (co,)),
                  ("conv.conv_conv.5.weight", (co,)), ("conv.conv_conv.5.bias", (co,))]
        entries, off = [], 0
        for name, shape in layout:
            entries.append((name, 0, shape, off))
            off += math.prod(shape)
            mod, leaf = name.rsplit(".", 1)
            if leaf == "bias" and self.is_norm(name):               # BatchNorm: its buffers follow its parameters
                bi = 0 if mod.endswith("1") else 1
                entries += [(mod + ".running_mean", 1, (co,), 2 * bi * co), (mod + ".running_var", 1, (co,), (2 * bi + 1) * co),
                            (mod + ".num_batches_tracked", 2, (), bi)]
        assert off == n
        self._build_arenas(entries, n, 4 * co)

    def _desc(self, N, h, w):
        return _lib.WslUpBlockDesc(self.c1, self.c2, self.co, N, h, w, self.p)

    def set_dropout_mask(self, emask):
        """inject the nn.Dropout keep mask [N, Co, 2h, 2w] uint8 of the next forward(s) (parity tests); None = draw"""
        self._forced_masks = emask

    def _run_forward(self, x1, x2, keep=False):
        x1, x2 = rt.f32c(x1, "x1"), rt.f32c(x2, "x2")
        self._ensure_arena()
        N, c1, h, w = x1.shape
        if c1 != self.c1 or tuple(x2.shape) != (N, self.c2, 2 * h, 2 * w):
            raise _lib.WslError(f"UpBlock: x1 {tuple(x1.shape)} / x2 {tuple(x2.shape)} do not fit ({self.c1}, {self.c2})")
        d = self._desc(N, h, w)
        nws = rt.L().wsl_upblock_t_ws_bytes(C.byref(d))
        ws = rt.workspace(("upblock", id(self), "train" if keep else "infer"), nws)
        training = self.training
        em = None
        if training and self.p > 0:
            em = self._forced_masks
            if em is None:
                em = torch.empty((N, self.co, 2 * h, 2 * w), dtype=torch.uint8, device=x1.device)
                seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
                rt.call("wsl_draw_masks", 1, rt.ptr_array([em]), (C.c_int64 * 1)(em.numel()), (C.c_float * 1)(1.0 - self.p),
                        (C.c_float * 1)(1.0), (C.c_int * 1)(0), C.c_uint64(seed), rt.stream())
        out = torch.empty((N, self.co, 2 * h, 2 * w), dtype=torch.float32, device=x1.device)
        rt.call("wsl_upblock_t_forward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(self._buf_arena), rt.ptr(self._nbt),
                rt.ptr(x1), rt.ptr(x2), rt.ptr(em), int(training), rt.ptr(out), rt.ptr(ws), nws, rt.stream())
        if keep:
            self._keep(d, ws, nws, em)
        return out

    def _run_backward(self, x1, x2, gout, need):
        d, ws, nws, em = self._saved
        g = rt.f32c(gout, "grad_output")
        x1, x2 = rt.f32c(x1, "x1"), rt.f32c(x2, "x2")
        dx1 = torch.empty(x1.shape, dtype=torch.float32, device=x1.device) if need[0] else None     # dense, whatever x's strides
        dx2 = torch.empty(x2.shape, dtype=torch.float32, device=x2.device) if need[1] else None
        rt.call("wsl_upblock_t_backward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(x1), rt.ptr(x2), rt.ptr(em), rt.ptr(g),
                rt.ptr(self._grad_arena), rt.ptr(dx1), rt.ptr(dx2), rt.ptr(ws), nws, rt.stream())
        return dx1, dx2, self._grad_views(private=True)

    def forward(self, x1, x2):
        if self.training and torch.is_grad_enabled():
            return _UpFn.apply(self, x1, x2, *[p for p, _, _, _ in self._plist])
        # eval (or no-grad) forward: same convention as UNet / UNet_CCT.forward -- a gradient with respect to an INPUT is refused,
        # otherwise the result comes back without a graph (gradients in eval mode are not built: the backward kernels replay the
        # training-mode BatchNorm); wrap evaluation in torch.no_grad() as the reference's val_2D.py does
        if torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad):
            raise NotImplementedError("UpBlock: gradients in eval mode are not built; call .train() or wrap the forward in torch.no_grad()")
        if torch.is_grad_enabled() and not self.training and not getattr(self, "_warned_eval_grad", False) and \
                any(p.requires_grad for p, _, _, _ in self._plist):
            import warnings     # (a loss computed under .eval() with grad enabled would otherwise fail late or train nothing)
            warnings.warn("UpBlock.forward in eval mode returns a tensor WITHOUT an autograd graph although its parameters require grad: "
                          "parameter gradients in eval mode are not built -- call .train() for training or wrap evaluation in torch.no_grad()",
                          RuntimeWarning, stacklevel=2)
            self._warned_eval_grad = True
        return self._run_forward(x1, x2)
