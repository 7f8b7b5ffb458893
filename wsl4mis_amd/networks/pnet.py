"""HIP-backed PNet2D with the reference's module interface (ref: networks/pnet.py PNet2D, the DeepIGeoS P-Net).

Same constructor arguments `PNet2D(in_chns, out_chns, num_filters, ratios)`, same forward return (logits [N, out_chns, H, W]), same
state_dict keys / shapes / order (block{1..5}.conv1 / conv2 / in1 / in2, catblock.conv1 / conv2, out.conv1 / conv2) and parameters()
order, so reference checkpoints load both ways.  As for the UNet (networks/unet.py): parameters and buffers are views into flat fp32
arenas, and a forward is one autograd node that enqueues the whole kernel sequence (wsl_pnet_forward / wsl_pnet_backward): the
dilated 3x3 convolutions of the blocks, BatchNorm, the free concat, the 1x1 head.  fp32 only.
"""
import ctypes as C

import torch

from .. import _lib
from .. import runtime as rt
from ._arena import ArenaNet, c_layout

_P_DROP = 0.3   # OutPutBlock's two nn.Dropout2d(0.3)


class PNet2D(ArenaNet):
    """ref: networks/pnet.py PNet2D(in_chns, out_chns, num_filters, ratios) -> logits [N, out_chns, H, W]; any H x W."""
    _n_dec = 1
    PRECISIONS = {"f32": 0}
    _NORM = ("in1", "in2")

    def __init__(self, in_chns, out_chns, num_filters, ratios, conv_precision="f32"):
        super().__init__()
        if conv_precision not in self.PRECISIONS:
            raise NotImplementedError(f"conv_precision {conv_precision!r}: PNet2D is built for fp32 only")
        ratios = [int(r) for r in ratios]
        if len(ratios) != 5:
            raise ValueError(f"PNet2D takes five dilation ratios, got {ratios}")
        self.in_chns, self.out_chns, self.num_filters, self.ratios = int(in_chns), int(out_chns), int(num_filters), ratios
        self.class_num = self.out_chns
        self.conv_precision = conv_precision
        d0 = self._desc(1, 16, 16)
        self._build_arenas(*c_layout("wsl_pnet", d0))
        self.n_enc_param = rt.L().wsl_pnet_block_param_count(C.byref(d0))   # the blocks: the head of the arena (data-parallel buckets)

    def _desc(self, N, H, W):
        return _lib.WslPNetDesc(self.in_chns, self.out_chns, self.num_filters, (C.c_int32 * 5)(*self.ratios), N, H, W)

    # ------------------------------------------------------------------ Dropout2d masks
    def set_dropout_masks(self, cmasks):
        """Inject the channel multipliers of the two nn.Dropout2d(0.3) sites of the next training forward(s): [N, 2F] (before
        out.conv1) and [N, F] (before out.conv2), each 0 or 1/(1-p) (parity tests replay the reference's); None = draw; a callable
        (N, H, W) -> [m1, m2] for masks that depend on the batch shape."""
        self._forced_masks = cmasks

    def _draw_masks(self, N, H, W, training, slot="infer"):
        if not training:                                   # nn.Dropout2d is the identity in eval()
            return None
        if callable(self._forced_masks):
            return list(self._forced_masks(N, H, W))
        if self._forced_masks is not None:
            return list(self._forced_masks)
        dev = self._param_arena.device
        F = self.num_filters
        outs, = self._mask_slot(slot, (N, H, W), lambda: (
            [torch.empty((N, 2 * F), dtype=torch.float32, device=dev), torch.empty((N, F), dtype=torch.float32, device=dev)],))
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        keep = 1.0 - _P_DROP
        rt.call("wsl_draw_masks", 2, rt.ptr_array(outs), (C.c_int64 * 2)(*[t.numel() for t in outs]), (C.c_float * 2)(keep, keep),
                (C.c_float * 2)(1.0 / keep, 1.0 / keep), (C.c_int * 2)(1, 1), C.c_uint64(seed), rt.stream())
        return outs

    # ------------------------------------------------------------------ execution
    def _run_forward(self, x, keep_for_backward=False):
        x = rt.f32c(x, "input")
        if x.dim() != 4 or x.shape[1] != self.in_chns:
            raise _lib.WslError(f"expected input [N,{self.in_chns},H,W], got {tuple(x.shape)}")
        N, _, H, W = x.shape
        self._ensure_arena()
        d = self._desc(N, H, W)
        nws = rt.L().wsl_pnet_ws_bytes(C.byref(d))
        if nws == 0:
            raise _lib.WslError(rt.L().wsl_last_error().decode())
        training = self.training
        grad_mode = training and keep_for_backward
        ws = rt.workspace(("pnet", id(self), "train" if grad_mode else "infer"), nws)
        cm = self._draw_masks(N, H, W, training, "train" if grad_mode else "infer")
        logits = torch.empty((N, self.out_chns, H, W), dtype=torch.float32, device=x.device)
        rt.call("wsl_pnet_forward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(self._buf_arena), rt.ptr(self._nbt), rt.ptr(x),
                rt.ptr_array(cm), int(training), rt.ptr(logits), rt.ptr(ws), nws, rt.stream())
        self._last_masks = cm
        if grad_mode:
            self._keep(d, ws, nws, cm)
        return (logits,)

    def _run_backward(self, x, gouts, phase=0):
        d, ws, nws, cm = self._saved
        g = rt.f32c(gouts[0], "grad_output") if gouts[0] is not None else \
            torch.zeros((d.N, self.out_chns, d.H, d.W), dtype=torch.float32, device=x.device)
        rt.call("wsl_pnet_backward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(x), rt.ptr_array(cm), rt.ptr(g),
                rt.ptr(self._grad_arena), rt.ptr(ws), nws, phase, rt.stream())
        return self._grad_views()

