"""HIP-backed FCDiscriminator with the reference's module interface (ref: networks/discriminator.py FCDiscriminator, the adversary of
train_deep_adversarial_network_2D.py).

Same constructor arguments `FCDiscriminator(num_classes, ndf=64, n_channel=1)`, same `forward(map, feature)` -> logits [N, 2], same
state_dict keys / shapes / order (conv0, conv1, conv2, conv3, conv4, classifier) and the same initial values under torch.manual_seed,
so reference checkpoints load both ways.  Parameters and gradients are views into flat fp32 arenas (ArenaModule); a forward is ONE
autograd node that enqueues the whole kernel sequence (wsl_dan_forward / wsl_dan_backward: the 4x4 stride-2 convolutions of
csrc/wsl_dan.hip with conv0 + conv1 merged into one pass, LeakyReLU(0.2) and Dropout2d(0.5) inside the consumers' loaders, the pooled
head) and returns gradients for `map` and the parameters -- never for `feature` (the image).

`pool` is this project's one extension: the window of the AvgPool2d in front of the Linear(ndf*32, 2).  It defaults to the reference's 7,
which needs H = W in [224, 336) (or e.g. 112 x 448): the pooled map must have exactly 4 positions.  `pool=1` makes 32 x 32 inputs legal,
so the engine tests can run on the host emulator; nothing else is meant to use it.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib
from .. import runtime as rt
from ._arena import ArenaModule, c_layout

_P_DROP = 0.5          # nn.Dropout2d(0.5) after conv2 and after conv3
GRAD_MAP, GRAD_PARAMS = 1, 2


class _DanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, map_, feature, *params):
        map_, feature = rt.f32c(map_, "map"), rt.f32c(feature, "feature")
        logits, _ = mod._run_forward(map_, feature, keep_for_backward=True)
        ctx.mod, ctx.map, ctx.feature, ctx.token = mod, map_, feature, mod._fwd_token
        return logits

    @staticmethod
    def backward(ctx, g):
        mod = ctx.mod
        if ctx.token != mod._fwd_token:
            raise _lib.WslError("backward() after a newer forward of the same module: the activations kept in the module's "
                                "workspace were overwritten (use a second model instance)")
        flags = (GRAD_MAP if ctx.needs_input_grad[1] else 0) | (GRAD_PARAMS if any(ctx.needs_input_grad[3:]) else 0)
        n = len(mod._plist)
        if not flags:
            return (None, None, None) + (None,) * n
        dmap = mod._run_backward(ctx.map, ctx.feature, rt.f32c(g, "grad_output"), flags)
        grads = mod._grad_views(private=True) if flags & GRAD_PARAMS else (None,) * n
        return (None, dmap, None) + tuple(grads)


class FCDiscriminator(ArenaModule):
    """ref: networks/discriminator.py FCDiscriminator(num_classes, ndf=64, n_channel=1); forward(map, feature) -> logits [N, 2]"""
    _NORM = ()

    def __init__(self, num_classes, ndf=64, n_channel=1, *, pool=7):
        super().__init__()
        self.num_classes, self.ndf, self.n_channel, self.pool = int(num_classes), int(ndf), int(n_channel), int(pool)
        self._build_arenas(*c_layout("wsl_dan", self._desc(1, 0, 0)))

    def _desc(self, N, H, W):
        return _lib.WslDanDesc(self.num_classes, self.n_channel, self.ndf, self.pool, N, H, W, 0)

    @torch.no_grad()
    def _default_init(self):
        """nn.Conv2d / nn.Linear default initialisation drawn from torch's global CPU generator in the reference's construction
        order: every weight kaiming_uniform_(a=sqrt(5)), every bias U(+-1/sqrt(fan_in)) of the weight before it -- the 2-D classifier
        weight included, which the base class would take for a bias."""
        fan_in = 1
        for name, kind, shape, off in self._entries:
            n = int(math.prod(shape))
            if len(shape) >= 2:
                w = torch.empty(shape)
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                fan_in = int(math.prod(shape[1:]))
            else:
                bound = 1 / math.sqrt(fan_in)
                w = torch.empty(shape).uniform_(-bound, bound)
            self._param_arena[off:off + n].copy_(w.view(-1))

    # ------------------------------------------------------------------ Dropout2d masks
    def set_dropout_masks(self, cmasks):
        """Inject the channel multipliers of the two nn.Dropout2d(0.5) sites of the next training forward(s): [m2 [N, 2 ndf] (after
        conv2), m3 [N, 4 ndf] (after conv3)], each 0 or 2 (parity tests replay the reference's); None = draw."""
        self._forced_masks = cmasks

    def _draw_masks(self, N, training, slot):
        if not training:                                   # nn.Dropout2d is the identity in eval()
            return None
        if self._forced_masks is not None:
            return [rt.f32c(m, "dropout mask") for m in self._forced_masks]
        dev = self._param_arena.device
        f = self.ndf
        outs, = self._mask_slot(slot, (N,), lambda: (
            [torch.empty((N, 2 * f), dtype=torch.float32, device=dev), torch.empty((N, 4 * f), dtype=torch.float32, device=dev)],))
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        keep = 1.0 - _P_DROP
        rt.call("wsl_draw_masks", 2, rt.ptr_array(outs), (C.c_int64 * 2)(*[t.numel() for t in outs]), (C.c_float * 2)(keep, keep),
                (C.c_float * 2)(1.0 / keep, 1.0 / keep), (C.c_int * 2)(1, 1), C.c_uint64(seed), rt.stream())
        return outs

    # ------------------------------------------------------------------ execution
    def _run_forward(self, map_, feature, keep_for_backward=False, target=None, gscale=1.0):
        """-> (logits [N, 2], loss [1] or None).  target: int32 [N] in {0, 1} -- the fused head then also computes the cross entropy
        and keeps its gradient (times gscale) in the workspace for _run_backward(dlogits=None)."""
        if map_.dim() != 4 or map_.shape[1] != self.num_classes:
            raise _lib.WslError(f"expected map [N,{self.num_classes},H,W], got {tuple(map_.shape)}")
        N, _, H, W = map_.shape
        if tuple(feature.shape) != (N, self.n_channel, H, W):
            raise _lib.WslError(f"expected feature [{N},{self.n_channel},{H},{W}], got {tuple(feature.shape)}")
        self._ensure_arena()
        d = self._desc(N, H, W)
        nws = rt.L().wsl_dan_ws_bytes(C.byref(d))
        if nws == 0:
            raise _lib.WslError(rt.L().wsl_last_error().decode())
        training = self.training
        slot = "train" if keep_for_backward else "infer"
        ws = rt.workspace(("dan", id(self), slot), nws)
        cm = self._draw_masks(N, training, slot)
        if cm is not None and (tuple(cm[0].shape) != (N, 2 * self.ndf) or tuple(cm[1].shape) != (N, 4 * self.ndf)):
            raise _lib.WslError(f"dropout masks must be [{N},{2 * self.ndf}] and [{N},{4 * self.ndf}]")
        logits = torch.empty((N, 2), dtype=torch.float32, device=map_.device)
        loss = torch.empty((1,), dtype=torch.float32, device=map_.device) if target is not None else None
        if target is not None and (target.dtype != torch.int32 or target.numel() != N or target.device != map_.device):
            raise _lib.WslError("target must be int32 [N] on the engine's device")
        rt.call("wsl_dan_forward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(map_), rt.ptr(feature), rt.ptr_array(cm), int(training),
                rt.ptr(target), C.c_float(gscale), rt.ptr(logits), rt.ptr(loss), rt.ptr(ws), nws, rt.stream())
        self._last_masks = cm
        if keep_for_backward:
            self._keep(d, ws, nws, cm)
        return logits, loss

    def _run_backward(self, map_, feature, dlogits, flags):
        """backward of the forward kept by _run_forward(keep_for_backward=True); dlogits None = the fused head's own gradient.
        -> dmap (or None); with GRAD_PARAMS the gradient arena is overwritten."""
        d, ws, nws, cm = self._saved
        dmap = torch.empty_like(map_) if flags & GRAD_MAP else None
        rt.call("wsl_dan_backward", C.byref(d), rt.ptr(self._param_arena), rt.ptr(map_), rt.ptr(feature), rt.ptr_array(cm), rt.ptr(dlogits),
                flags, rt.ptr(dmap), rt.ptr(self._grad_arena), rt.ptr(ws), nws, rt.stream())
        return dmap

    def forward(self, map, feature):
        if feature.requires_grad:
            raise NotImplementedError("gradient with respect to `feature` (the image) is not built: the trainer differentiates the "
                                      "adversary's loss into `map` only")
        if torch.is_grad_enabled() and (map.requires_grad or any(p.requires_grad for p, _, _, _ in self._plist)):
            return _DanFn.apply(self, map, feature, *[p for p, _, _, _ in self._plist])
        return self._run_forward(rt.f32c(map, "map"), rt.f32c(feature, "feature"))[0]
