"""ArenaModule: what every HIP-backed module of this package shares on the Python side of the C ABI.

All parameters are views into ONE flat fp32 arena (so the optimiser and the RCCL all-reduce see a single buffer), gradients and
buffers likewise, and the num_batches_tracked counters are one int64 array.  A subclass describes its state as a list of entries
`(state_dict name, kind, shape, offset)` -- kind 0: parameter (offset into the parameter arena), 1: float buffer (buffer arena),
2: num_batches_tracked (index of the counter) -- in the reference's state_dict order, and keeps only what is its own: its
descriptor, where the entries come from, its mask semantics and its two C calls.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib
from .. import runtime as rt


def c_layout(prefix, desc):
    """(entries, n_param, n_buf) of a network the library enumerates: <prefix>_num_entries / _entry / _param_count / _buffer_count."""
    L = rt.L()
    n_ent = getattr(L, prefix + "_num_entries")(C.byref(desc))
    if n_ent <= 0:
        raise _lib.WslError(L.wsl_last_error().decode())
    entries = []
    for i in range(n_ent):
        e = _lib.WslNetEntry()
        rt.call(prefix + "_entry", C.byref(desc), i, C.byref(e))
        entries.append((e.name.decode(), e.kind, tuple(e.shape[k] for k in range(e.ndim)), e.offset))
    return entries, getattr(L, prefix + "_param_count")(C.byref(desc)), getattr(L, prefix + "_buffer_count")(C.byref(desc))


class ArenaModule(nn.Module):
    _NORM = ("1", "5")     # names of the BatchNorm modules inside their parent (is_norm)
    _MOVED = "model parameters were moved off the GPU / cast away from float32"

    def _build_arenas(self, entries, n_param, n_buf):
        dev = rt.device()
        self._entries, self.n_param = entries, int(n_param)
        # flat arenas (device memory); 64-float padding keeps float4 paths legal for any tail
        self._param_arena = torch.zeros(self.n_param + 64, dtype=torch.float32, device=dev)
        self._grad_arena = torch.zeros(self.n_param + 64, dtype=torch.float32, device=dev)
        self._buf_arena = torch.zeros(n_buf + 64, dtype=torch.float32, device=dev)
        self._nbt = torch.zeros(sum(1 for e in entries if e[1] == 2), dtype=torch.int64, device=dev)
        self._build_tree(entries)
        self._default_init()
        self._fwd_token, self._saved = 0, None
        self._forced_masks = None
        self._last_masks = None
        self._mask_bufs = {}

    # ------------------------------------------------------------------ structure
    def _build_tree(self, entries):
        """Container modules named after the reference's attribute path, so state_dict() keys are identical."""
        self._plist = []
        for name, kind, shape, off in entries:
            *path, leaf = name.split(".")
            m = self
            for part in path:
                if part not in m._modules:
                    m.add_module(part, nn.Module())
                m = m._modules[part]
            n = int(math.prod(shape)) if shape else 1
            if kind == 0:
                p = nn.Parameter(self._param_arena[off:off + n].view(shape))
                m.register_parameter(leaf, p)
                self._plist.append((p, off, n, shape))
            elif kind == 1:
                m.register_buffer(leaf, self._buf_arena[off:off + n].view(shape))
            else:
                m.register_buffer(leaf, self._nbt[off])

    def is_norm(self, name):
        return name.split(".")[-2] in self._NORM

    @torch.no_grad()
    def _default_init(self):
        """nn.Conv2d / nn.ConvTranspose2d / nn.BatchNorm2d default initialisation drawn from torch's global CPU generator in the
        reference's construction order (BatchNorm draws nothing), so `torch.manual_seed(s); net_factory(...)` reproduces the
        reference's initial weights bit for bit (ref: net_factory.py:9-10 builds the module on the CPU, then .cuda()).  A bias is
        U(+-1/sqrt(fan_in)) of the weight before it; torch takes fan_in from dim 1 of a transposed convolution's weight too."""
        fan_in = 1
        for name, kind, shape, off in self._entries:
            n = int(math.prod(shape)) if shape else 1
            if kind == 0 and len(shape) == 4:
                w = torch.empty(shape)
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                self._param_arena[off:off + n].copy_(w.view(-1))
                fan_in = shape[1] * shape[2] * shape[3]
            elif kind == 0 and self.is_norm(name):
                self._param_arena[off:off + n].fill_(1.0 if name.endswith("weight") else 0.0)
            elif kind == 0:
                bound = 1 / math.sqrt(fan_in)
                self._param_arena[off:off + n].copy_(torch.empty(shape).uniform_(-bound, bound))
            elif kind == 1:
                self._buf_arena[off:off + n].fill_(1.0 if name.endswith("running_var") else 0.0)
        self._nbt.zero_()

    def _ensure_arena(self):
        """Re-attach parameters that were re-allocated behind our back (model.to(...), p.data = ..., .double().float())."""
        base = self._param_arena.data_ptr()
        for p, off, n, shape in self._plist:
            if p.data_ptr() != base + 4 * off:
                if p.device != self._param_arena.device or p.dtype != torch.float32:
                    raise _lib.WslError(self._MOVED)
                with torch.no_grad():
                    self._param_arena[off:off + n].copy_(p.data.reshape(-1))
                    p.data = self._param_arena[off:off + n].view(shape)

    # ------------------------------------------------------------------ forward / backward bookkeeping
    def _keep(self, *saved):
        """A training forward ran on the module's workspace: what its backward reads again; older autograd nodes are now stale."""
        self._fwd_token += 1
        self._saved = saved

    def _grad_views(self, private=False):
        """Per-parameter views of the gradient arena.  private: of a clone -- autograd keeps what a node returns as p.grad and later
        ACCUMULATES into it in place, so it never gets the arena the next backward overwrites (the fused TrainEngine reads the arena)."""
        flat = self._grad_arena.clone() if private else self._grad_arena
        return tuple(flat[off:off + n].view(shape) for _, off, n, shape in self._plist)

    def _mask_slot(self, slot, key, make):
        """Persistent mask buffers, refilled in place every forward.  slot: 'train' for a forward whose masks a pending backward will
        read again, 'infer' for every other forward -- two sets, so a no_grad / eval forward between forward and backward cannot
        redraw the saved masks."""
        bufs = self._mask_bufs.get(slot)
        if bufs is None or bufs[0] != key:
            bufs = self._mask_bufs[slot] = (key,) + tuple(make())
        return bufs[1:]

    # flat views for the fused trainer / data-parallel engine
    def flat_params(self):
        self._ensure_arena()
        return self._param_arena[:self.n_param]

    def flat_grads(self):
        return self._grad_arena[:self.n_param]

    def cuda(self, device=None):   # already resident; keep net_factory(...).cuda()-style call sites working
        return self


class _NetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, *params):
        x = rt.f32c(x, "input")     # the kernels address x as dense NCHW: keep the tensor the forward actually read
        outs = mod._run_forward(x, keep_for_backward=True)
        ctx.mod, ctx.x, ctx.token = mod, x, mod._fwd_token
        return outs if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *gouts):
        mod = ctx.mod
        if ctx.token != mod._fwd_token:
            raise _lib.WslError("backward() after a newer training forward of the same module: the activations kept "
                                "in the module's workspace were overwritten (use a second model instance)")
        mod._run_backward(ctx.x, gouts)
        return (None, None) + mod._grad_views(private=True)


class ArenaNet(ArenaModule):
    """A network: one image batch in, one or two logits tensors out.  A training forward is ONE autograd node (_NetFn) around the
    subclass's _run_forward(x, keep_for_backward) -> tuple of logits / _run_backward(x, gouts, phase)."""

    def forward(self, x):
        if x.requires_grad:
            raise NotImplementedError("gradient with respect to the input image is not built (no trainer of the "
                                      "reference's hot path asks for it)")
        if self.training and torch.is_grad_enabled():
            return _NetFn.apply(self, x, *[p for p, _, _, _ in self._plist])
        outs = self._run_forward(x)
        return outs if len(outs) > 1 else outs[0]
