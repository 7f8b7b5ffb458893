"""Fused training engine: one optimiser step of the reference's 2-D weakly-supervised trainers as a fixed sequence of
C-ABI calls on one HIP stream, data-parallel over the GPUs of a node with RCCL.

Steps reproduced (reference file:line, all under code/):
  'ours_proposed'   train_weakly_supervised_segmentation_pCE_ours_proposed.py:105-132  (unet_cct)
  'pce'             train_weakly_supervised_pCE_2D.py:96-108 (unet) / dual-branch 0.5*(ce1+ce2) (unet_cct, config 1)
  'pce_gatedcrf'    train_weakly_supervised_pCE_GatedCRFLoss_2D.py:108-130 (unet);  unet_cct: 0.5*(ce1+ce2) +
                    0.1*GatedCRF(beta*s1+(1-beta)*s2) as in train_ACDC_scribblevc.py:171-206
  'pce_tv' | 'pce_ms' | 'pce_entropy'   pCE + 1e-2 tv_loss(softmax[1:]) | + 1e-6 MumfordShah(image, softmax) | + 0.1
                    entropy_loss(softmax, 4)  (..._pCE_TV_2D.py:113-114, ..._pCE_MumfordShah_Loss_2D.py:102-103,
                    ..._pCE_Entropy_Mini_2D.py:99-102), unet only
  'ustm'            train_weakly_supervised_ustm_2D.py:119-163: pCE + w(t) * uncertainty-masked consistency against the EMA
                    teacher (T = 8 stochastic teacher passes on the rot90'ed batch), unet only
  'mean_teacher'    SURVEY 8d config 4 (unet student + EMA teacher): pCE + 1e-2*tv_loss(softmax[1:]) (pCE_TV_2D.py:113-114)
                    + w(t)*mean((softmax(s)-softmax(teacher(x+noise)))^2) (train_mean_teacher_2D.py:147-171); teacher =
                    EMA of the student every step (train_weakly_supervised_ustm_2D.py:61-65,163), kept in train mode
  's2l'             train_s2l.py:123-147,214-243 (Scribble2Label; unet | pnet): pCE while it < thr_iter, then pCE + 0.5 * CE on the
                    pseudo labels thresholded from the running prediction average `weight` (step(..., weight=w));
                    update_ensemble(dataset) is that average's refresh, due after every step with it % period_iter == 0
  'pce_interintra'  train_weakly_supervised_pCE_Inter&Intra_Class_2D.py:30-37,112-118 (unet | pnet): pCE + w(t) * (inter_class_variance
                    (softmax, image) - intra_class_variance(softmax, image)), w(t) = var_consistency * sigmoid_rampup(it // 150,
                    var_rampup) with `it` before its increment (var_rampup = 0: the constant weight).  One fused call
                    (wsl_head_reg_fwd_bwd, WSL_REG_CLASS_VAR); fused_heads = False runs the chain head -> softmax ->
                    wsl_class_variance_fwd_bwd -> softmax backward -> axpy.  Zero-variance terms (an all-zero image slice, equal
                    class means) contribute 0 and no gradient, as torch.std does
  'semi_mt' | 'semi_uamt' | 'semi_entmin'   the semi-supervised trainers (unet | pnet): step(x_l, label_l, unlabeled=x_u) runs the
                    student TWICE, as the scripts do -- the labeled half with its own BatchNorm batch statistics, then the unlabeled
                    half with its own -- loss = 0.5 * (CE(z_l, label) + DiceLoss(softmax(z_l), label)) + w(t) * U(z_u), with
                    U = mean((softmax(z_u) - softmax(teacher(x_u + noise)))^2)                  train_mean_teacher_2D.py:147-171
                      | the same distance masked by the teacher's uncertainty (T = 8 stochastic passes, no rot90)
                                                                        train_uncertainty_aware_mean_teacher_2D.py:147-190
                      | entropy_loss(softmax(z_u), 4)                                  train_entropy_minimization_2D.py:130-143
                    and w(t) = consistency * sigmoid_rampup(it // 300, consistency_rampup), `it` before its increment.  The loss is
                    a sum of a term of the first forward and a term of the second, so the step is forward(x_l) -> supervised head ->
                    backward -> keep the gradient arena; forward(x_u) -> unsupervised head -> backward -> add the kept arena: the
                    parameter gradient of the reference's single backward(), BatchNorm running statistics updated in the same order.
                    wsl_sup_head_fwd_bwd / wsl_entropy_logits_fwd_bwd are the fused heads (fused_heads = False: the chains of calls).
                    teacher_update: the reference's two mean-teacher scripts DEFINE update_ema_variables and never call it -- their
                    teacher keeps its initial weights for the whole run.  "frozen" reproduces that literally (a step leaves the
                    teacher's parameter arena bit-unchanged); "ema" (default) places the call as train_weakly_supervised_ustm_2D.py:163
                    does, alpha = min(1 - 1 / (it + 1), ema_decay), which is what the method is
  'semi_dan'        train_deep_adversarial_network_2D.py:135-184 (unet | pnet): the same two student forwards, with
                    U = CE(DAN(softmax(z_u), x_u), t_u), t_u[i] = 1 if i < N_l else 0, DAN = networks/discriminator.py FCDiscriminator in
                    eval mode, and w(t) = consistency * sigmoid_rampup(it // 150, consistency_rampup) -- 150, not 300.  The adversary's
                    loss is differentiated into softmax(z_u) (wsl_dan_backward, data gradient only: the generator update needs none
                    of its weight gradients), then through wsl_softmax_bwd into the student.  After the SGD step,
                    discriminator_step(x_l, x_u): two EVAL forwards of the student (updated weights and running statistics, no
                    gradient), softmax into one (N_l + N_u) batch, the adversary in train mode (Dropout2d drawn or replayed),
                    CE against [1] * N_l + [0] * N_u, parameter gradients only, Adam(dan_lr, dan_betas) (wsl_adam_step)
Optimiser: SGD(lr, momentum 0.9, wd 1e-4) with the poly schedule applied one step late (ours_proposed.py:126-132).

Data parallel (DDP-equivalent semantics): one process per GPU, per-rank BatchNorm statistics and loss
normalisation, gradients averaged.  The flat gradient arena is all-reduced in two buckets on a side stream: the
decoders' slice as soon as the decoder backward has been enqueued (it overlaps the encoder backward), then the
encoder's slice.  Losses stay on the device; `losses()` is the only host sync.
"""
import ctypes as C
import math
import random

import torch
import torch.distributed as dist

from . import _lib
from . import runtime as rt
from .networks.net_factory import net_factory
from .utils.ramps import sigmoid_rampup


class TrainEngine:
    # pCE + weight * regulariser(softmax(outputs)) of the single-branch scripts: (weight, reference lines)
    REGULARISED = ("pce_tv", "pce_ms", "pce_entropy", "ce_dice")
    SEMI = ("semi_mt", "semi_uamt", "semi_entmin", "semi_dan")     # two student forwards per step: step(x_l, label_l, unlabeled=x_u)
    FUSED_REG = {"pce_tv": 1, "pce_ms": 2, "pce_entropy": 3}     # WSL_REG_* of wsl_head_reg_fwd_bwd (include/wsl_hip.h)
    REG_WEIGHT = {"pce_tv": 1e-2,        # train_weakly_supervised_pCE_TV_2D.py:113-114 (tv_loss on outputs_soft[1:])
                  "pce_ms": 1e-6,        # ..._pCE_MumfordShah_Loss_2D.py:102-103 (MumfordShah_Loss(image, softmax))
                  "pce_entropy": 0.1,    # ..._pCE_Entropy_Mini_2D.py:99-102 (entropy_loss(softmax, C=4))
                  "ce_dice": 0.5}        # train_fully_supervised_2D.py:100-102 and ..._pCE_random_walker_2D.py:99-101:
    #                                      0.5 * (CE(outputs, label) + DiceLoss(softmax, label.unsqueeze(1))) on dense labels

    def __init__(self, net_type="unet_cct", in_chns=1, class_num=4, base_lr=0.01, max_iterations=60000, momentum=0.9,
                 weight_decay=1e-4, loss="ours_proposed", w_pse=0.5, crf_radius=5, crf_weight=0.1,
                 crf_desc=None, ignore_index=4, model=None, force_dp=False, conv_precision="f32", thr_iter=6000, thr_conf=0.8,
                 s2l_alpha=0.2, period_iter=100, var_consistency=0.1, var_rampup=200.0, consistency=0.1, consistency_rampup=200.0,
                 ema_decay=0.99, teacher_update="ema", dan_lr=1e-4, dan_betas=(0.9, 0.99), dan_ndf=64, dan_pool=7):
        if loss not in ("ours_proposed", "pce", "pce_gatedcrf", "mean_teacher", "ustm", "s2l", "pce_interintra") + self.REGULARISED + self.SEMI:
            raise NotImplementedError(f"loss composition '{loss}'")
        # conv_precision: "f32" (default, the headline path) | "split_f16x3" (opt-in: networks/unet.py, include/wsl_hip.h)
        self.model = model if model is not None else net_factory(net_type, in_chns, class_num, conv_precision=conv_precision)
        if self.model is None:
            raise _lib.WslError(f"unknown net_type {net_type}")
        self.model.train()
        self.dual = self.model._n_dec == 2
        if loss == "ours_proposed" and not self.dual:
            raise _lib.WslError("'ours_proposed' needs the dual-branch unet_cct")
        if loss in self.REGULARISED and self.dual:
            raise _lib.WslError(f"'{loss}' is a single-branch (unet) composition")
        if loss in ("s2l", "pce_interintra") + self.SEMI and self.dual:
            raise _lib.WslError(f"'{loss}' is a single-decoder composition (unet, pnet)")
        if loss in ("mean_teacher", "ustm") and self.dual:
            raise _lib.WslError(f"'{loss}' is defined for the single-decoder unet")
        if teacher_update not in ("ema", "frozen"):
            raise ValueError(f"teacher_update {teacher_update!r} (one of 'ema', 'frozen')")
        self.loss_kind, self.w_pse, self.ignore = loss, w_pse, ignore_index
        # inter/intra-class variance (..._pCE_Inter&Intra_Class_2D.py:62-70 --consistency / --consistency_rampup, :115 the ramp's argument)
        self.var_consistency, self.var_rampup, self._var_w, self._var_slot = var_consistency, var_rampup, 0.0, 4
        # Scribble2Label (train_s2l.py:62-65): threshold iteration / confidence, EMA weight of the store, update period; w_u: :147
        self.thr_iter, self.thr_conf, self.s2l_alpha, self.period_iter, self.s2l_w_u = thr_iter, thr_conf, s2l_alpha, period_iter, 0.5
        self._s2l_fused, self._patch = False, None
        self.crf_radius, self.crf_weight = crf_radius, crf_weight
        self.crf_desc = crf_desc or {"weight": 1.0, "xy": 6.0, "rgb": 0.1}
        self.base_lr, self.max_it, self.mu, self.wd = base_lr, max_iterations, momentum, weight_decay
        self.lr, self.it = base_lr, 0
        dev = rt.device()
        self.n = self.model.n_param
        self.mom = torch.zeros(self.n + 64, dtype=torch.float32, device=dev)
        self.loss_out = torch.zeros(8, dtype=torch.float32, device=dev)
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # force_dp: take the data-parallel route (split backward, bucketed all-reduce on the side stream) in a 1-rank group too
        self.dp = self.world > 1 or (force_dp and dist.is_available() and dist.is_initialized())
        self.comm = torch.cuda.Stream() if (self.dp and dev.type == "cuda") else None
        if self.world > 1:   # identical start on every rank
            dist.broadcast(self.model._param_arena, src=0)
            dist.broadcast(self.model._buf_arena, src=0)
        self._bufs = {}
        self._diag = None                                  # comm_diag(True): [(event, event)] around the waits for the comm stream
        self.teacher = None
        self._tstream, self._zt = None, None
        self.fused_heads = True                            # regulariser / mean-teacher loss heads through wsl_head_reg_fwd_bwd (False: the chain of calls)
        self.concurrent = True                             # teacher forward on a side stream; set False to serialise
        if loss in ("mean_teacher", "ustm"):
            self.teacher = self._make_teacher(net_type, in_chns, class_num)
            self.tv_weight, self.cons_max, self.ema_decay = 1e-2, 0.1, 0.99
        # semi-supervised trainers (train_mean_teacher_2D.py:60-66 --ema_decay / --consistency / --consistency_rampup, :73-75 the ramp)
        self.consistency, self.consistency_rampup, self.teacher_update = consistency, consistency_rampup, teacher_update
        self._semi_w, self._semi_thr, self._kept = 0.0, 0.0, None
        if loss in ("semi_mt", "semi_uamt"):
            self.teacher = self._make_teacher(net_type, in_chns, class_num)
            self.ema_decay = ema_decay
        self.discriminator = None
        if loss == "semi_dan":
            from .networks.discriminator import FCDiscriminator
            # (train_deep_adversarial_network_2D.py:117-123: FCDiscriminator(num_classes, n_channel = the image's), Adam(1e-4, (0.9, 0.99)))
            self.discriminator = D = FCDiscriminator(class_num, dan_ndf, in_chns, pool=dan_pool)
            self.dan_lr, self.dan_betas, self.dan_eps, self.dan_it = float(dan_lr), (float(dan_betas[0]), float(dan_betas[1])), 1e-8, 0
            self.dan_m = torch.zeros(D.n_param + 64, dtype=torch.float32, device=dev)
            self.dan_v = torch.zeros(D.n_param + 64, dtype=torch.float32, device=dev)
            self._dan_targets = {}
            if self.world > 1:
                dist.broadcast(D._param_arena, src=0)
        if loss == "semi_uamt":
            # measured (profiles/semi_bench.md): at the reference's batch of 6 + 6 the fused supervised head leaves this step 1.9 % slower than
            # the chain against a spread of 0.1 % (1.0 % faster at 32 + 32) -- the one row of six that misses the condition for a fused default
            self.fused_heads = False

    # ------------------------------------------------------------------ helpers
    def _make_teacher(self, net_type, in_chns, class_num):
        """a second network that starts as a copy of the student: parameters and BatchNorm buffers"""
        teacher = net_factory(net_type, in_chns, class_num, conv_precision=self.model.conv_precision)
        teacher.train()                                   # the reference never puts the EMA model in eval()
        with torch.no_grad():
            teacher._param_arena.copy_(self.model._param_arena)
            teacher._buf_arena.copy_(self.model._buf_arena)
        return teacher

    def _tensors(self, N, H, W):
        key = (N, H, W)
        if key not in self._bufs:
            dev, C_ = rt.device(), self.model.class_num
            mk = lambda: torch.empty((N, C_, H, W), dtype=torch.float32, device=dev)  # noqa: E731
            t = {"dz1": mk(), "dz2": mk() if self.dual else None}
            if self.loss_kind == "pce_gatedcrf":
                t["y"], t["msg"] = mk(), mk()
            if self.loss_kind == "ustm":
                t["zr"], t["dzx"], t["pm"] = mk(), mk(), mk()
            if self.loss_kind in self.REGULARISED + ("pce_interintra", "mean_teacher"):     # softmax(z), its gradient, a second dz
                t["s"], t["ds"], t["dzx"] = mk(), mk(), mk()
            self._bufs = {key: t}                         # deliberately ONE shape: a new (N, H, W) drops every buffer kept for the last
        return self._bufs[key]

    def _allreduce(self, flat):
        if self.comm is None:
            dist.all_reduce(flat)
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.comm.wait_event(ev)
        with torch.cuda.stream(self.comm):
            if self._diag is not None:     # per-bucket all-reduce time: HIP events on the COMM stream (torch.cuda.Event times the stream it is recorded on)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(self.comm)
                dist.all_reduce(flat)
                b.record(self.comm)
                self._diag_buckets.append((int(flat.numel()), a, b))
            else:
                dist.all_reduce(flat)

    # ------------------------------------------------------------------ one optimiser step
    def step(self, x, label_u8, beta=0.5, noise=None, weight=None, unlabeled=None, masks=None, dan_masks=None):
        """One optimiser step: forward, loss, backward (+ gradient all-reduce), SGD (+EMA teacher), poly-LR update.
        weight ('s2l'): the loader's [N,H,W,C] batch of the running prediction average; read from `thr_iter` on.
        unlabeled ('semi_*'): the unlabeled image batch x_u (any N, the H x W of x); masks: see forward_backward.
        'semi_dan': then the discriminator's update (discriminator_step; dan_masks replays its two Dropout2d multipliers)."""
        self.forward_backward(x, label_u8, beta, noise, weight, unlabeled, masks)
        self.optimizer_step()
        if self.loss_kind == "semi_dan":
            self.discriminator_step(x, unlabeled, dan_masks)

    def _noisy(self, x, noise, reps=1):
        """x (repeated `reps` times along the batch) + clamp(randn * 0.1, +-0.2) in one library launch (ustm_2D.py:125-127,
        133-135 / train_mean_teacher_2D.py:147-149); `noise`: a tensor to add instead (parity tests replay the reference's)"""
        out = torch.empty((reps * x.shape[0],) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        if noise is not None:
            noise = rt.f32c(noise, "noise")
            if noise.numel() != out.numel():
                raise _lib.WslError(f"noise has {noise.numel()} elements, expected {out.numel()}")
        seed = 0 if noise is not None else int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        rt.call("wsl_noisy_copy", rt.ptr(x), rt.ptr(noise), rt.ptr(out), x.numel(), reps, 0.1, 0.2, C.c_uint64(seed), rt.stream())
        return out

    def _teacher_forward(self, x, noise, reps=1):
        with torch.no_grad():
            return self.teacher._run_forward(self._noisy(x, noise, reps))[0]

    def _start_teacher(self, x, noise):
        """The teacher's forward is independent of the student's: on the GPU it runs on a side stream, forked here (before
        the student forward is enqueued) and joined where its logits are consumed."""
        if x.device.type != "cuda" or not self.concurrent:
            self._zt = None
            return
        if self._tstream is None:
            self._tstream = torch.cuda.Stream(device=x.device)
        cur = torch.cuda.current_stream()
        self._tstream.wait_stream(cur)
        with torch.cuda.stream(self._tstream):
            self._zt = self._teacher_forward(x, noise)
        self._zt.record_stream(cur)

    def _teacher_logits(self, x, noise):
        if self._zt is None:
            return self._teacher_forward(x, noise)
        torch.cuda.current_stream().wait_stream(self._tstream)
        zt, self._zt = self._zt, None
        return zt

    # ------------------------------------------------------------------ the sequences of calls the compositions share
    def _pce_head(self, z, label_u8, dz, w_ce, N, C_, HW, lws, nl):
        """w_ce * pCE(z, label) of ONE decoder: loss_out[0..3], the gradient written to dz"""
        rt.call("wsl_head_fwd_bwd", rt.ptr(z), None, rt.ptr(label_u8), self.ignore, 0.0, 0.0, w_ce, rt.ptr(self.loss_out), None,
                rt.ptr(dz), None, N, C_, HW, rt.ptr(lws), nl, rt.stream())

    def _head_reg(self, z, label_u8, reg_id, w, image, zt, w_cons, t, N, C_, H, W, lws, nl):
        """one call: the head's first pass keeps softmax(z), the regulariser reg_id (WSL_REG_*; `image` where it reads one) turns it into
        its weighted gradient, w_cons * softmax-MSE against the teacher logits zt joins where given, the head's second pass writes dz once"""
        rt.call("wsl_head_reg_fwd_bwd", rt.ptr(z), rt.ptr(label_u8), self.ignore, 1.0, reg_id, w, rt.ptr(image), rt.ptr(zt), w_cons,
                rt.ptr(self.loss_out), rt.ptr(t["dz1"]), rt.ptr(t["s"]), rt.ptr(t["ds"]), N, C_, H, W, rt.ptr(lws), nl, rt.stream())

    def _softmax_term(self, z, t, dz, term, N, C_, HW, add=True):
        """The gradient of a loss term on softmax(z): s = softmax(z) into t["s"]; term(s) enqueues the term and returns the tensor that holds
        its gradient with respect to s; softmax backward -- into t["dzx"] and from there ADDED to dz, or (add=False) straight into dz."""
        rt.call("wsl_softmax_fwd", rt.ptr(z), rt.ptr(t["s"]), N, C_, HW, rt.stream())
        ds = term(t["s"])
        out = t["dzx"] if add else dz
        rt.call("wsl_softmax_bwd", rt.ptr(t["s"]), rt.ptr(ds), rt.ptr(out), N, C_, HW, rt.stream())
        if add:
            rt.call("wsl_axpy", rt.ptr(dz), rt.ptr(out), 1.0, N * C_ * HW, rt.stream())

    def _dice(self, s, label_u8, w, t, N, C_, HW, lws, nl):
        """DiceLoss(s, label) into loss_out[4], w times its gradient with respect to s into t["ds"] (returned)"""
        if "dice" not in t:
            t["dice"] = (torch.empty(3 * C_, dtype=torch.float32, device=s.device), torch.full((1,), w, dtype=torch.float32, device=s.device))
        sums, gout = t["dice"]
        rt.call("wsl_pdice_fwd", rt.ptr(s), rt.ptr(label_u8), 0, -1, rt.ptr(self.loss_out[4:]), rt.ptr(sums), N, C_, HW, rt.ptr(lws), nl, rt.stream())
        rt.call("wsl_pdice_bwd", rt.ptr(s), rt.ptr(label_u8), 0, -1, rt.ptr(sums), rt.ptr(gout), rt.ptr(t["ds"]), N, C_, HW, rt.stream())
        return t["ds"]

    def _mc_teacher_mean(self, x, noises, pm, N, C_, HW):
        """pm = the mean softmax of T = 8 stochastic teacher passes on x + noise, two per double batch (x.repeat(2, 1, 1, 1));
        noises[1:]: the T//2 double-batch noises to replay (None: drawn)"""
        T_ = 8
        for i in range(T_ // 2):
            z2 = self._teacher_forward(x, noises[1 + i] if noises is not None else None, reps=2)
            for h in range(2):
                rt.call("wsl_softmax_accum", rt.ptr(z2[h * N:]), rt.ptr(pm), 1.0 / T_, int(i == 0 and h == 0), N, C_, HW, rt.stream())

    def _regularised_losses(self, x, label_u8, z, t, lws, nl):
        """pCE + weight * R(softmax(z)) with R = tv_loss([1:]) | MumfordShah(image, .) | entropy_loss(., C), and the dense-label
        0.5 * (CE + DiceLoss) of the fully-supervised / random-walker scripts."""
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        HW, C_ = H * W, self.model.class_num
        lo, kind, w = self.loss_out, self.loss_kind, self.REG_WEIGHT[self.loss_kind]
        if kind in self.FUSED_REG and self.fused_heads:
            # (wsl_head_reg_fwd_bwd; the chain below is kept for ce_dice and as the reference of the fused form)
            self._head_reg(z, label_u8, self.FUSED_REG[kind], w, x, None, 0.0, t, N, C_, H, W, lws, nl)
            return
        self._pce_head(z, label_u8, t["dz1"], 0.5 if kind == "ce_dice" else 1.0, N, C_, HW, lws, nl)

        def regulariser(s):
            if kind == "pce_tv":
                rt.call("wsl_tv_fwd_bwd", rt.ptr(s), 1, rt.ptr(lo[4:]), rt.ptr(t["ds"]), w, N, C_, H, W, rt.ptr(lws), nl, rt.stream())
            elif kind == "pce_ms":
                rt.call("wsl_mumford_shah_fwd_bwd", rt.ptr(x), rt.ptr(s), rt.ptr(lo[4:]), rt.ptr(t["ds"]), w, N, C_, H, W,
                        rt.ptr(lws), nl, rt.stream())
            elif kind == "ce_dice":
                return self._dice(s, label_u8, w, t, N, C_, HW, lws, nl)
            else:
                rt.call("wsl_entropy_fwd_bwd", rt.ptr(s), rt.ptr(lo[4:]), rt.ptr(t["ds"]), w, N, C_, HW, C_, rt.ptr(lws), nl, rt.stream())
            return t["ds"]
        self._softmax_term(z, t, t["dz1"], regulariser, N, C_, HW)

    def var_weight(self, it=None):
        """w(t) of 'pce_interintra': get_current_consistency_weight(iter_num // 150) of the trainer (lines 68-70, 115)"""
        return self.var_consistency * sigmoid_rampup((self.it if it is None else it) // 150, self.var_rampup)

    def _interintra_losses(self, x, label_u8, z, t, lws, nl):
        """pCE + w(t) * (inter_class_variance(softmax, image) - intra_class_variance(softmax, image))"""
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        HW, C_ = H * W, self.model.class_num
        if x.shape[1] != 1:
            raise NotImplementedError("the class-variance terms are built for a single-channel image")
        w = self._var_w = self.var_weight()
        if self.fused_heads:      # out[4] = inter - intra, out[6] = inter, out[7] = intra
            self._var_slot = 4
            self._head_reg(z, label_u8, 4, w, x, None, 0.0, t, N, C_, H, W, lws, nl)
            return
        self._var_slot = 5        # the stand-alone entry point writes {inter - intra, inter, intra} contiguously: slots 5, 6, 7
        self._pce_head(z, label_u8, t["dz1"], 1.0, N, C_, HW, lws, nl)

        def class_variance(s):
            rt.call("wsl_class_variance_fwd_bwd", rt.ptr(x), rt.ptr(s), rt.ptr(self.loss_out[5:]), rt.ptr(t["ds"]), w, -w, N, C_, H, W,
                    rt.ptr(lws), nl, rt.stream())
            return t["ds"]
        self._softmax_term(z, t, t["dz1"], class_variance, N, C_, HW)

    def _ustm_losses(self, x, label_u8, z, t, noise, lws, nl):
        """train_weakly_supervised_ustm_2D.py:119-157: pCE + w(t) * uncertainty-masked consistency.  `noise`: None (drawn
        like the script) or a list of T//2 + 1 tensors (teacher input noise, then the T//2 double-batch noises)."""
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        HW, C_ = H * W, self.model.class_num
        if H != W:
            raise _lib.WslError("ustm rotates the batch by multiples of 90 degrees: square inputs only")
        self._pce_head(z, label_u8, t["dz1"], 1.0, N, C_, HW, lws, nl)
        k = random.randrange(0, 4)                            # ustm_2D.py:121 (the script's only python-RNG draw per step)
        xr = torch.empty_like(x)
        rt.call("wsl_rot90", rt.ptr(x), rt.ptr(xr), N * x.shape[1], H, W, k, rt.stream())
        zt = self._teacher_forward(xr, noise[0] if noise is not None else None)
        self._mc_teacher_mean(xr, noise, t["pm"], N, C_, HW)
        self._cons_w = 1.0 * sigmoid_rampup(self.it // 1000, 60)      # ustm_2D.py:56-58,146: get_current_consistency_weight(iter // 1000)
        thr = self.uncertainty_threshold()
        rt.call("wsl_rot90", rt.ptr(z), rt.ptr(t["zr"]), N * C_, H, W, k, rt.stream())
        rt.call("wsl_ustm_consistency_fwd_bwd", rt.ptr(t["zr"]), rt.ptr(zt), rt.ptr(t["pm"]), float(thr), rt.ptr(self.loss_out[4:]),
                rt.ptr(t["dzx"]), self._cons_w, N, C_, HW, rt.ptr(lws), nl, rt.stream())
        rt.call("wsl_rot90", rt.ptr(t["dzx"]), rt.ptr(t["zr"]), N * C_, H, W, 4 - k, rt.stream())    # gradient back through rot90
        rt.call("wsl_axpy", rt.ptr(t["dz1"]), rt.ptr(t["zr"]), 1.0, N * C_ * HW, rt.stream())

    def _mean_teacher_losses(self, x, label_u8, z, t, noise, lws, nl):
        """dz of pCE + tv + consistency for the student logits z; teacher logits from x + noise (no gradient)."""
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        HW, C_ = H * W, self.model.class_num
        zt = self._teacher_logits(x, noise)                # usually already in flight on the side stream
        lo = self.loss_out
        self._cons_w = self.cons_max * sigmoid_rampup(self.it // 300, 200.0)
        if self.fused_heads:      # pCE + tv_weight * TV(softmax[1:]) + w(t) * softmax-MSE(student, teacher): one call, dz written once
            self._head_reg(z, label_u8, 1, self.tv_weight, None, zt, self._cons_w, t, N, C_, H, W, lws, nl)
            return
        self._pce_head(z, label_u8, t["dz1"], 1.0, N, C_, HW, lws, nl)

        def tv(s):
            rt.call("wsl_tv_fwd_bwd", rt.ptr(s), 1, rt.ptr(lo[4:]), rt.ptr(t["ds"]), self.tv_weight, N, C_, H, W, rt.ptr(lws), nl,
                    rt.stream())
            return t["ds"]
        self._softmax_term(z, t, t["dz1"], tv, N, C_, HW)
        rt.call("wsl_softmax_mse_fwd_bwd", rt.ptr(z), rt.ptr(zt), rt.ptr(lo[5:]), rt.ptr(t["dzx"]), self._cons_w, N, C_, HW,
                rt.ptr(lws), nl, rt.stream())
        rt.call("wsl_axpy", rt.ptr(t["dz1"]), rt.ptr(t["dzx"]), 1.0, N * C_ * HW, rt.stream())

    def forward_backward(self, x, label_u8, beta=0.5, noise=None, weight=None, unlabeled=None, masks=None):
        """Everything up to (and including) the gradient all-reduce; flat_grads() then holds the SUM over ranks.
        'semi_*': x / label_u8 are the labeled half, `unlabeled` the unlabeled image batch; noise: None (drawn like the scripts) or
        the teacher's input noise -- a tensor ('semi_mt') / a list of 1 + T//2 tensors ('semi_uamt': the teacher input's, then the
        four double batches'); masks = (m_l, m_u) replays dropout masks for the two student forwards, each entry what the model's
        set_dropout_masks takes (a tuple for several arguments)."""
        if self.loss_kind in self.SEMI:
            if unlabeled is None:
                raise _lib.WslError(f"'{self.loss_kind}' needs step(x_l, label_l, unlabeled=x_u): the unlabeled image batch")
            return self._semi_forward_backward(x, label_u8, unlabeled, noise, masks)
        if unlabeled is not None or masks is not None:
            raise _lib.WslError(f"unlabeled= / masks= belong to the semi-supervised compositions {self.SEMI}, not to '{self.loss_kind}'")
        m = self.model
        x = rt.f32c(x, "image batch")
        N, _, H, W = x.shape
        HW = H * W
        t = self._tensors(N, H, W)
        m.train()
        self._patch = (H, W)
        if self.loss_kind == "mean_teacher":
            self._start_teacher(x, noise)
        outs = m._run_forward(x, keep_for_backward=True)
        z1, z2 = outs[0], (outs[1] if self.dual else None)
        nl = rt.L().wsl_loss_ws_bytes(N, m.class_num, HW)
        lws = rt.workspace("loss", nl)      # the one loss workspace of the step: every composition below gets it passed down
        if self.loss_kind == "mean_teacher":
            self._mean_teacher_losses(x, label_u8, z1, t, noise, lws, nl)
        elif self.loss_kind == "ustm":
            self._ustm_losses(x, label_u8, z1, t, noise, lws, nl)
        elif self.loss_kind in self.REGULARISED:
            self._regularised_losses(x, label_u8, z1, t, lws, nl)
        elif self.loss_kind == "pce_interintra":
            self._interintra_losses(x, label_u8, z1, t, lws, nl)
        elif self.loss_kind == "s2l" and self.it >= self.thr_iter:      # train_s2l.py:125-147 (iter_num before its increment)
            if weight is None:
                raise _lib.WslError(f"'s2l' from thr_iter = {self.thr_iter} on needs step(..., weight=the loader's weight batch)")
            weight = rt.f32c(weight, "weight batch")
            if tuple(weight.shape) != (N, H, W, m.class_num):
                raise _lib.WslError(f"weight batch {tuple(weight.shape)}, expected channels-last {(N, H, W, m.class_num)}")
            ns = rt.L().wsl_s2l_head_ws_bytes(N, m.class_num, HW)
            rt.call("wsl_s2l_head_fwd_bwd", rt.ptr(z1), rt.ptr(label_u8), rt.ptr(weight), self.ignore, float(self.thr_conf),
                    self.s2l_w_u, 1.0, rt.ptr(self.loss_out), None, rt.ptr(t["dz1"]), N, m.class_num, HW,
                    rt.ptr(rt.workspace("s2l_head", ns)), ns, rt.stream())
        elif self.loss_kind == "pce_gatedcrf":            # pCE + crf_weight * GatedCRF(y): one fused entry point
            d = self.crf_desc
            rt.call("wsl_head_gatedcrf_fwd_bwd", rt.ptr(z1), rt.ptr(z2), rt.ptr(label_u8), self.ignore, float(beta), rt.ptr(x),
                    self.crf_radius, d["xy"], d["rgb"], d["weight"], self.crf_weight, rt.ptr(self.loss_out), rt.ptr(t["dz1"]),
                    rt.ptr(t["dz2"]), rt.ptr(t["y"]), rt.ptr(t["msg"]), N, m.class_num, H, W, rt.ptr(lws), nl, rt.stream())
        else:
            w_pse = self.w_pse if self.loss_kind == "ours_proposed" else 0.0
            rt.call("wsl_head_fwd_bwd", rt.ptr(z1), rt.ptr(z2), rt.ptr(label_u8), self.ignore, float(beta), w_pse, 1.0,
                    rt.ptr(self.loss_out), None, rt.ptr(t["dz1"]), rt.ptr(t["dz2"]), N, m.class_num, HW, rt.ptr(lws), nl,
                    rt.stream())
        self._s2l_fused = self.loss_kind == "s2l" and self.it >= self.thr_iter
        self._finish_backward(x, t)

    # ------------------------------------------------------------------ semi-supervised: two student forwards per step
    def consistency_weight(self, it=None):
        """w(t) of the 'semi_*' compositions: get_current_consistency_weight(iter_num // 300) (train_mean_teacher_2D.py:73-75, 164-165)
        -- iter_num // 150 for 'semi_dan' (train_deep_adversarial_network_2D.py:153); consistency_rampup = 0: the constant weight"""
        div = 150 if self.loss_kind == "semi_dan" else 300
        return self.consistency * sigmoid_rampup((self.it if it is None else it) // div, self.consistency_rampup)

    def uncertainty_threshold(self, it=None):
        """(0.75 + 0.25 * sigmoid_rampup(iter_num, max_iterations)) * ln 2 (train_uncertainty_aware_mean_teacher_2D.py:184-185)"""
        return (0.75 + 0.25 * sigmoid_rampup(self.it if it is None else it, self.max_it)) * math.log(2.0)

    def _set_masks(self, mk):
        m = self.model
        m.set_dropout_masks(*mk) if isinstance(mk, tuple) else m.set_dropout_masks(mk)

    def _sup_head(self, z, label_u8, dz, t, N, C_, HW):
        """0.5 * (CE(z, label) + DiceLoss(softmax(z), label)) of the labeled half: loss_out[0..3] = {sup, ce, dice, n_valid}"""
        lo = self.loss_out
        nl = rt.L().wsl_loss_ws_bytes(N, C_, HW)
        lws = rt.workspace("loss", nl)
        if self.fused_heads:
            rt.call("wsl_sup_head_fwd_bwd", rt.ptr(z), rt.ptr(label_u8), self.ignore, 0.5, 0.5, 1.0, rt.ptr(lo), rt.ptr(dz), N, C_, HW,
                    rt.ptr(lws), nl, rt.stream())
            return
        # the chain `ce_dice` runs: head (0.5 * CE), softmax, DiceLoss forward / backward, softmax backward, axpy; the Dice value lands in
        # loss_out[4] and moves to slot 2 (the head's unused `pse`), so both routes leave the same layout
        self._pce_head(z, label_u8, dz, 0.5, N, C_, HW, lws, nl)
        self._softmax_term(z, t, dz, lambda s: self._dice(s, label_u8, 0.5, t, N, C_, HW, lws, nl), N, C_, HW)
        lo[2:3].copy_(lo[4:5])      # (slot 0 holds the head's plain CE on this route: losses() forms sup from ce and dice on both)

    def _semi_tensors(self, N, H, W, which):
        key = ("semi", which, N, H, W)
        if key not in self._bufs:
            dev, C_ = rt.device(), self.model.class_num
            mk = lambda: torch.empty((N, C_, H, W), dtype=torch.float32, device=dev)  # noqa: E731
            t = {"dz": mk(), "mk": mk}
            if which == "u" and self.loss_kind == "semi_uamt":
                t["pm"] = mk()
            if which == "u" and self.loss_kind == "semi_dan":
                t["s"] = mk()                             # softmax(z_u): the adversary's `map`
            self._bufs[key] = t
        t = self._bufs[key]
        chain = not self.fused_heads and (which == "l" or self.loss_kind == "semi_entmin")
        if chain and "s" not in t:                        # the chains of calls keep softmax(z) and its gradient
            t["s"], t["ds"], t["dzx"] = t["mk"](), t["mk"](), t["mk"]()
        return t

    def _semi_forward_backward(self, x, label_u8, xu, noise, masks):
        """forward(x_l) -> supervised head -> backward -> keep the arena; forward(x_u) -> unsupervised head -> backward -> add the kept
        arena.  loss_out: [0..3] = {sup, ce, dice, n_valid}, [4] = the raw unsupervised term, [5] = sum(mask) ('semi_uamt')."""
        m, kind = self.model, self.loss_kind
        x, xu = rt.f32c(x, "image batch"), rt.f32c(xu, "unlabeled image batch")
        if xu.dim() != 4 or x.dim() != 4 or tuple(xu.shape[1:]) != tuple(x.shape[1:]):
            raise _lib.WslError(f"labeled batch {tuple(x.shape)} and unlabeled batch {tuple(xu.shape)} may differ in N only")
        if masks is not None and len(masks) != 2:
            raise _lib.WslError("masks = (m_l, m_u): one entry per student forward")
        N, _, H, W = x.shape
        Nu, HW, C_ = xu.shape[0], H * W, m.class_num
        tl, tu = self._semi_tensors(N, H, W, "l"), self._semi_tensors(Nu, H, W, "u")
        lo = self.loss_out
        m.train()
        self._patch = (H, W)
        n0 = noise if (noise is None or torch.is_tensor(noise)) else noise[0]
        if kind == "semi_uamt" and noise is not None and (torch.is_tensor(noise) or len(noise) != 5):
            raise _lib.WslError("'semi_uamt' replays 1 + T//2 = 5 noise tensors: the teacher input's, then the four double batches'")
        if self.teacher is not None:
            self._start_teacher(xu, n0)
        try:
            # ---- the labeled half
            if masks is not None:
                self._set_masks(masks[0])
            z_l = m._run_forward(x, keep_for_backward=True)[0]
            self._sup_head(z_l, label_u8, tl["dz"], tl, N, C_, HW)
            m._run_backward(x, [tl["dz"], None], phase=0)
            flat_g = m.flat_grads()
            if self._kept is None or self._kept.numel() != flat_g.numel() or self._kept.device != flat_g.device:
                self._kept = torch.empty_like(flat_g)
            self._kept.copy_(flat_g)                      # wsl_net_backward OVERWRITES the arena
            # ---- the unlabeled half
            if masks is not None:
                self._set_masks(masks[1])
            z_u = m._run_forward(xu, keep_for_backward=True)[0]
        finally:
            if masks is not None:
                m.set_dropout_masks(None)
        w = self._semi_w = self.consistency_weight()
        nl = rt.L().wsl_loss_ws_bytes(Nu, C_, HW)
        lws = rt.workspace("loss", nl)
        if kind == "semi_entmin":
            if self.fused_heads:
                rt.call("wsl_entropy_logits_fwd_bwd", rt.ptr(z_u), rt.ptr(lo[4:]), rt.ptr(tu["dz"]), w, Nu, C_, HW, 4, rt.ptr(lws), nl, rt.stream())
            else:
                def entropy(s):
                    rt.call("wsl_entropy_fwd_bwd", rt.ptr(s), rt.ptr(lo[4:]), rt.ptr(tu["ds"]), w, Nu, C_, HW, 4, rt.ptr(lws), nl, rt.stream())
                    return tu["ds"]
                self._softmax_term(z_u, tu, tu["dz"], entropy, Nu, C_, HW, add=False)
        elif kind == "semi_dan":
            # w * CE(DAN(softmax(z_u), x_u), t_u): the adversary in eval mode, its loss differentiated into softmax(z_u) only (no weight
            # gradient: the reference discards them), the weight w folded into the head's gradient scale
            D, adv = self.discriminator, None
            D.eval()

            def adversary(s):                             # -> the data gradient its backward returns
                nonlocal adv
                _, adv = D._run_forward(s, xu, keep_for_backward=True, target=self._dan_target(N, Nu, False), gscale=float(w))
                return D._run_backward(s, xu, None, 1)
            self._softmax_term(z_u, tu, tu["dz"], adversary, Nu, C_, HW, add=False)
            lo[4:5].copy_(adv)
        elif kind == "semi_mt":
            zt = self._teacher_logits(xu, n0)             # usually already in flight on the side stream
            rt.call("wsl_softmax_mse_fwd_bwd", rt.ptr(z_u), rt.ptr(zt), rt.ptr(lo[4:]), rt.ptr(tu["dz"]), w, Nu, C_, HW, rt.ptr(lws), nl, rt.stream())
        else:
            zt = self._teacher_logits(xu, n0)             # joins the side stream: the passes below reuse the teacher's workspace
            self._mc_teacher_mean(xu, noise, tu["pm"], Nu, C_, HW)
            thr = self._semi_thr = self.uncertainty_threshold()
            rt.call("wsl_ustm_consistency_fwd_bwd", rt.ptr(z_u), rt.ptr(zt), rt.ptr(tu["pm"]), float(thr), rt.ptr(lo[4:]), rt.ptr(tu["dz"]), w,
                    Nu, C_, HW, rt.ptr(lws), nl, rt.stream())
        self._finish_backward(xu, {"dz1": tu["dz"], "dz2": None}, kept=self._kept)

    # ------------------------------------------------------------------ DAN: the adversary's own update
    def _dan_target(self, n_l, n_u, both):
        """both: DAN_target = [1] * N_l + [0] * N_u (train_deep_adversarial_network_2D.py:138-140); else its first N_u entries, the
        generator update's target (line 152) -- all ones while N_u <= N_l, kept literal beyond"""
        key = (n_l, n_u, both)
        if key not in self._dan_targets:
            full = [1] * n_l + [0] * n_u
            self._dan_targets[key] = torch.tensor(full if both else full[:n_u], dtype=torch.int32, device=rt.device())
        return self._dan_targets[key]

    def discriminator_step(self, x_l, x_u, masks=None):
        """The second half of a 'semi_dan' step (train_deep_adversarial_network_2D.py:162-176), after optimizer_step(): the student in
        eval mode without gradient on both halves, softmax, the adversary in train mode on the concatenation, CE against
        [1] * N_l + [0] * N_u, its parameter gradients only (conv0's data gradient is skipped), all-reduced as one bucket under data
        parallelism, Adam.  masks = [m2 [N, 2 ndf], m3 [N, 4 ndf]] replays the two Dropout2d multipliers (0 or 2); None = drawn.
        Leaves the student's parameters, gradient arena, BatchNorm running statistics and num_batches_tracked untouched."""
        if self.loss_kind != "semi_dan":
            raise _lib.WslError("discriminator_step belongs to the 'semi_dan' composition")
        m, D = self.model, self.discriminator
        x_l, x_u = rt.f32c(x_l, "image batch"), rt.f32c(x_u, "unlabeled image batch")
        N, Nu, H, W, C_ = x_l.shape[0], x_u.shape[0], x_l.shape[2], x_l.shape[3], m.class_num
        key = ("dan", N + Nu, H, W)
        if key not in self._bufs:
            self._bufs[key] = torch.empty((N + Nu, C_, H, W), dtype=torch.float32, device=x_l.device)
        s = self._bufs[key]
        m.eval()
        try:
            with torch.no_grad():
                z_l = m._run_forward(x_l)[0]
                rt.call("wsl_softmax_fwd", rt.ptr(z_l), rt.ptr(s), N, C_, H * W, rt.stream())
                z_u = m._run_forward(x_u)[0]
                rt.call("wsl_softmax_fwd", rt.ptr(z_u), rt.ptr(s[N:]), Nu, C_, H * W, rt.stream())
        finally:
            m.train()
        xcat = torch.cat([x_l, x_u], 0)
        D.train()
        if masks is not None:
            D.set_dropout_masks(masks)
        try:
            _, dl = D._run_forward(s, xcat, keep_for_backward=True, target=self._dan_target(N, Nu, True), gscale=1.0)
        finally:
            if masks is not None:
                D.set_dropout_masks(None)
        D._run_backward(s, xcat, None, 2)
        if self.dp:
            self._allreduce(D.flat_grads())
            if self.comm is not None:
                torch.cuda.current_stream().wait_stream(self.comm)
        self.dan_it += 1
        rt.call("wsl_adam_step", rt.ptr(D._param_arena), rt.ptr(D._grad_arena), rt.ptr(self.dan_m), rt.ptr(self.dan_v), D.n_param,
                self.dan_lr, self.dan_betas[0], self.dan_betas[1], self.dan_eps, self.dan_it, 1.0 / self.world, rt.stream())
        self.loss_out[5:6].copy_(dl)

    # ------------------------------------------------------------------ Scribble2Label: the running prediction average
    def ensemble_due(self):
        """train_s2l.py:214: after a step, `iter_num > 0 and iter_num % period_iter == 0` (iter_num already incremented)"""
        return self.it > 0 and self.it % self.period_iter == 0

    def update_ensemble(self, dataset, mode="reference", masks=None, patch_size=None, batch_size=32):
        """Refresh the `weight` store of every slice of `dataset` (a BaseDataSets_s2l) from the current model
        (ref: train_s2l.py:214-243): image zoomed with order 0 to the patch size, pred = softmax(model(image)), pred zoomed back
        with order 0 to the slice's native size, weight = alpha * pred + (1 - alpha) * weight in fp32.

        mode="reference": what the reference does, literally -- its model is in train() mode during this pass, so every slice is
        ONE forward at N = 1 whose BatchNorm layers normalise by the slice's own statistics, whose running statistics take a
        momentum update per slice, and whose dropout is live (drawn by the library; `masks`: a list with one entry per slice --
        what the model's set_dropout_masks takes, a tuple for several arguments -- replays recorded masks in parity tests).
        mode="eval": NOT what the reference does -- an opt-in departure: eval-mode forwards in batches of `batch_size`, no dropout,
        BatchNorm from the running statistics, which stay untouched (as do all parameters and buffers).
        patch_size: (H, W) of the network input; default: the last step's, else 256 x 256 (the reference hard-codes 256).
        With several ranks every rank keeps and updates its own full store; there is no collective in this pass."""
        if mode not in ("reference", "eval"):
            raise ValueError(f"update_ensemble: mode {mode!r} (one of 'reference', 'eval')")
        m, dev = self.model, rt.device()
        Hn, Wn = patch_size or self._patch or (256, 256)
        C_, n_all = m.class_num, len(dataset)
        if masks is not None and (mode != "reference" or len(masks) != n_all):
            raise _lib.WslError("update_ensemble: masks replay the reference-mode forwards, one entry per slice")
        chunk = 64 if mode == "reference" else max(1, int(batch_size))      # slices per zoom launch / ensemble launch
        was_training = m.training
        m.train(mode == "reference")
        try:
            with torch.no_grad():
                for b0 in range(0, n_all, chunk):
                    idxs = list(range(b0, min(b0 + chunk, n_all)))
                    n = len(idxs)
                    aug = (_lib.WslAugSampleS2l * n)()
                    slots = (_lib.WslS2lSlot * n)()
                    hold = []
                    for j, idx in enumerate(idxs):
                        img = dataset.staged(idx)[0]
                        w = dataset.images[idx]["weight"]
                        if w.device != dev or w.dtype != torch.float32 or not w.is_contiguous() or \
                                tuple(w.shape) != tuple(img.shape) + (C_,):
                            raise _lib.WslError(f"slice {idx}: the weight store must be a contiguous float32 device tensor "
                                                f"{tuple(img.shape) + (C_,)}, got {tuple(w.shape)} {w.dtype} on {w.device}")
                        hold += [img, w]
                        aug[j].img, aug[j].h, aug[j].w, aug[j].op = rt.ptr(img), img.shape[0], img.shape[1], 0
                        slots[j].weight, slots[j].h, slots[j].w = rt.ptr(w), img.shape[0], img.shape[1]
                    x = torch.empty((n, 1, Hn, Wn), dtype=torch.float32, device=dev)
                    rt.call("wsl_augment_batch_s2l", aug, n, C_, rt.ptr(x), None, None, None, Hn, Wn, rt.stream())     # zoom(img, order=0)
                    if mode == "eval":
                        z = m._run_forward(x)[0]
                    else:
                        z = torch.empty((n, C_, Hn, Wn), dtype=torch.float32, device=dev)
                        for j, idx in enumerate(idxs):
                            if masks is not None:
                                self._set_masks(masks[idx])
                            z[j:j + 1].copy_(m._run_forward(x[j:j + 1])[0])
                    rt.call("wsl_s2l_ensemble_update", rt.ptr(z), slots, n, C_, Hn, Wn, float(self.s2l_alpha), rt.stream())
        finally:
            if masks is not None:
                m.set_dropout_masks(None)
            m.train(was_training)

    def _finish_backward(self, x, t, kept=None):
        """kept ('semi_*'): the gradient arena of the step's FIRST backward, added to this one's before each bucket leaves (the first
        backward never all-reduces); the elementwise additions are the same with and without data parallelism"""
        m = self.model
        g = [t["dz1"], t["dz2"]]
        flat_g = m.flat_grads()
        ne = m.n_enc_param
        if self.dp:
            m._run_backward(x, g, phase=1)
            if kept is not None:
                rt.call("wsl_axpy", rt.ptr(flat_g[ne:]), rt.ptr(kept[ne:]), 1.0, flat_g.numel() - ne, rt.stream())
            self._allreduce(flat_g[ne:])
            m._run_backward(x, g, phase=2)
            if kept is not None:
                rt.call("wsl_axpy", rt.ptr(flat_g[:ne]), rt.ptr(kept[:ne]), 1.0, ne, rt.stream())
            self._allreduce(flat_g[:ne])
            if self.comm is not None:
                cur = torch.cuda.current_stream()
                if self._diag is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(cur)
                    cur.wait_stream(self.comm)
                    e1.record(cur)
                    self._diag.append((e0, e1))
                else:
                    cur.wait_stream(self.comm)
        else:
            m._run_backward(x, g, phase=0)
            if kept is not None:
                rt.call("wsl_axpy", rt.ptr(flat_g), rt.ptr(kept), 1.0, flat_g.numel(), rt.stream())

    def comm_diag(self, on):
        """on=True: start timing how long the main stream sits blocked on the all-reduce stream at the end of every backward;
        on=False: stop, return the total in ms (host sync on the recorded events)."""
        if on:
            self._diag, self._diag_buckets = [], []
            return 0.0
        pairs, self._diag = self._diag or [], None
        if pairs:
            pairs[-1][1].synchronize()
        return float(sum(a.elapsed_time(b) for a, b in pairs))

    def bucket_diag(self):
        """after comm_diag(False): {elements of the bucket: mean microseconds of its all-reduce on the comm stream} of the timed steps
        (decoders' bucket first, then the encoder's) -- what explains a scaling line without a second run"""
        recs, self._diag_buckets = getattr(self, "_diag_buckets", []), []
        if not recs:
            return {}
        recs[-1][2].synchronize()
        out = {}
        for n, a, b in recs:
            out.setdefault(n, []).append(a.elapsed_time(b) * 1e3)
        return {str(n): round(sum(v) / len(v), 2) for n, v in out.items()}

    def optimizer_step(self):
        m = self.model
        ema, alpha = None, 0.0
        if self.teacher is not None and not (self.loss_kind in self.SEMI and self.teacher_update == "frozen"):
            # update_ema_variables(model, ema_model, 0.99, iter_num), iter before increment ("frozen": the call the reference's two
            # mean-teacher scripts never make)
            ema, alpha = self.teacher._param_arena, min(1.0 - 1.0 / (self.it + 1), self.ema_decay)
        rt.call("wsl_sgd_step", rt.ptr(m._param_arena), rt.ptr(m._grad_arena), rt.ptr(self.mom), self.n, float(self.lr),
                self.mu, self.wd, int(self.it == 0), 1.0 / self.world, rt.ptr(ema), alpha, rt.stream())
        self.lr = self.base_lr * (1.0 - self.it / self.max_it) ** 0.9      # takes effect at the NEXT step
        self.it += 1

    def losses(self):
        """{loss, ce, pse|crf, n_valid} of the last step (host sync); 'semi_*': {loss, ce, dice, sup, cons, w, n_valid} with
        sup = 0.5 * (ce + dice), cons the raw unsupervised term and loss = sup + w * cons ('semi_uamt' adds n_certain, threshold)."""
        o = self.loss_out.tolist()
        if self.loss_kind == "pce_gatedcrf":
            return {"loss": o[1] + self.crf_weight * o[4], "ce": o[1], "crf": o[4], "n_valid": o[3]}
        if self.loss_kind in self.SEMI:        # cons is the raw (unweighted) unsupervised term, w the weight the step used
            sup = 0.5 * (o[1] + o[2])
            d = {"loss": sup + self._semi_w * o[4], "ce": o[1], "dice": o[2], "sup": sup, "cons": o[4], "w": self._semi_w, "n_valid": o[3]}
            if self.loss_kind == "semi_uamt":
                d["n_certain"], d["threshold"] = o[5], self._semi_thr
            if self.loss_kind == "semi_dan":              # the adversary's own loss of the last discriminator_step
                d["dan_loss"] = o[5]
            return d
        if self.loss_kind == "ce_dice":
            return {"loss": 0.5 * (o[1] + o[4]), "ce": o[1], "dice": o[4], "n_valid": o[3]}
        if self.loss_kind in self.REGULARISED:  # reg is the raw (unweighted) regulariser
            return {"loss": o[1] + self.REG_WEIGHT[self.loss_kind] * o[4], "ce": o[1], "reg": o[4], "n_valid": o[3]}
        if self.loss_kind == "pce_interintra":  # reg = inter - intra (unweighted), w = the weight the step used
            return {"loss": o[1] + self._var_w * o[self._var_slot], "ce": o[1], "reg": o[self._var_slot], "inter": o[6], "intra": o[7],
                    "w": self._var_w, "n_valid": o[3]}
        if self.loss_kind == "ustm":           # cons is the raw (unweighted) masked consistency; n_certain = sum(mask)
            return {"loss": o[1] + self._cons_w * o[4], "ce": o[1], "cons": o[4], "n_certain": o[5], "n_valid": o[3]}
        if self.loss_kind == "mean_teacher":   # tv / cons are the raw (unweighted) terms
            return {"loss": o[1] + self.tv_weight * o[4] + self._cons_w * o[5], "ce": o[1], "tv": o[4], "cons": o[5],
                    "n_valid": o[3]}
        if self.loss_kind == "s2l":            # before thr_iter the second CE is not part of the loss: ce_u 0, n_u 0
            f = self._s2l_fused
            return {"loss": o[0], "ce": o[1], "ce_u": o[2] if f else 0.0, "n_valid": o[3], "n_u": o[4] if f else 0.0}
        return {"loss": o[0], "ce": o[1], "pse": o[2], "n_valid": o[3]}
