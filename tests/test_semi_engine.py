"""Semi-supervised training through the Python layer: TrainEngine(loss="semi_mt" | "semi_uamt" | "semi_entmin") and the example, against the
oracle (two oracle forwards, the trainers' loss lines on torch ops, ONE backward), the package's own modules under autograd with the
interleaved loop of INTEGRATION.md, the closed forms of the schedules, and the reference's own recipe over several steps (fixtures
g15_semi_*, tests/golden/make_golden_semi.py: the trainers' loops on the reference's own UNet, losses and ramps).
`mode` = emul runs the Python layer against the host-emulation library with CPU tensors; `mode` = hip (gpu mark) is the real thing."""
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, close, get_backend, golden, grad_tol, mixed_err, rel_err, summary_line
from detinit import det_state
import semi_dp_worker as W

TOL = 1e-4
ACDC = os.path.join(ROOT, "tests", "golden", "acdc")
KINDS = ("semi_mt", "semi_uamt", "semi_entmin")
# semi_uamt: a more confident teacher head (x 10), so that the uncertainty threshold splits the pixels, and a teacher initialisation chosen by
# the REFERENCE's own conditioning.  The factor scales the teacher's logits and with them the round-off of its N = 2 forward (two values per
# channel in the deepest BatchNorm), which the softmax turns into a relative error of the targets: with det_state seed 24 the oracle's own
# float32 and float64 teacher forwards already give consistency gradients 5.7 x the close() criterion apart (mixed_err), with seed 30 0.27 x
# -- below a third of the bound -- with 40 % of the pixels certain and none within 3e-3 (relative) of the threshold.  semi_mt keeps the
# unsharpened seed 24.
SHARP = 10.0
TEACHER_SEED = {"semi_mt": 24, "semi_uamt": 30}


@pytest.fixture(params=[pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)])
def mode(request):
    from wsl4mis_amd import _lib, runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    if request.param == "emul":
        _lib.use_library_for_tests(get_backend("emul").lib)
    yield request.param
    _lib._reset_for_tests()
    runtime._ws_cache.clear()


def cases(emul, hip):
    """explicit (mode, *args) parameters.  Every loss and route runs on both backends for the checks against a reference (oracle step,
    interleaved module loop, example, recipe); only the two self-consistency checks (bit-reproducibility, the 1-rank data-parallel route),
    which run each step twice, keep one loss on the host emulator -- a network step costs it tens of seconds -- and all on the device"""
    ident = lambda c: "-".join(str(v) for v in c)  # noqa: E731
    return [pytest.param("emul", *c, id="emul-" + ident(c)) for c in emul] + \
           [pytest.param("hip", *c, id="hip-" + ident(c), marks=pytest.mark.gpu) for c in hip]


def dev():
    from wsl4mis_amd import runtime
    return runtime.device()


def T(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev())


def TL(ms):
    return [T(m) for m in ms]


def load_det(model, seed, sharp=False):
    sd = model.state_dict()
    vals = det_state({k: tuple(v.shape) for k, v in sd.items()}, seed)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}
    if sharp:
        sd["decoder.out_conv.weight"] = sd["decoder.out_conv.weight"] * SHARP
    model.load_state_dict(sd)


def oracle_state(seed, sharp=False):
    from oracle import torch_ref as R
    layout = {k: tuple(s) for k, s in R.state_layout("unet", 1, 4)}
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in det_state(layout, seed).items()}
    if sharp:
        sd["decoder.out_conv.weight"] = sd["decoder.out_conv.weight"] * SHARP
    return sd


def weight_formula(it, consistency=0.1, rampup=200.0):
    if rampup == 0:
        return consistency
    t = min(max(float(it // 300), 0.0), rampup) / rampup
    return consistency * math.exp(-5.0 * (1.0 - t) ** 2)


def threshold_formula(it, max_it):
    t = min(max(float(it), 0.0), float(max_it)) / max_it
    return (0.75 + 0.25 * math.exp(-5.0 * (1.0 - t) ** 2)) * math.log(2.0)


def script_losses(kind, z_l, z_u, lab, it, max_it, zt=None, preds=None, consistency=0.1, rampup=200.0):
    """the trainers' loss lines on torch ops (train_mean_teacher_2D.py:161-171, train_uncertainty_aware_mean_teacher_2D.py:171-190,
    train_entropy_minimization_2D.py:132-143): (loss, ce, dice, sup, cons, w, extra)"""
    from oracle import torch_ref as R
    ce = F.cross_entropy(z_l, lab.long())
    dice = R.dice(torch.softmax(z_l, 1), lab.long().unsqueeze(1))
    sup = 0.5 * (dice + ce)
    w = weight_formula(it, consistency, rampup)
    extra = {}
    s_u = torch.softmax(z_u, 1)
    if kind == "semi_mt":
        cons = torch.mean((s_u - torch.softmax(zt, 1)) ** 2)
    elif kind == "semi_uamt":
        N, C = z_u.shape[:2]
        p = torch.softmax(torch.cat(list(preds), 0), 1).reshape(8, N, C, z_u.shape[2], z_u.shape[3]).mean(0)
        unc = -1.0 * torch.sum(p * torch.log(p + 1e-6), dim=1, keepdim=True)
        thr = threshold_formula(it, max_it)
        mask = (unc < thr).to(z_u.dtype)
        cons = torch.sum(mask * (s_u - torch.softmax(zt, 1)) ** 2) / (2 * torch.sum(mask) + 1e-16)
        extra = {"n_certain": float(mask.sum()), "threshold": thr, "margin": float(((unc - thr).abs() / thr).min())}
    else:
        cons = torch.mean(-1 * torch.sum(s_u * torch.log(s_u + 1e-6), dim=1) / math.log(4))
    return sup + w * cons, ce, dice, sup, cons, w, extra


# ------------------------------------------------------------------------------------------------ one step against the oracle
ALL_STEPS = [(k, f) for k in KINDS for f in ("fused", "chain")]


@pytest.mark.parametrize("mode,kind,route", cases(ALL_STEPS, ALL_STEPS), indirect=["mode"])
def test_engine_step_against_oracle(mode, kind, route):
    """one engine step (N_l = 3, N_u = 2 -- unequal on purpose -- at 16 x 16) against two oracle forwards, the script's loss lines and ONE
    backward(): both logit gradients by close(), every loss value to 1e-4, parameters and BatchNorm running statistics after the step by
    close() (two momentum updates, labeled then unlabeled), the EMA teacher, and with teacher_update='frozen' a bit-unchanged teacher arena.
    Both student forwards keep every pre-activation clear of the LeakyReLU kink and every pooling window clear of a tie (asserted)."""
    from netutil import KinkMargins
    from oracle import torch_ref as R
    from wsl4mis_amd.engine import TrainEngine
    fused = route == "fused"
    d = W.semi_inputs(W.STEP_SEED)
    it0, max_it, Nu = W.IT0, W.MAX_IT, d["x_u"].shape[0]
    sharp = kind == "semi_uamt"
    t_seed = TEACHER_SEED.get(kind, 24)
    sd, sd_t = oracle_state(23), oracle_state(t_seed, sharp=sharp)
    pk = [k for k in sd if R.is_param(k)]
    for k in pk:
        sd[k].requires_grad_(True)
    with KinkMargins() as km:
        z_l = R.net_forward(sd, d["x_l"], "unet", d["m_l"], None, True)
        z_u = R.net_forward(sd, d["x_u"], "unet", d["m_u"], None, True)
    assert km.leaky >= 1e-5 and km.pool >= 1e-5, ("the batches are not kink-clear any more", km.leaky, km.pool)
    zt = preds = None
    if kind != "semi_entmin":
        with torch.no_grad():
            zt = R.net_forward(sd_t, d["x_u"] + d["noise"][0], "unet", d["m_t"][Nu], None, True)
            if kind == "semi_uamt":
                preds = [R.net_forward(sd_t, d["x_u"].repeat(2, 1, 1, 1) + d["noise"][1 + i], "unet", d["m_t"][2 * Nu], None, True) for i in range(4)]
    z_l.retain_grad(), z_u.retain_grad()
    loss, ce, dice, sup, cons, w, extra = script_losses(kind, z_l, z_u, d["lab"], it0, max_it, zt, preds)
    loss.backward()
    if kind == "semi_uamt":
        assert 0.1 * Nu * 256 < extra["n_certain"] < 0.9 * Nu * 256, extra          # the threshold actually splits the pixels
        assert extra["margin"] > 1e-3, extra                                        # ... and no pixel sits on it: a flip is discrete
    with torch.no_grad():
        ps = [sd[k] for k in pk]
        R.sgd_step(ps, [p.grad for p in ps], [torch.zeros_like(p) for p in ps], 0.01, first=False)
        if zt is not None:
            R.ema_update([sd_t[k] for k in pk], ps, 0.99, it0)
    # ---- engine
    updates = ("ema",) if kind == "semi_entmin" else ("ema", "frozen")
    for update in updates:
        eng = TrainEngine("unet", 1, 4, base_lr=0.01, max_iterations=max_it, loss=kind, teacher_update=update)
        eng.fused_heads = fused
        load_det(eng.model, 23)
        eng.it = it0
        noise = None
        if eng.teacher is not None:
            load_det(eng.teacher, t_seed, sharp=sharp)
            eng.teacher.set_dropout_masks(lambda n, h, w_: (TL(d["m_t"][n]), None))
            noise = T(d["noise"][0]) if kind == "semi_mt" else TL(d["noise"])
            t_before = eng.teacher._param_arena.clone()
        eng.forward_backward(T(d["x_l"]), T(d["lab"]), unlabeled=T(d["x_u"]), noise=noise, masks=(TL(d["m_l"]), TL(d["m_u"])))
        o = eng.losses()
        dz_l, dz_u = eng._semi_tensors(3, 16, 16, "l")["dz"].cpu().numpy(), eng._semi_tensors(Nu, 16, 16, "u")["dz"].cpu().numpy()
        for name, got_g, ref_g in (("dz_l", dz_l, z_l.grad.numpy()), ("dz_u", dz_u, z_u.grad.numpy())):
            print(f"SEMI-STEP [{mode}] {kind} {route} {update} {name}: rel_err {rel_err(got_g, ref_g):.3e} mixed_err {mixed_err(got_g, ref_g, TOL):.3e}")
        if kind == "semi_uamt":
            print(f"SEMI-STEP [{mode}] {kind} n_certain {o['n_certain']} (oracle {extra['n_certain']}), closest pixel to the threshold {extra['margin']:.2e} rel.")
        assert close(dz_l, z_l.grad.numpy(), TOL)
        assert close(dz_u, z_u.grad.numpy(), TOL)
        eng.optimizer_step()
        assert rel_err([o["loss"], o["ce"], o["dice"], o["sup"], o["cons"]], [loss.item(), ce.item(), dice.item(), sup.item(), cons.item()]) < TOL, o
        assert rel_err(o["cons"], cons.item()) < TOL and o["w"] == pytest.approx(w, rel=1e-12) and o["n_valid"] == 3 * 256
        assert set(o) == {"loss", "ce", "dice", "sup", "cons", "w", "n_valid"} | ({"n_certain", "threshold"} if kind == "semi_uamt" else set())
        assert o["sup"] == pytest.approx(0.5 * (o["ce"] + o["dice"]), rel=1e-6) and o["loss"] == pytest.approx(o["sup"] + o["w"] * o["cons"], rel=1e-6)
        if kind == "semi_uamt":
            assert o["n_certain"] == extra["n_certain"] and o["threshold"] == pytest.approx(extra["threshold"], rel=1e-12)
        got = eng.model.state_dict()
        for k in pk:
            assert close(got[k].detach().cpu().numpy(), sd[k].detach().numpy(), TOL), k
        for k in sd:
            if k.endswith(("running_mean", "running_var")):
                assert close(got[k].cpu().numpy(), sd[k].numpy(), TOL), k
            elif k.endswith("num_batches_tracked"):
                assert int(got[k]) == int(sd[k]) == int(oracle_state(23)[k]) + 2, k
        if eng.teacher is not None and update == "ema":
            got_t = eng.teacher.state_dict()
            for k in pk:
                assert rel_err(got_t[k].detach().cpu(), sd_t[k].detach()) < TOL, k
        elif eng.teacher is not None:
            assert torch.equal(eng.teacher._param_arena, t_before)


# ------------------------------------------------------------------------------------------------ the module path, interleaved
def interleaved_loop(model, kind, x_l, lab, x_u, w, zt=None):
    """sup.backward() BEFORE the second model(...), (w * cons).backward() after it -- p.grad accumulates"""
    from oracle import torch_ref as R
    z_l = model(x_l)
    ce = F.cross_entropy(z_l, lab.long())
    dice = R.dice(torch.softmax(z_l, 1), lab.long().unsqueeze(1))
    sup = 0.5 * (dice + ce)
    sup.backward()
    z_u = model(x_u)
    s_u = torch.softmax(z_u, 1)
    if kind == "semi_mt":
        cons = torch.mean((s_u - torch.softmax(zt, 1)) ** 2)
    else:
        cons = torch.mean(-1 * torch.sum(s_u * torch.log(s_u + 1e-6), dim=1) / math.log(4))
    (w * cons).backward()
    return ce, dice, cons


@pytest.mark.parametrize("mode,kind", cases([("semi_mt",), ("semi_entmin",)], [("semi_mt",), ("semi_entmin",)]), indirect=["mode"])
def test_interleaved_module_loop_gives_the_engine_gradients_unet(mode, kind):
    """the reference-style loop on the package's own UNet module -- two model(...) calls, a backward() after each -- accumulates the
    gradient arena the engine's step holds; the literal order (two forwards, then one backward) still raises"""
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.networks.net_factory import net_factory
    d = W.semi_inputs(W.STEP_SEED)
    eng = TrainEngine("unet", 1, 4, loss=kind, consistency_rampup=0)
    load_det(eng.model, 23)
    noise = None
    if eng.teacher is not None:
        load_det(eng.teacher, 24)
        eng.teacher.set_dropout_masks(TL(d["m_t"][2]))
        noise = T(d["noise"][0])
    x_l, lab, x_u = T(d["x_l"]), T(d["lab"]), T(d["x_u"])
    eng.forward_backward(x_l, lab, unlabeled=x_u, noise=noise, masks=(TL(d["m_l"]), TL(d["m_u"])))
    o, g_eng = eng.losses(), eng.model.flat_grads().clone()
    model = net_factory("unet", 1, 4)
    load_det(model, 23)
    model.train()
    zt = None
    if kind == "semi_mt":
        teacher = net_factory("unet", 1, 4)
        load_det(teacher, 24)
        teacher.train()
        teacher.set_dropout_masks(TL(d["m_t"][2]))
        with torch.no_grad():
            zt = teacher(x_u + T(d["noise"][0]))
    seq = iter((TL(d["m_l"]), TL(d["m_u"])))
    model.set_dropout_masks(lambda n, h, w_: (next(seq), None))
    ce, dice, cons = interleaved_loop(model, kind, x_l, lab, x_u, 0.1, zt)
    assert rel_err([o["ce"], o["dice"], o["cons"]], [ce.item(), dice.item(), cons.item()]) < TOL, o
    off = 0
    for k, p in model.named_parameters():
        n = p.numel()
        got, ref = g_eng[off:off + n].cpu().numpy().astype(np.float64), p.grad.reshape(-1).cpu().numpy().astype(np.float64)
        if k.endswith(("conv_conv.0.bias", "conv_conv.4.bias")):        # feeds a BatchNorm: mathematically zero
            assert np.max(np.abs(got - ref)) <= TOL * np.max(np.abs(ref)) + 1e-5, k
        else:
            assert close(got, ref, TOL), k
        off += n
    # the literal order of the scripts: two forwards, one backward
    model.set_dropout_masks(None)
    model.zero_grad()
    z1, z2 = model(x_l), model(x_u)
    with pytest.raises(_lib.WslError, match="after a newer training forward"):
        (z1.sum() + z2.sum()).backward()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["semi_entmin", "semi_mt"])
def test_engine_step_against_module_path_pnet(kind):
    """the step on PNet2D at N = 2, 32 x 32 against the package's own module under autograd with the interleaved loop and torch's SGD:
    losses to 1e-4, gradients by close(), parameters after the step to 1e-6.  Device only: PNet's 64-channel dilated stack is minutes on
    the emulator"""
    from wsl4mis_amd import _lib, runtime
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.networks.net_factory import net_factory
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    dv = torch.device("cuda:0")
    N, S, w = 2, 32, 0.1
    gen = torch.Generator().manual_seed(17)
    x_l, x_u = torch.rand((N, 1, S, S), generator=gen).to(dv), torch.rand((N, 1, S, S), generator=gen).to(dv)
    lab = torch.randint(0, 4, (N, S, S), generator=gen).to(torch.uint8).to(dv)
    noise = torch.clamp(torch.randn((N, 1, S, S), generator=gen) * 0.1, -0.2, 0.2).to(dv)
    ms = [[((torch.rand((N, c), generator=gen) >= 0.3).float() / 0.7).to(dv) for c in (128, 64)] for _ in range(3)]
    eng = TrainEngine("pnet", 1, 4, loss=kind, consistency=w, consistency_rampup=0)
    load_det(eng.model, 31)
    if eng.teacher is not None:
        load_det(eng.teacher, 32)
        eng.teacher.set_dropout_masks(ms[2])
    eng.forward_backward(x_l, lab, unlabeled=x_u, noise=noise if kind == "semi_mt" else None, masks=(ms[0], ms[1]))
    o, g_eng = eng.losses(), eng.model.flat_grads().clone()
    eng.optimizer_step()
    model = net_factory("pnet", 1, 4)
    load_det(model, 31)
    model.train()
    zt = None
    if kind == "semi_mt":
        teacher = net_factory("pnet", 1, 4)
        load_det(teacher, 32)
        teacher.train()
        teacher.set_dropout_masks(ms[2])
        with torch.no_grad():
            zt = teacher(x_u + noise)
    seq = iter((ms[0], ms[1]))
    model.set_dropout_masks(lambda n, h, w_: next(seq))
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    opt.zero_grad()
    ce, dice, cons = interleaved_loop(model, kind, x_l, lab, x_u, w, zt)
    assert rel_err([o["ce"], o["dice"], o["cons"], o["loss"]], [ce.item(), dice.item(), cons.item(), 0.5 * (ce.item() + dice.item()) + w * cons.item()]) < TOL, o
    off = 0
    for k, p in model.named_parameters():
        n = p.numel()
        got, ref = g_eng[off:off + n].cpu().numpy().astype(np.float64), p.grad.reshape(-1).cpu().numpy().astype(np.float64)
        if k.startswith("block") and k.endswith(("conv1.bias", "conv2.bias")):      # feeds a BatchNorm: mathematically zero
            assert np.max(np.abs(got - ref)) <= TOL * np.max(np.abs(ref)) + 1e-5, k
        else:
            assert close(got, ref, TOL), k
        off += n
    opt.step()
    got_p = eng.model.state_dict()
    for k, p in model.named_parameters():
        assert rel_err(got_p[k].cpu(), p.detach().cpu()) < 1e-6, k


# ------------------------------------------------------------------------------------------------ schedules, losses(), refusals
def test_weight_and_threshold_schedules(mode):
    """w(t) = consistency * sigmoid_rampup(it // 300, consistency_rampup) and the uncertainty threshold against their closed forms; the
    weight a step uses is the one of `it` BEFORE the increment; the key set of losses(); loss == sup + w * cons"""
    from wsl4mis_amd.engine import TrainEngine
    eng = TrainEngine("unet", 1, 4, loss="semi_uamt", max_iterations=60000)
    assert (eng.consistency, eng.consistency_rampup, eng.ema_decay, eng.teacher_update) == (0.1, 200.0, 0.99, "ema")
    for it in (0, 299, 300, 60000):
        eng.it = it
        assert eng.consistency_weight() == pytest.approx(weight_formula(it), rel=1e-12), it
        assert eng.uncertainty_threshold() == pytest.approx(threshold_formula(it, 60000), rel=1e-12), it
    assert eng.consistency_weight(0) == eng.consistency_weight(299) == pytest.approx(0.1 * math.exp(-5.0))
    assert eng.consistency_weight(300) > eng.consistency_weight(299) and eng.consistency_weight(60000) == pytest.approx(0.1)
    assert eng.uncertainty_threshold(0) == pytest.approx((0.75 + 0.25 * math.exp(-5.0)) * math.log(2.0))
    assert eng.uncertainty_threshold(60000) == pytest.approx(math.log(2.0))
    assert TrainEngine("unet", 1, 4, loss="semi_entmin", consistency=0.3, consistency_rampup=0).consistency_weight() == 0.3
    d = W.semi_inputs(W.STEP_SEED)
    eng = TrainEngine("unet", 1, 4, loss="semi_entmin")
    load_det(eng.model, 23)
    eng.it = 300
    eng.step(T(d["x_l"]), T(d["lab"]), unlabeled=T(d["x_u"]))
    o = eng.losses()
    assert eng.it == 301 and o["w"] == pytest.approx(weight_formula(300), rel=1e-12) and o["w"] != weight_formula(299)
    assert set(o) == {"loss", "ce", "dice", "sup", "cons", "w", "n_valid"}       # (semi_uamt's two extra keys: the oracle test)
    assert o["sup"] == pytest.approx(0.5 * (o["ce"] + o["dice"]), rel=1e-6) and o["loss"] == pytest.approx(o["sup"] + o["w"] * o["cons"], rel=1e-6)
    assert np.isfinite(o["loss"]) and o["cons"] > 0


def test_refusals(mode):
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    for kind in KINDS:
        with pytest.raises(_lib.WslError, match="single-decoder"):
            TrainEngine("unet_cct", 1, 4, loss=kind)
    assert TrainEngine("pnet", 1, 4, loss="semi_mt").teacher is not None
    # the default route per loss is a measured decision (profiles/semi_bench.md): the chain for semi_uamt, the fused heads otherwise
    assert {k: TrainEngine("unet", 1, 4, loss=k).fused_heads for k in KINDS} == {"semi_mt": True, "semi_uamt": False, "semi_entmin": True}
    with pytest.raises(ValueError):
        TrainEngine("unet", 1, 4, loss="semi_mt", teacher_update="sometimes")
    d = W.semi_inputs(W.STEP_SEED)
    x_l, lab, x_u = T(d["x_l"]), T(d["lab"]), T(d["x_u"])
    eng = TrainEngine("unet", 1, 4, loss="semi_entmin")
    with pytest.raises(_lib.WslError, match="unlabeled"):
        eng.step(x_l, lab)
    with pytest.raises(_lib.WslError, match="differ in N only"):
        eng.step(x_l, lab, unlabeled=T(torch.zeros((2, 1, 16, 32))))
    with pytest.raises(_lib.WslError, match="unlabeled"):
        TrainEngine("unet", 1, 4, loss="pce").step(x_l, lab, unlabeled=x_u)
    assert eng.it == 0


# ------------------------------------------------------------------------------------------------ reproducibility, data parallel
def small_run(kind, fused=True, force_dp=False):
    from wsl4mis_amd.engine import TrainEngine
    d = W.semi_inputs(W.STEP_SEED)
    eng = TrainEngine("unet", 1, 4, loss=kind, consistency_rampup=0, force_dp=force_dp)
    eng.fused_heads = fused
    load_det(eng.model, 23)
    if eng.teacher is not None:
        load_det(eng.teacher, 24, sharp=True)
    torch.manual_seed(77)
    eng.forward_backward(T(d["x_l"]), T(d["lab"]), unlabeled=T(d["x_u"]))
    g = eng.model.flat_grads().clone()
    eng.optimizer_step()
    return np.array(list(eng.losses().values())), eng.model.flat_params().clone(), g, eng.loss_out.clone(), eng


@pytest.mark.parametrize("mode,kind", cases([("semi_mt",)], [(k,) for k in KINDS]), indirect=["mode"])
def test_whole_step_is_bit_reproducible(mode, kind):
    """two runs with the same torch.manual_seed give the same bits in losses, parameters and gradients: every reduction of the new heads is
    order-fixed, and the library-drawn dropout masks and teacher noises are functions of torch's seed"""
    a, b = small_run(kind), small_run(kind)
    assert np.all(np.isfinite(a[0])) and a[0][4] > 0
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("mode,kind", cases([("semi_entmin",)], [("semi_mt",), ("semi_entmin",)]), indirect=["mode"])
def test_one_rank_group_through_the_dp_route_changes_nothing(mode, kind):
    """force_dp in a 1-rank gloo group: the second backward in two phases, the kept arena added per bucket before its all-reduce -- the
    same elementwise additions as the plain route, so the gradients (and the parameters after the step) are torch.equal"""
    import torch.distributed as dist
    plain = small_run(kind)
    assert not plain[4].dp
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        routed = small_run(kind, force_dp=True)
        assert routed[4].dp
    finally:
        dist.destroy_process_group()
    assert torch.equal(plain[2], routed[2]) and torch.equal(plain[1], routed[1]) and np.array_equal(plain[0], routed[0])


def test_two_rank_gloo_semi_mt_matches_the_oracle(tmp_path):
    """two gloo ranks on the emulator, each with its own labeled / unlabeled shard (2 + 2 slices of 32 x 32, the shard shape of
    tests/test_dp.py): the averaged gradient per tensor (grad_tol), the SGD step and the EMA teacher to 1e-6 equal the oracle's per-shard
    computation averaged (DDP-equivalent semantics), replicas bit-identical"""
    from netutil import KinkMargins
    from oracle import torch_ref as R
    get_backend("emul")
    port = str(_free_port())
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "semi_dp_worker.py"), str(r), "2", port, str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=1500)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    assert np.array_equal(r0["grads"], r1["grads"]) and np.array_equal(r0["params_after"], r1["params_after"])
    assert np.array_equal(r0["teacher_after"], r1["teacher_after"])
    shard_grads, pk = [], None
    for r, rr in enumerate((r0, r1)):
        d = W.semi_inputs(W.SHARD_SEEDS[r], *W.SHARD_SHAPE)
        sd = oracle_state(23)
        pk = [k for k in sd if R.is_param(k)]
        for k in pk:
            sd[k].requires_grad_(True)
        with KinkMargins() as km:
            z_l = R.net_forward(sd, d["x_l"], "unet", d["m_l"], None, True)
            z_u = R.net_forward(sd, d["x_u"], "unet", d["m_u"], None, True)
        assert km.leaky > 4e-6 and km.pool > 1e-6, (r, km.leaky, km.pool)        # the margins tests/test_dp.py asks of its shards
        with torch.no_grad():
            zt = R.net_forward(oracle_state(24), d["x_u"] + d["noise"][0], "unet", d["m_t"][d["x_u"].shape[0]], None, True)
        loss = script_losses("semi_mt", z_l, z_u, d["lab"], W.IT0, W.MAX_IT, zt)[0]
        loss.backward()
        assert abs(float(rr["loss"]) - float(loss)) <= TOL * abs(float(loss)), (r, float(rr["loss"]), float(loss))
        shard_grads.append(np.concatenate([sd[k].grad.numpy().ravel() for k in pk]).astype(np.float64))
    ref = 0.5 * (shard_grads[0] + shard_grads[1])
    s23, s24 = oracle_state(23), oracle_state(24)
    off, bad = 0, []
    for k in pk:
        n = s23[k].numel()
        err = float(np.max(np.abs(r0["grads"][off:off + n] - ref[off:off + n])))
        if err > grad_tol(k, ref[off:off + n]):
            bad.append((k, err, float(np.max(np.abs(ref[off:off + n])))))
        off += n
    assert not bad, bad[:6]
    p0 = np.concatenate([s23[k].numpy().ravel() for k in pk]).astype(np.float64)
    p1 = p0 - 0.01 * (ref + 1e-4 * p0)              # it = 30000: the momentum buffer starts at zero -> buf = g
    assert np.max(np.abs(r0["params_after"] - p1)) <= 1e-6 * np.max(np.abs(p1))
    t0 = np.concatenate([s24[k].numpy().ravel() for k in pk]).astype(np.float64)
    assert np.max(np.abs(r0["teacher_after"] - (0.99 * t0 + 0.01 * p1))) <= 1e-6 * np.max(np.abs(t0))


# ------------------------------------------------------------------------------------------------ the example
@pytest.mark.parametrize("mode,kind", cases([(k,) for k in KINDS], [(k,) for k in KINDS]), indirect=["mode"])
def test_example_trainer_runs_semi(mode, tmp_path, kind):
    """--loss semi_* end to end on the committed ACDC fixture, fold3 (patients 010 / 030 labeled, 094 unlabeled): two loaders of
    batch_size // 2, the model defaults to unet, every logged loss is sup + w * cons, --teacher_update reaches the engine"""
    spec = importlib.util.spec_from_file_location("train_acdc_semi", os.path.join(ROOT, "examples", "train_acdc_scribble.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    curve = os.path.join(str(tmp_path), "curve.json")
    seen = {}
    from wsl4mis_amd import engine as E

    class Spy(E.TrainEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen["eng"] = self
    real, mod.TrainEngine = mod.TrainEngine, Spy
    try:
        hist = mod.main(["--root_path", ACDC, "--fold", "fold3", "--loss", kind, "--max_iterations", "2", "--batch_size", "4",
                         "--patch_size", "16", "16", "--val_every", "1000", "--log_every", "1", "--consistency", "0.2", "--consistency_rampup", "0",
                         "--teacher_update", "frozen", "--quiet", "--curve_json", curve])
    finally:
        mod.TrainEngine = real
    eng = seen["eng"]
    assert eng.teacher_update == "frozen" and eng.loss_kind == kind and type(eng.model).__name__ == "UNet" and eng.it == 2
    assert len(hist) == 2 and all(np.isfinite(l) for _, l in hist)
    log = json.load(open(curve))["curve"]
    assert len(log) == 2 and all(r["w"] == 0.2 and r["n_valid"] == 2 * 256 and np.isfinite(r["cons"]) for r in log)
    assert all(abs(r["loss"] - (r["sup"] + 0.2 * r["cons"])) < 1e-5 and abs(r["sup"] - 0.5 * (r["ce"] + r["dice"])) < 1e-5 for r in log)


# ------------------------------------------------------------------------------------------------ the reference's recipe
def _unpack(g, key, n, P):
    return [T(np.unpackbits(g[f"{key}_em{l}"])[:n * (16 << l) * (P >> l) * (P >> l)].reshape(n, 16 << l, P >> l, P >> l)) for l in range(5)]


def run_recipe(kind, steps):
    from wsl4mis_amd.engine import TrainEngine
    g = golden("g15_" + kind)
    cons, ramp, max_it, lr, s_seed, t_seed, sharp = (float(v) for v in g["meta_hyper"])
    xl, xu, lab = g["in_xl"], g["in_xu"], g["in_lab"]
    n, P = xl.shape[1], xl.shape[3]
    eng = TrainEngine("unet", 1, 4, base_lr=lr, max_iterations=int(max_it), loss=kind, consistency=cons, consistency_rampup=ramp,
                      teacher_update="frozen")            # the scripts never call update_ema_variables
    load_det(eng.model, int(s_seed))
    if eng.teacher is not None:
        load_det(eng.teacher, int(t_seed))
        if sharp != 1.0:
            with torch.no_grad():
                eng.teacher.decoder.out_conv.weight.mul_(sharp)
    got = []
    for it in range(steps):
        noise = None
        if kind != "semi_entmin":
            order = iter([_unpack(g, f"s{it}_t0", n, P)] + ([_unpack(g, f"s{it}_t{i + 1}", 2 * n, P) for i in range(4)] if kind == "semi_uamt" else []))
            eng.teacher.set_dropout_masks(lambda n_, h, w_, order=order: (next(order), None))
            noise = T(g["in_noise0"][it]) if kind == "semi_mt" else [T(g["in_noise0"][it])] + [T(g["in_noiseT"][it, i]) for i in range(4)]
        eng.step(T(xl[it]), T(lab[it]), unlabeled=T(xu[it]), noise=noise, masks=(_unpack(g, f"s{it}_l", n, P), _unpack(g, f"s{it}_u", n, P)))
        o = eng.losses()
        got.append([o["loss"], o["ce"], o["dice"], o["cons"], o.get("n_certain", 0.0)])
    return np.array(got), g, eng


@pytest.mark.parametrize("mode,kind", cases([(k,) for k in KINDS], [(k,) for k in KINDS]), indirect=["mode"])
def test_engine_follows_the_reference_recipe(mode, kind):
    """the trainer's loop on the reference's own UNet, DiceLoss / softmax_mse_loss / entropy_loss and ramps (6 steps of semi_mt, 4 of
    semi_uamt and semi_entmin, N_l = N_u = 2, 32 x 32, constant weight 0.1, the teacher never updated -- as the scripts run it): loss, ce,
    dice and the unsupervised term per step against the reference's float32 run -- the first two steps to 1e-4, the tail to 3e-2, the
    first 256 values of three final tensors to 5e-2 -- and for semi_uamt the number of certain pixels exactly.  The fixture's own
    float32-vs-float64 spread (asserted below a third of each bound when it was generated) is reported next to the measured error.
    The emulator leg runs the two tightly bounded steps only."""
    steps_all = {"semi_mt": 6, "semi_uamt": 4, "semi_entmin": 4}[kind]
    steps = 2 if mode == "emul" else steps_all
    got, g, eng = run_recipe(kind, steps)
    ref, ref64 = g["meta_losses_f32"][:steps], g["meta_losses_f64"][:steps]
    rel = np.abs(got[:, :4] - ref[:, :4]) / np.abs(ref[:, :4])
    spread = np.abs(ref[:, :4] - ref64[:, :4]) / np.abs(ref64[:, :4])
    summary_line(f"SEMI-CURVE {kind} [{mode}]: worst rel. error per step over (loss, ce, dice, cons) {np.array2string(rel.max(1), precision=2)}; "
                 f"the reference's own fp32-vs-fp64 spread {np.array2string(spread.max(1), precision=2)}")
    assert np.all(np.isfinite(got))
    assert np.max(rel[:2]) < 1e-4, (got, ref)
    assert np.max(rel) < 3e-2, (got, ref)
    if kind == "semi_uamt":
        assert np.array_equal(got[:, 4], ref[:, 4]), (got[:, 4], ref[:, 4])
    if steps == steps_all:
        sd = eng.model.state_dict()
        for k in [k[10:] for k in g.files if k.startswith("final_f32:")]:
            assert rel_err(sd[k].cpu().numpy().ravel()[:256], g["final_f32:" + k]) < 5e-2, k
