"""TrainEngine(loss='semi_dan'): the adversarial semi-supervised step (ref: train_deep_adversarial_network_2D.py:135-184) -- the generator
update against the oracle composition (two forwards, one backward, torch ops for the adversary), the discriminator update, the // 150
weight schedule, the literal t_u rule, what each half leaves untouched, the module-path loop, the example, two gloo ranks, the reference's
own recipe (fixture g16_dan_recipe, tests/golden/make_golden_dan.py) and bit-reproducibility.

`mode` = emul runs the Python layer against the host-emulation library with CPU tensors; `mode` = hip (gpu mark) is the real thing.  A
network step costs the emulator tens of seconds, so its cases are few: one engine step (both halves checked on it), the module loop, the
example, the two ranks and two steps of the recipe."""
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

import dan_ref as DR
import dan_dp_worker as DW
import semi_dp_worker as W
from conftest import ROOT, close, get_backend, golden, grad_tol, rel_err
from detinit import det_state

TOL = 1e-4
ACDC = os.path.join(ROOT, "tests", "golden", "acdc")
NDF, DAN_SEED = 8, 9
# generator seed of the one-step batch (N_l = 2, N_u = 3 -- N_u > N_l on purpose: t_u = [1, 1, 0] -- at 32 x 32), searched so that no
# pre-activation / pooling window of either student forward (det_state 23) lies within fp32 noise of a kink (the 4e-6 / 1e-6 of
# tests/test_dp.py's 32 x 32 shards) and none of the adversary's (rand_state 9) within 1e-4; the test re-checks the margins
STEP_SEED, STEP_SHAPE = 719, (2, 3, 32)
LR_DAN, BETAS, EPS = 1e-4, (0.9, 0.99), 1e-8


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


@pytest.fixture
def hip():
    from wsl4mis_amd import _lib, runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    yield "hip"
    runtime._ws_cache.clear()


def dev():
    from wsl4mis_amd import runtime
    return runtime.device()


def T(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev())


def TL(ms):
    return [T(m) for m in ms]


def load_det(model, seed):
    vals = det_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})


def oracle_state(seed):
    from oracle import torch_ref as R
    layout = {k: tuple(s) for k, s in R.state_layout("unet", 1, 4)}
    return {k: torch.from_numpy(np.asarray(v)).clone() for k, v in det_state(layout, seed).items()}


def weight_formula(it, consistency=0.1, rampup=200.0):
    if rampup == 0:
        return consistency
    t = min(max(float(it // 150), 0.0), rampup) / rampup
    return consistency * math.exp(-5.0 * (1.0 - t) ** 2)


def dan_targets(n_l, n_u):
    full = torch.tensor([1] * n_l + [0] * n_u)
    return full, full[:n_u]


def make_engine(**kw):
    from wsl4mis_amd.engine import TrainEngine
    eng = TrainEngine("unet", 1, 4, loss="semi_dan", dan_ndf=NDF, dan_pool=1, **kw)
    load_det(eng.model, 23)
    eng.discriminator.load_state_dict(DR.rand_state(DAN_SEED, 4, NDF, 1))
    return eng


def adam_update_ok(before, after, grad, step=1):
    """`after` is one float64 Adam step of `before` on `grad`: each update within 1e-4 of lr, plus the rounding of storing p in float32"""
    p = torch.from_numpy(before).double()
    DR.adam_step(p, torch.from_numpy(np.asarray(grad)).double(), torch.zeros_like(p), torch.zeros_like(p), step, LR_DAN, BETAS, EPS)
    err = np.abs((after.astype(np.float64) - before) - (p.numpy() - before))
    return bool(np.all(err <= 1e-4 * LR_DAN + 2.0 ** -23 * np.abs(before))), float(err.max())


# ------------------------------------------------------------------------------------------------ one step, both halves
def test_step_against_the_oracle_composition(mode):
    """Generator update: every parameter gradient of the segmentation net against two oracle forwards, the script's loss lines with the
    adversary on torch ops, ONE backward() -- 1e-4 of each tensor's scale; it leaves the adversary's parameters and Adam state bit-unchanged.
    Discriminator update: its parameter gradients and loss against the oracle's EVAL forwards of the post-SGD state (and NOT of the
    pre-SGD one), one Adam step; it leaves the net's parameters, gradient arena, running statistics and counters bit-unchanged."""
    from netutil import KinkMargins
    from oracle import torch_ref as R
    d = W.semi_inputs(STEP_SEED, *STEP_SHAPE)
    n_l, n_u = STEP_SHAPE[:2]
    t_full, t_u = dan_targets(n_l, n_u)
    assert t_u.tolist() == [1, 1, 0]                       # N_u > N_l: the literal rule, not "all ones"
    w, it0, max_it, lr = 0.1, W.IT0, W.MAX_IT, 0.1           # (lr 0.1: the SGD step must move the eval forwards visibly)
    sd, dsd = oracle_state(23), DR.rand_state(DAN_SEED, 4, NDF, 1)
    pk = [k for k in sd if R.is_param(k)]
    for k in pk:
        sd[k].requires_grad_(True)
    with KinkMargins() as km:
        z_l = R.net_forward(sd, d["x_l"], "unet", d["m_l"], None, True)
        z_u = R.net_forward(sd, d["x_u"], "unet", d["m_u"], None, True)
    mg = []
    ce = F.cross_entropy(z_l, d["lab"].long())
    dice = R.dice(torch.softmax(z_l, 1), d["lab"].long().unsqueeze(1))
    cons = F.cross_entropy(DR.forward(dsd, torch.softmax(z_u, 1), d["x_u"], None, 1, mg), t_u)
    assert km.leaky >= 4e-6 and km.pool >= 1e-6 and min(mg) >= 1e-4, ("the batch is not kink-clear any more", km.leaky, km.pool, min(mg))
    loss = 0.5 * (dice + ce) + w * cons
    loss.backward()
    # ---- engine: generator update
    eng = make_engine(base_lr=lr, max_iterations=max_it, consistency=w, consistency_rampup=0)
    eng.it = it0
    D = eng.discriminator
    dan_before = (D._param_arena.clone(), eng.dan_m.clone(), eng.dan_v.clone())
    x_l, lab, x_u = T(d["x_l"]), T(d["lab"]), T(d["x_u"])
    eng.forward_backward(x_l, lab, unlabeled=x_u, masks=(TL(d["m_l"]), TL(d["m_u"])))
    o = eng.losses()
    print(f"DAN-STEP [{mode}] losses {o}; oracle loss {loss.item():.6f} ce {ce.item():.6f} dice {dice.item():.6f} cons {cons.item():.6f}")
    assert rel_err([o["loss"], o["ce"], o["dice"], o["cons"]], [loss.item(), ce.item(), dice.item(), cons.item()]) < TOL, o
    assert abs(o["cons"] - cons.item()) <= TOL * abs(cons.item()) and o["w"] == w
    assert o["loss"] == pytest.approx(o["sup"] + o["w"] * o["cons"], rel=1e-6)
    g_eng, off, bad = eng.model.flat_grads().cpu().numpy(), 0, []
    for k in pk:
        n = sd[k].numel()
        ref = sd[k].grad.numpy().ravel()
        err = float(np.abs(g_eng[off:off + n] - ref).max())
        if err > grad_tol(k, ref, TOL):
            bad.append((k, err, float(np.abs(ref).max())))
        off += n
    assert not bad, bad[:6]
    pre_sgd = {k: v.detach().clone() for k, v in sd.items()}
    with torch.no_grad():                                    # the oracle's own SGD step: sd becomes the post-SGD state
        ps = [sd[k] for k in pk]
        R.sgd_step(ps, [p.grad for p in ps], [torch.zeros_like(p) for p in ps], lr, first=False)
    post = {k: v.detach() for k, v in sd.items()}
    eng.optimizer_step()
    assert all(torch.equal(a, b) for a, b in zip(dan_before, (D._param_arena, eng.dan_m, eng.dan_v))) and eng.dan_it == 0
    # ---- engine: discriminator update
    m = eng.model
    net_before = (m._param_arena.clone(), m._grad_arena.clone(), m._buf_arena.clone(), m._nbt.clone())

    def adversary_loss(state, dmasks):
        with torch.no_grad():
            s = torch.cat([torch.softmax(R.net_forward(state, x, "unet", None, None, False), 1) for x in (d["x_l"], d["x_u"])], 0)
        p = {k: v.clone().requires_grad_() for k, v in dsd.items()}
        mg2 = []
        dl = F.cross_entropy(DR.forward(p, s, torch.cat([d["x_l"], d["x_u"]], 0), dmasks, 1, mg2), t_full)
        dl.backward()
        return dl.item(), p, min(mg2)
    g = torch.Generator().manual_seed(5)
    dmasks = [(torch.rand((n_l + n_u, c * NDF), generator=g) >= 0.5).float() * 2 for c in (2, 4)]
    dl_post, p_post, margin = adversary_loss(post, dmasks)
    # the adversary's pre-activations are of order 1 and sums of at most 512 float32 products (error some 1e-6 at worst): the 4e-6 this
    # project asks of a kink-clear batch (tests/test_dp.py).  The smallest one sits in conv2's output, in front of any dropout, so it is a
    # property of the batch and not of the mask draw
    assert margin >= 4e-6, margin
    dl_pre, _, _ = adversary_loss(pre_sgd, dmasks)
    eng.discriminator_step(x_l, x_u, TL(dmasks))
    assert all(torch.equal(a, b) for a, b in zip(net_before, (m._param_arena, m._grad_arena, m._buf_arena, m._nbt))) and m.training
    for k in pk:                                             # (the net the update saw is the oracle's post-SGD one)
        assert close(m.state_dict()[k].detach().cpu().numpy(), post[k].numpy(), TOL), k
    got = eng.losses()["dan_loss"]
    print(f"DAN-STEP [{mode}] dan_loss {got:.6f}; oracle on the post-SGD state {dl_post:.6f}, on the pre-SGD state {dl_pre:.6f}")
    assert abs(dl_post - dl_pre) > 20 * TOL * abs(dl_post)              # the two states are told apart ...
    assert abs(got - dl_post) <= TOL * abs(dl_post)                    # ... and the update saw the post-SGD weights and statistics
    gd = D.flat_grads().cpu().numpy()
    off = 0
    for k, _ in DR.state_shapes(4, NDF, 1):
        ref = p_post[k].grad.numpy().ravel()
        assert np.abs(gd[off:off + ref.size] - ref).max() <= grad_tol(k, ref, TOL), k
        off += ref.size
    ok, err = adam_update_ok(dan_before[0][:D.n_param].cpu().numpy(), D.flat_params().detach().cpu().numpy(), gd)
    assert ok and eng.dan_it == 1, err


# ------------------------------------------------------------------------------------------------ schedule, refusals
def test_weight_schedule_and_refusals(mode):
    """w(t) = consistency * sigmoid_rampup(it // 150, consistency_rampup): 150, where the other semi_* compositions divide by 300"""
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    eng = TrainEngine("unet", 1, 4, loss="semi_dan", dan_ndf=NDF)
    assert (eng.consistency, eng.consistency_rampup, eng.dan_lr, eng.dan_betas, eng.discriminator.pool) == (0.1, 200.0, 1e-4, (0.9, 0.99), 7)
    for it in (0, 149, 150, 299, 300, 30000):
        eng.it = it
        assert eng.consistency_weight() == pytest.approx(weight_formula(it), rel=1e-12), it
    assert eng.consistency_weight(149) == eng.consistency_weight(0) < eng.consistency_weight(150) < eng.consistency_weight(300)
    assert eng.consistency_weight(150) != TrainEngine("unet", 1, 4, loss="semi_entmin").consistency_weight(150)
    assert eng.consistency_weight(30000) == pytest.approx(0.1)
    assert type(eng.discriminator).__name__ == "FCDiscriminator" and eng.discriminator.ndf == NDF
    with pytest.raises(_lib.WslError, match="single-decoder"):
        TrainEngine("unet_cct", 1, 4, loss="semi_dan")
    with pytest.raises(_lib.WslError, match="unlabeled"):
        eng.step(T(torch.zeros(2, 1, 32, 32)), T(torch.zeros(2, 32, 32, dtype=torch.uint8)))
    with pytest.raises(_lib.WslError, match="semi_dan"):
        TrainEngine("unet", 1, 4, loss="semi_entmin").discriminator_step(T(torch.zeros(2, 1, 32, 32)), T(torch.zeros(2, 1, 32, 32)))
    assert TrainEngine("unet", 1, 4, loss="semi_entmin").discriminator is None


# ------------------------------------------------------------------------------------------------ the module path
def test_module_path_loop_against_the_engine(mode):
    """the reference's loop on this package's modules -- net_factory's UNet, FCDiscriminator, torch.optim.SGD and
    torch.optim.Adam -- with its one re-ordering (sup.backward() before the second training forward) gives the engine's step: losses to
    1e-4, the net's parameters to 1e-6, the adversary's Adam updates to 1e-4 of lr"""
    from oracle import torch_ref as R
    from wsl4mis_amd.networks.discriminator import FCDiscriminator
    from wsl4mis_amd.networks.net_factory import net_factory
    d = W.semi_inputs(W.SHARD_SEEDS[0], *W.SHARD_SHAPE)
    w = 0.1
    x_l, lab, x_u = T(d["x_l"]), T(d["lab"]), T(d["x_u"])
    t_full, t_u = (T(t) for t in dan_targets(2, 2))
    dmasks = TL(DW.dan_masks(0, 4))
    eng = make_engine(consistency=w, consistency_rampup=0)
    dan0 = eng.discriminator.flat_params().detach().cpu().numpy().copy()
    eng.step(x_l, lab, unlabeled=x_u, masks=(TL(d["m_l"]), TL(d["m_u"])), dan_masks=dmasks)
    o = eng.losses()
    # ---- the loop
    model = net_factory("unet", 1, 4)
    load_det(model, 23)
    DAN = FCDiscriminator(4, ndf=NDF, n_channel=1, pool=1).cuda()
    DAN.load_state_dict(DR.rand_state(DAN_SEED, 4, NDF, 1))
    optimizer = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)
    DAN_optimizer = torch.optim.Adam(DAN.parameters(), lr=0.0001, betas=(0.9, 0.99))
    seq = iter((TL(d["m_l"]), TL(d["m_u"])))
    model.set_dropout_masks(lambda n, h, w_: (next(seq), None))
    model.train()
    DAN.eval()
    optimizer.zero_grad()
    outputs_labeled = model(x_l)
    loss_ce = F.cross_entropy(outputs_labeled, lab.long())
    loss_dice = R.dice(torch.softmax(outputs_labeled, 1), lab.long().unsqueeze(1))
    supervised_loss = 0.5 * (loss_dice + loss_ce)
    supervised_loss.backward()                               # the one re-ordering: before the second training forward
    outputs_unlabeled = model(x_u)
    consistency_loss = F.cross_entropy(DAN(torch.softmax(outputs_unlabeled, 1), x_u), t_u.long())
    (w * consistency_loss).backward()
    optimizer.step()
    model.set_dropout_masks(None)                            # (the replayed student masks are used up; eval forwards draw none)
    model.eval()
    DAN.train()
    DAN.set_dropout_masks(dmasks)
    with torch.no_grad():
        soft = torch.cat([torch.softmax(model(x_l), 1), torch.softmax(model(x_u), 1)], 0)
    DAN_loss = F.cross_entropy(DAN(soft, torch.cat([x_l, x_u], 0)), t_full.long())
    DAN_optimizer.zero_grad()
    DAN_loss.backward()
    g_mod = torch.cat([p.grad.reshape(-1) for p in DAN.parameters()]).cpu().numpy().astype(np.float64)
    DAN_optimizer.step()
    ref = [0.5 * (loss_dice.item() + loss_ce.item()) + w * consistency_loss.item(), loss_ce.item(), loss_dice.item(), consistency_loss.item(), DAN_loss.item()]
    assert rel_err([o["loss"], o["ce"], o["dice"], o["cons"], o["dan_loss"]], ref) < TOL, (o, ref)
    got = eng.model.state_dict()
    for k, p in model.named_parameters():
        assert rel_err(got[k].cpu(), p.detach().cpu()) < 1e-6, k
    for k, b in model.named_buffers():
        assert rel_err(got[k].cpu().double(), b.detach().cpu().double()) < 1e-6, k
    # the adversary: the same gradient (the engine's fused head against torch's cross entropy on the module's logits), then the same update.
    # Adam's first update is lr * g / (|g| + eps): where |g| is not far above eps = 1e-8 it is ill-conditioned in g -- its derivative is
    # lr * eps / (|g| + eps)^2 -- so each element's allowance is 1e-4 of lr, the rounding of storing p, and the two paths' ACTUAL gradient
    # difference carried through that derivative (twice, for the second order)
    g_eng = eng.discriminator.flat_grads().cpu().numpy().astype(np.float64)
    off = 0
    for k, shape in DR.state_shapes(4, NDF, 1):
        n = int(np.prod(shape))
        assert np.abs(g_eng[off:off + n] - g_mod[off:off + n]).max() <= grad_tol(k, g_mod[off:off + n], TOL), k
        off += n
    a, b = eng.discriminator.flat_params().detach().cpu().numpy().astype(np.float64), DAN.flat_params().detach().cpu().numpy().astype(np.float64)
    carried = 2 * LR_DAN * EPS * np.abs(g_eng - g_mod) / (np.minimum(np.abs(g_eng), np.abs(g_mod)) + EPS) ** 2
    err = np.abs((a - dan0) - (b - dan0))
    print(f"DAN-LOOP [{mode}] worst Adam update difference {err.max():.2e}; without the carried gradient difference {np.sum(err > 1e-4 * LR_DAN + 2.0 ** -23 * np.abs(dan0))} "
          f"of {err.size} elements exceed 1e-4 of lr")
    assert np.all(err <= 1e-4 * LR_DAN + 2.0 ** -23 * np.abs(dan0) + carried), float(err.max())
    assert float(np.abs(a - dan0).max()) > 0.5 * LR_DAN      # (Adam's first step moves by about lr)


# ------------------------------------------------------------------------------------------------ the example
def test_example_trainer_runs_semi_dan(mode, tmp_path):
    """--loss semi_dan end to end on the committed ACDC fixture, fold3: 32 x 32 patches with --dan_pool 1 --dan_ndf 8 (the smallest legal
    adversary), the model defaults to unet, every logged loss is sup + w * cons and carries the adversary's own loss"""
    spec = importlib.util.spec_from_file_location("train_acdc_dan", os.path.join(ROOT, "examples", "train_acdc_scribble.py"))
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
        hist = mod.main(["--root_path", ACDC, "--fold", "fold3", "--loss", "semi_dan", "--max_iterations", "2", "--batch_size", "4",
                         "--patch_size", "32", "32", "--val_every", "1000", "--log_every", "1", "--consistency", "0.2", "--consistency_rampup", "0",
                         "--dan_pool", "1", "--dan_ndf", "8", "--quiet", "--curve_json", curve])
    finally:
        mod.TrainEngine = real
    eng = seen["eng"]
    assert eng.loss_kind == "semi_dan" and type(eng.model).__name__ == "UNet" and eng.it == 2 and eng.dan_it == 2
    assert (eng.discriminator.pool, eng.discriminator.ndf) == (1, 8)
    assert len(hist) == 2 and all(np.isfinite(l) for _, l in hist)
    log = json.load(open(curve))["curve"]
    assert len(log) == 2 and all(r["w"] == 0.2 and r["n_valid"] == 2 * 1024 and r["cons"] > 0 and r["dan_loss"] > 0 for r in log)
    assert all(abs(r["loss"] - (r["sup"] + 0.2 * r["cons"])) < 1e-5 for r in log)


# ------------------------------------------------------------------------------------------------ data parallel
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_gloo_discriminator_update(tmp_path):
    """two gloo ranks on the emulator, each with its own 2 + 2 shard: both end the step with bit-identical discriminator (and net)
    parameters, and those equal one Adam step on the MEAN of the two ranks' 1-rank discriminator gradients from the same state"""
    get_backend("emul")
    port = str(_free_port())
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dan_dp_worker.py"), str(r), "2", port, str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=1500)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    assert np.array_equal(r0["dan_before"], r1["dan_before"]) and np.array_equal(r0["net_after"], r1["net_after"])
    assert np.array_equal(r0["dan_after"], r1["dan_after"])
    assert not np.array_equal(r0["shard_grad"], r1["shard_grad"]) and float(r0["dan_loss"]) != float(r1["dan_loss"])
    mean = 0.5 * (r0["shard_grad"].astype(np.float64) + r1["shard_grad"].astype(np.float64))
    ok, err = adam_update_ok(r0["dan_before"], r0["dan_after"], mean)
    assert ok, err
    only0, _ = adam_update_ok(r0["dan_before"], r0["dan_after"], r0["shard_grad"])
    assert not only0                                          # (the check tells the mean from one shard's gradient)


# ------------------------------------------------------------------------------------------------ the reference's recipe
def _unpack(g, key, n, P):
    return [T(np.unpackbits(g[f"{key}_em{l}"])[:n * (16 << l) * (P >> l) * (P >> l)].reshape(n, 16 << l, P >> l, P >> l)) for l in range(5)]


def test_engine_follows_the_reference_recipe(mode):
    """the trainer's loop on the reference's own UNet and FCDiscriminator (fixture g16_dan_recipe): {loss, ce, dice, cons, dan_loss} of
    every step against the float64 run within the fixture's bounds (profiles/dan_margins.md: derived from the reference's own fp32-fp64
    spread), and after the last step the net's tensors and the adversary's tensors (against their change over the run).  The emulator leg
    runs the first two steps."""
    g = golden("g16_dan_recipe")
    cons, ramp, max_it, lr, s_seed, d_seed, ndf = (float(v) for v in g["meta_hyper"])
    b_first, b_all, b_net, b_dan = (float(v) for v in g["meta_bounds"])
    xl, xu, lab = g["in_xl"], g["in_xu"], g["in_lab"]
    steps_all, n, P = xl.shape[0], xl.shape[1], xl.shape[3]
    steps = 2 if mode == "emul" else steps_all
    from wsl4mis_amd.engine import TrainEngine
    eng = TrainEngine("unet", 1, 4, base_lr=lr, max_iterations=int(max_it), loss="semi_dan", consistency=cons, consistency_rampup=ramp,
                      dan_ndf=int(ndf), dan_pool=1)
    load_det(eng.model, int(s_seed))
    eng.discriminator.load_state_dict(DR.rand_state(int(d_seed), 4, int(ndf), 1))
    got = []
    for it in range(steps):
        eng.step(T(xl[it]), T(lab[it]), unlabeled=T(xu[it]), masks=(_unpack(g, f"s{it}_l", n, P), _unpack(g, f"s{it}_u", n, P)),
                 dan_masks=[T(g[f"s{it}_d_cm0"]), T(g[f"s{it}_d_cm1"])])
        o = eng.losses()
        got.append([o["loss"], o["ce"], o["dice"], o["cons"], o["dan_loss"]])
    got, ref = np.array(got), g["meta_losses_f64"][:steps]
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"DAN-RECIPE [{mode}] worst relative loss error per step {rel.max(1)} (bounds {b_first:g} first two, {b_all:g} all)")
    assert rel[:2].max() <= b_first and rel.max() <= b_all, rel
    if steps == steps_all:
        sd, dsd = eng.model.state_dict(), eng.discriminator.state_dict()
        for k in [f for f in g.files if f.startswith("final_f64:")]:
            name, ref64 = k.split(":", 1)[1], g[k]
            if name.startswith("dan."):
                cur = dsd[name[4:]].detach().cpu().double().numpy().ravel()[:256]
                den, bound = np.abs(ref64 - g["final_init:" + name]).max(), b_dan
            else:
                cur = sd[name].detach().cpu().double().numpy().ravel()[:256]
                den, bound = np.abs(ref64).max(), b_net
            err = float(np.abs(cur - ref64).max() / (den + 1e-12))
            print(f"DAN-RECIPE [{mode}] {name}: {err:.2e} (bound {bound:g})")
            assert err <= bound, (name, err)


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.gpu
def test_whole_step_is_bit_reproducible(hip):
    """two runs with the same torch.manual_seed give the same bits in losses, both networks' parameters and both gradient arenas: every
    reduction of the new kernels is order-fixed, and the library-drawn dropout masks are functions of torch's seed"""
    d = W.semi_inputs(STEP_SEED, *STEP_SHAPE)

    def run():
        eng = make_engine(consistency_rampup=0)
        torch.manual_seed(77)
        for _ in range(2):
            eng.step(T(d["x_l"]), T(d["lab"]), unlabeled=T(d["x_u"]))
        D = eng.discriminator
        return (np.array(list(eng.losses().values())), eng.model.flat_params().clone(), eng.model.flat_grads().clone(),
                D.flat_params().detach().clone(), D.flat_grads().clone(), eng.dan_m.clone(), eng.dan_v.clone())
    a, b = run(), run()
    assert np.all(np.isfinite(a[0])) and np.array_equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
