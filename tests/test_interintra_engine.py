"""Inter/intra-class variance training through the Python layer: utils.losses.{inter,intra}_class_variance / class_variance_loss,
TrainEngine(loss="pce_interintra") and the example, against the plain torch expression, the oracle and the reference's own recipe
(fixture g14_interintra_curve, tests/golden/make_golden_interintra.py).
`mode` = emul runs the Python layer against the host-emulation library with CPU tensors; `mode` = hip (gpu mark) is the real thing."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, close, get_backend, golden, rel_err, summary_line
from detinit import det_state

TOL = 1e-4
ACDC = os.path.join(ROOT, "tests", "golden", "acdc")


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


def dev():
    from wsl4mis_amd import runtime
    return runtime.device()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def load_det(model, seed):
    sd = model.state_dict()
    vals = det_state({k: tuple(v.shape) for k, v in sd.items()}, seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})


def ref_terms(p, img):
    """the trainer's two functions as plain torch: (inter, intra)"""
    q = img * p
    return torch.std(q.mean(dim=[2, 3]), dim=1).mean(), torch.std(q, dim=[2, 3]).mean()


def biased_logits(gen, shape):
    return 2.0 * torch.randn(shape, generator=gen) + torch.arange(float(shape[1])).view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------ module path
def test_module_functions_against_torch(mode):
    """values and gradients THROUGH softmax of the three functions against the float64 torch expression; a linear combination of the two
    outputs back-propagates in one call"""
    from wsl4mis_amd.utils import losses
    gen = torch.Generator().manual_seed(3)
    z0, img = biased_logits(gen, (2, 4, 24, 20)), torch.rand((2, 1, 24, 20), generator=gen) + 0.05
    zd = z0.double().requires_grad_()
    ri, ra = ref_terms(torch.softmax(zd, 1), img.double())
    for name, fn, ref in (("inter", lambda p, i: losses.inter_class_variance(p, i), ri), ("intra", lambda p, i: losses.intra_class_variance(p, i), ra),
                          ("loss", lambda p, i: losses.class_variance_loss(p, i), ri - ra),
                          ("combination", lambda p, i: 0.3 * losses.inter_class_variance(p, i) - 0.7 * losses.intra_class_variance(p, i), 0.3 * ri - 0.7 * ra)):
        z = T(z0.numpy()).requires_grad_()
        v = fn(losses.softmax(z), T(img.numpy()))
        v.backward()
        zd.grad = None
        ref.backward(retain_graph=True)
        assert rel_err(v.item(), ref.item()) < 1e-5, (name, v.item(), ref.item())
        assert close(z.grad.cpu().numpy(), zd.grad.numpy(), TOL), name


def test_module_functions_refuse_what_is_not_built(mode):
    from wsl4mis_amd import _lib
    from wsl4mis_amd.utils import losses
    gen = torch.Generator().manual_seed(4)
    p = T(torch.softmax(torch.randn((2, 4, 8, 8), generator=gen), 1).numpy())
    img = T(torch.rand((2, 1, 8, 8), generator=gen).numpy())
    with pytest.raises(NotImplementedError):                     # multi-channel image
        losses.intra_class_variance(p, T(torch.rand((2, 3, 8, 8), generator=gen).numpy()))
    with pytest.raises(NotImplementedError):                     # gradient with respect to the image
        losses.class_variance_loss(p, img.clone().requires_grad_())
    with pytest.raises(_lib.WslError):                           # one class: torch returns NaN, the entry point WSL_EINVAL
        losses.inter_class_variance(p[:, :1].contiguous(), img)
    with pytest.raises(_lib.WslError):                           # one pixel
        losses.intra_class_variance(p[:, :, :1, :1].contiguous(), img[:, :, :1, :1].contiguous())


# ------------------------------------------------------------------------------------------------ one step against the oracle
def _torch_loss(z, x, lab, w):
    ce = torch.nn.functional.cross_entropy(z, lab.long(), ignore_index=4)
    inter, intra = ref_terms(torch.softmax(z, 1), x)
    return ce + w * (inter - intra), ce, inter, intra


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
def test_engine_step_against_oracle_unet(mode, fused):
    """one engine step: losses to 1e-4, the logit gradient the loss head hands to the network by close(), parameters after SGD by close()
    -- against the oracle's UNet forward, the trainer's loss lines on torch ops and the oracle's SGD.  The batch, weights and masks are
    those of test_s2l_engine.py::test_engine_step_from_thr_iter_on_against_oracle (same draws in the same order), whose forward keeps
    every pre-activation clear of the LeakyReLU kink and every max-pool window clear of a tie (asserted).
    (Parameter GRADIENTS are not compared here: on this 3 x 16 x 16 batch the untouched network's plain `pce` gradients already differ
    from the float32 oracle by 1.6e-4 of a tensor's scale and from the float64 one by 1.1e-4, measured; the composition's own gradient
    is what the head writes, and that is compared.)"""
    from netutil import KinkMargins
    from oracle import torch_ref as R
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import scribble_labels
    N, S, w = 3, 16, 0.1
    gen = torch.Generator().manual_seed(42)
    x = torch.rand((N, 1, S, S), generator=gen)
    lab = torch.from_numpy(scribble_labels(N, S, S, 4, share=0.08))
    torch.rand((N, S, S, 4), generator=gen), torch.rand((N, S, S), generator=gen), torch.randint(0, 4, (N, S, S), generator=gen)
    masks = [(torch.rand((N, 16 << l, S >> l, S >> l), generator=gen) >= R.DROP[l]).to(torch.uint8) for l in range(5)]
    eng = TrainEngine("unet", 1, 4, base_lr=0.01, loss="pce_interintra", var_consistency=w, var_rampup=0)
    eng.fused_heads = fused
    load_det(eng.model, 23)
    eng.it = 5
    eng.model.set_dropout_masks([T(m.numpy()) for m in masks])
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in det_state(
        {k: tuple(v.shape) for k, v in eng.model.state_dict().items()}, 23).items()}
    pk = [k for k in sd if R.is_param(k)]
    for k in pk:
        sd[k].requires_grad_(True)
    with KinkMargins() as km:
        z = R.net_forward(sd, x, "unet", masks, None, True)
    assert km.leaky >= 1e-5 and km.pool >= 1e-5, ("the batch is not kink-clear any more", km.leaky, km.pool)
    z.retain_grad()
    loss, ce, inter, intra = _torch_loss(z, x, lab, w)
    loss.backward()
    with torch.no_grad():
        ps = [sd[k] for k in pk]
        R.sgd_step(ps, [p.grad for p in ps], [torch.zeros_like(p) for p in ps], 0.01, first=False)
    eng.forward_backward(T(x.numpy()), T(lab.numpy()))
    o = eng.losses()
    assert close(eng._tensors(N, S, S)["dz1"].cpu().numpy(), z.grad.numpy(), TOL)
    eng.optimizer_step()
    assert rel_err([o["loss"], o["ce"], o["inter"], o["intra"], o["reg"]],
                   [loss.item(), ce.item(), inter.item(), intra.item(), inter.item() - intra.item()]) < TOL, o
    assert o["w"] == w and o["n_valid"] == int((lab != 4).sum())
    got = eng.model.state_dict()
    for k in pk:
        assert close(got[k].detach().cpu().numpy(), sd[k].detach().numpy(), TOL), k


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
def test_engine_step_against_module_path_pnet(fused):
    """the same step on PNet2D.  The oracle has no PNet forward, so -- as tests/test_pnet_engine.py does for the other compositions -- the
    reference is the package's own PNet module under autograd with the trainer's loss lines on torch ops and torch's SGD: losses to 1e-4,
    gradients by close(), parameters after the step to 1e-6.  Device only: PNet's 64-channel dilated stack is minutes on the emulator"""
    from wsl4mis_amd import _lib, runtime
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.networks.net_factory import net_factory
    from wsl4mis_amd.synthetic import scribble_labels
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    d = torch.device("cuda:0")
    N, S, w = 2, 32, 0.1
    gen = torch.Generator().manual_seed(17)
    x = torch.rand((N, 1, S, S), generator=gen).to(d)
    lab = torch.from_numpy(scribble_labels(N, S, S, 4, share=0.08)).to(d)
    ms = [((torch.rand((N, c), generator=gen) >= 0.3).float() / 0.7).to(d) for c in (128, 64)]
    eng = TrainEngine("pnet", 1, 4, loss="pce_interintra", var_consistency=w, var_rampup=0)
    eng.fused_heads = fused
    load_det(eng.model, 31)
    eng.model.set_dropout_masks(ms)
    eng.forward_backward(x, lab)
    o, g_eng = eng.losses(), eng.model.flat_grads().clone()
    eng.optimizer_step()
    model = net_factory("pnet", 1, 4)
    load_det(model, 31)
    model.train()
    model.set_dropout_masks(ms)
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    loss, ce, inter, intra = _torch_loss(model(x), x, lab, w)
    opt.zero_grad()
    loss.backward()
    assert rel_err([o["loss"], o["ce"], o["inter"], o["intra"]], [loss.item(), ce.item(), inter.item(), intra.item()]) < TOL, o
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


# ------------------------------------------------------------------------------------------------ schedule, refusals
def _formula(it, consistency=0.1, rampup=200.0):
    t = min(max(float(it // 150), 0.0), rampup) / rampup
    return consistency * math.exp(-5.0 * (1.0 - t) ** 2)


def test_weight_schedule(mode):
    """w(t) = var_consistency * sigmoid_rampup(it // 150, var_rampup) with `it` before its increment; var_rampup = 0: the constant"""
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import scribble_labels
    eng = TrainEngine("unet", 1, 4, loss="pce_interintra")
    assert (eng.var_consistency, eng.var_rampup) == (0.1, 200.0)
    for it in (0, 149, 150, 30000):
        eng.it = it
        assert eng.var_weight() == pytest.approx(_formula(it), rel=1e-12), it
    assert eng.var_weight(0) == eng.var_weight(149) == pytest.approx(0.1 * math.exp(-5.0)) and eng.var_weight(150) > eng.var_weight(149)
    assert eng.var_weight(30000) == pytest.approx(0.1)
    assert TrainEngine("unet", 1, 4, loss="pce_interintra", var_rampup=0).var_weight() == 0.1
    # the weight a step uses is the one of `it` BEFORE the increment, and it is what losses() reports
    gen = torch.Generator().manual_seed(5)
    x, lab = torch.rand((2, 1, 16, 16), generator=gen), scribble_labels(2, 16, 16, 4, share=0.08)
    load_det(eng.model, 23)
    eng.it = 150
    eng.step(T(x.numpy()), T(lab))
    o = eng.losses()
    assert eng.it == 151 and o["w"] == pytest.approx(_formula(150), rel=1e-12) and o["w"] != _formula(149)
    assert o["loss"] == pytest.approx(o["ce"] + o["w"] * o["reg"], rel=1e-6) and o["reg"] == pytest.approx(o["inter"] - o["intra"], abs=1e-6)
    assert set(o) == {"loss", "ce", "reg", "inter", "intra", "w", "n_valid"}


def test_interintra_is_single_decoder_only(mode):
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    with pytest.raises(_lib.WslError, match="single-decoder"):
        TrainEngine("unet_cct", 1, 4, loss="pce_interintra")
    assert TrainEngine("pnet", 1, 4, loss="pce_interintra").loss_kind == "pce_interintra"


# ------------------------------------------------------------------------------------------------ the reference's recipe
def unpack_masks(g, prefix, N, H, W):
    return [T(np.unpackbits(g[f"{prefix}_em{l}"])[:N * (16 << l) * (H >> l) * (W >> l)].reshape(N, 16 << l, H >> l, W >> l)) for l in range(5)]


def run_recipe(steps):
    from wsl4mis_amd.engine import TrainEngine
    g = golden("g14_interintra_curve")
    w, ramp = g["meta_hyper"]
    xs, labs = g["in_xs"], g["in_labels"]
    N, P = xs.shape[1], xs.shape[3]
    eng = TrainEngine("unet", 1, 4, base_lr=0.01, max_iterations=30000, loss="pce_interintra", var_consistency=float(w), var_rampup=float(ramp))
    load_det(eng.model, 41)
    got = []
    for it in range(steps):
        eng.model.set_dropout_masks(unpack_masks(g, f"s{it}", N, P, P))
        eng.step(T(xs[it]), T(labs[it]))
        o = eng.losses()
        got.append([o["loss"], o["ce"], o["inter"], o["intra"]])
    return np.array(got), g, eng


def test_engine_follows_the_reference_recipe(mode):
    """six steps of the trainer's loop on the reference's UNet (constant weight 0.1): loss, ce, inter and intra per step against the
    reference's float32 run -- the first two steps to 1e-4, the tail to 3e-2 (the criteria test_s2l_engine.py applies to g13_s2l_curve),
    and the first 256 values of three final tensors to 5e-2.  The fixture's own float32-vs-float64 spread is reported next to the
    measured error.  The emulator leg runs the two tightly bounded steps only (a 4 x 32 x 32 step takes the host emulator ten seconds)."""
    steps = 2 if mode == "emul" else 6
    got, g, eng = run_recipe(steps)
    ref, ref64 = g["meta_losses_f32"][:steps], g["meta_losses_f64"][:steps]
    rel = np.abs(got - ref) / np.abs(ref)
    spread = np.abs(ref - ref64) / np.abs(ref64)
    summary_line(f"INTERINTRA-CURVE [{mode}]: worst rel. error per step over (loss, ce, inter, intra) {np.array2string(rel.max(1), precision=2)}; "
                 f"the reference's own fp32-vs-fp64 spread {np.array2string(spread.max(1), precision=2)}")
    assert np.all(np.isfinite(got))
    assert np.max(rel[:2]) < 1e-4, (got, ref)
    assert np.max(rel) < 3e-2, (got, ref)
    if steps == 6:
        sd = eng.model.state_dict()
        for k in [k[10:] for k in g.files if k.startswith("final_f32:")]:
            assert rel_err(sd[k].cpu().numpy().ravel()[:256], g["final_f32:" + k]) < 5e-2, k


def small_run(fused):
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import scribble_labels
    rng = np.random.default_rng(9)
    N, S = 2, 16
    eng = TrainEngine("unet", 1, 4, loss="pce_interintra", var_rampup=0)
    eng.fused_heads = fused
    load_det(eng.model, 23)
    torch.manual_seed(77)
    eng.step(T(rng.random((N, 1, S, S), dtype=np.float32)), T(scribble_labels(N, S, S, 4, share=0.08)))
    return np.array(list(eng.losses().values())), eng.model.flat_params().clone(), eng.model.flat_grads().clone(), eng.loss_out.clone()


@pytest.mark.parametrize("fused", [True, pytest.param(False, marks=pytest.mark.gpu)], ids=["fused", "chain"])
def test_whole_step_is_bit_reproducible(mode, fused):
    """two runs give the same bits in losses, parameters and gradients: every reduction of the class-variance kernels is order-fixed and
    library-drawn dropout is a function of torch's seed.  (The chain of calls runs on the device only: the same kernels, and a network
    step costs the host emulator ten seconds.)"""
    a, b = small_run(fused), small_run(fused)
    assert np.all(np.isfinite(a[0])) and a[0][3] > 0 and a[0][4] > 0
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------ the example
def test_example_trainer_runs_interintra(mode, tmp_path):
    """--loss pce_interintra end to end on the committed ACDC fixture slices: the model defaults to unet, --consistency /
    --consistency_rampup reach the engine, every logged loss is ce + w * (inter - intra)"""
    spec = importlib.util.spec_from_file_location("train_acdc_interintra", os.path.join(ROOT, "examples", "train_acdc_scribble.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    curve = os.path.join(str(tmp_path), "curve.json")
    hist = mod.main(["--root_path", ACDC, "--fold", "fold3", "--loss", "pce_interintra", "--max_iterations", "2", "--batch_size", "2",
                     "--patch_size", "16", "16", "--val_every", "1000", "--log_every", "1", "--consistency", "0.2", "--consistency_rampup", "0",
                     "--quiet", "--curve_json", curve])
    assert len(hist) == 2 and all(np.isfinite(l) for _, l in hist)
    log = json.load(open(curve))["curve"]
    assert all(r["w"] == 0.2 and r["intra"] > 0 and r["inter"] > 0 for r in log)
    assert all(abs(r["loss"] - (r["ce"] + 0.2 * (r["inter"] - r["intra"]))) < 1e-5 for r in log)
