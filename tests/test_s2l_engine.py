"""Scribble2Label through the Python layer: utils.losses.s2l_loss, TrainEngine(loss="s2l") and update_ensemble against the
reference's own recipe (fixtures g13_s2l_head / g13_s2l_curve, tests/golden/make_golden_s2l.py) and the oracle.
`mode` = emul runs the Python layer against the host-emulation library with CPU tensors; `mode` = hip (gpu mark) is the real thing."""
import random

import numpy as np
import pytest
import torch

from conftest import close, get_backend, golden, rel_err, summary_line
from detinit import det_state

TOL = 1e-4


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


# ------------------------------------------------------------------------------------------------ module path
@pytest.mark.parametrize("tag", ["a", "b"])
def test_s2l_loss_value_and_gradient(mode, tag):
    from wsl4mis_amd.utils import losses
    g = golden("g13_s2l_head")
    z = T(g[f"{tag}_z"]).requires_grad_()
    loss, ce, cu = losses.s2l_loss(z, T(g[f"{tag}_scribble"]), T(g[f"{tag}_weight"]), thr_conf=float(g[f"{tag}_thr"]))
    (2.0 * loss).backward()
    assert close([loss.item(), ce.item(), cu.item()], g[f"{tag}_losses"], TOL)
    assert close(z.grad.cpu().numpy(), 2.0 * g[f"{tag}_dz"], TOL)
    _, parts, u = losses.s2l_head(z.detach(), T(g[f"{tag}_scribble"]), T(g[f"{tag}_weight"]), thr_conf=float(g[f"{tag}_thr"]))
    assert np.array_equal(u.cpu().numpy(), g[f"{tag}_u"]) and [int(parts[3]), int(parts[4])] == [int(v) for v in g[f"{tag}_counts"]]


def test_s2l_loss_nan_without_a_confident_pixel(mode):
    """the reference's loss is NaN then (CE over no valid pixel); the gradient of the scribble CE stays finite"""
    from wsl4mis_amd.utils import losses
    g = golden("g13_s2l_head")
    z = T(g["c_z"]).requires_grad_()
    loss, ce, cu = losses.s2l_loss(z, T(g["c_scribble"]), T(g["c_weight"]), thr_conf=0.8)
    loss.backward()
    assert np.isnan(loss.item()) and np.isnan(cu.item()) and close(ce.item(), g["c_losses"][1], TOL)
    assert close(z.grad.cpu().numpy(), g["c_dz"], TOL)
    with pytest.raises(Exception):
        losses.s2l_loss(z, T(g["c_scribble"]), T(g["c_weight"][..., :3].copy()))


# ------------------------------------------------------------------------------------------------ one step against the oracle
def test_engine_step_from_thr_iter_on_against_oracle(mode):
    """one engine step with the fused head: losses to 1e-4, parameters after SGD by close().  The weight batch is built here, not
    read from a fixture: g13_s2l_head's maps are 24 x 20, which the net does not accept (no multiple of 16), and no fixture holds a
    full parameter set after a step -- so the reference is the oracle's UNet forward with the reference's loss on torch ops and the
    oracle's SGD.  The head against the fixture's planted weights is test_s2l_loss_value_and_gradient, the engine against the
    reference's recorded recipe is test_engine_follows_the_reference_recipe.  The batch is one whose forward keeps
    every pre-activation clear of the LeakyReLU kink and every max-pool window clear of a tie by more than fp32 noise (asserted
    below, as __graft_entry__.smoke() does): gradient parity of two fp32 implementations is only defined there"""
    from netutil import KinkMargins
    from oracle import torch_ref as R
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import scribble_labels
    N, S, thr = 3, 16, 0.8
    gen = torch.Generator().manual_seed(42)
    x = torch.rand((N, 1, S, S), generator=gen)
    lab = torch.from_numpy(scribble_labels(N, S, S, 4, share=0.08))
    w = torch.rand((N, S, S, 4), generator=gen) * 0.7
    hot = torch.rand((N, S, S), generator=gen) < 0.4
    w[hot, torch.randint(0, 4, (N, S, S), generator=gen)[hot]] = 0.93
    masks = [(torch.rand((N, 16 << l, S >> l, S >> l), generator=gen) >= R.DROP[l]).to(torch.uint8) for l in range(5)]
    eng = TrainEngine("unet", 1, 4, base_lr=0.01, loss="s2l", thr_iter=5, thr_conf=thr)
    load_det(eng.model, 23)
    eng.it = 5
    eng.model.set_dropout_masks([T(m.numpy()) for m in masks])
    # ---- oracle: the oracle's UNet forward, the reference's loss lines on torch ops, SGD
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in det_state(
        {k: tuple(v.shape) for k, v in eng.model.state_dict().items()}, 23).items()}
    pk = [k for k in sd if R.is_param(k)]
    for k in pk:
        sd[k].requires_grad_(True)
    with KinkMargins() as km:
        z = R.net_forward(sd, x, "unet", masks, None, True)
    assert km.leaky >= 1e-5 and km.pool >= 1e-5, ("the batch is not kink-clear any more", km.leaky, km.pool)
    ce = torch.nn.functional.cross_entropy(z, lab.long(), ignore_index=4)
    u = torch.full((N, S, S), 4, dtype=torch.long)
    for c in range(4):
        u[(w[..., c] > thr) & (lab == 4)] = c
    cu = torch.nn.functional.cross_entropy(z, u, ignore_index=4)
    loss = ce + 0.5 * cu
    loss.backward()
    with torch.no_grad():
        ps = [sd[k] for k in pk]
        R.sgd_step(ps, [p.grad for p in ps], [torch.zeros_like(p) for p in ps], 0.01, first=False)
    # ---- engine
    with pytest.raises(Exception, match="weight"):
        eng.step(T(x.numpy()), T(lab.numpy()))
    eng.step(T(x.numpy()), T(lab.numpy()), weight=T(w.numpy()))
    o = eng.losses()
    assert rel_err([o["loss"], o["ce"], o["ce_u"]], [loss.item(), ce.item(), cu.item()]) < TOL, o
    assert (o["n_valid"], o["n_u"]) == (int((lab != 4).sum()), int((u != 4).sum()))
    got = eng.model.state_dict()
    for k in pk:
        assert close(got[k].detach().cpu().numpy(), sd[k].detach().numpy(), TOL), k


# ------------------------------------------------------------------------------------------------ the reference's recipe
def unpack_masks(g, prefix, N, H, W):
    return [T(np.unpackbits(g[f"{prefix}_em{l}"])[:N * (16 << l) * (H >> l) * (W >> l)].reshape(N, 16 << l, H >> l, W >> l)) for l in range(5)]


def curve_dataset(g):
    from wsl4mis_amd.dataloaders.dataset_s2l import BaseDataSets_s2l
    n = len(g["meta_sizes"])
    return BaseDataSets_s2l.from_slices([{"image": g[f"in{i}_image"], "mask": g[f"in{i}_mask"], "scribble": g[f"in{i}_scribble"]}
                                         for i in range(n)])


def run_recipe(steps, updates=None, on_update=None):
    """train_s2l.py's loop on the fixture's six slices: augmentation draws, training masks and update masks replayed"""
    from wsl4mis_amd.dataloaders.dataset_s2l import BatchRandomGenerator_s2l
    from wsl4mis_amd.engine import TrainEngine
    g = golden("g13_s2l_curve")
    thr_iter, period, alpha, thr = g["meta_hyper"]
    P, N = 32, g["meta_idxs"].shape[1]
    ds = curve_dataset(g)
    aug = BatchRandomGenerator_s2l((P, P))
    eng = TrainEngine("unet", 1, 4, base_lr=0.01, max_iterations=60000, loss="s2l", thr_iter=int(thr_iter), thr_conf=float(thr),
                      s2l_alpha=float(alpha), period_iter=int(period))
    load_det(eng.model, 31)
    got = []
    for it in range(steps):
        random.seed(int(g["meta_aug_seed"]) + it), np.random.seed(int(g["meta_aug_seed"]) + it)
        image, _, scr, weight = aug([ds[int(i)] for i in g["meta_idxs"][it]])
        eng.model.set_dropout_masks(unpack_masks(g, f"s{it}", N, P, P))
        eng.step(image, scr, weight=weight)
        o = eng.losses()
        got.append([o["loss"], o["ce"], o["ce_u"], o["n_u"]])
        if eng.ensemble_due() and (updates is None or it < updates):
            eng.update_ensemble(ds, mode="reference", masks=[unpack_masks(g, f"u{it}_{i}", 1, P, P) for i in range(len(ds))],
                                patch_size=(P, P))
            if on_update:
                on_update(it, eng, ds)
    return np.array(got), g, eng, ds


def test_update_ensemble_reference_mode_against_the_reference(mode):
    """after the first step: the store of every slice by close(), and the BatchNorm running statistics -- the reference's model is in
    train() mode during the pass, so they take one momentum update per slice (6 here, on top of the training step's)"""
    seen = {}

    def check(it, eng, ds):
        if it:
            return
        g = golden("g13_s2l_curve")
        for i in range(len(ds)):
            assert close(ds.images[i]["weight"].cpu().numpy(), g[f"store0_{i}"], TOL), i
        sd = eng.model.state_dict()
        keys = [k[5:] for k in g.files if k.startswith("buf0:")]
        assert len(keys) == sum(1 for k in sd if "running_" in k or "num_batches" in k)
        for k in keys:
            ref = g["buf0:" + k]
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(ref) == 3 + 1 + len(ds), k       # det init 3, one training step, one forward per slice
            else:
                assert close(sd[k].cpu().numpy(), ref, TOL), k
        seen["ok"] = True
        assert eng.model.training and eng.model._forced_masks is None

    run_recipe(1, on_update=check)
    assert seen.get("ok")


def test_engine_follows_the_reference_recipe(mode):
    """the loss curve of train_s2l.py's loop (thr_iter 2, period_iter 1, alpha 0.6, thr_conf 0.4): the first two steps to 1e-4, the tail
    to 3e-2 (tests/test_python_api.py's criteria); n_u per step within that step's near_thr -- the store pixels within 1e-4 relative
    of thr_conf after the preceding update, the only ones a 1e-4-accurate store can flip"""
    # the emulator leg stops after the first fused step: a step with its six N = 1 update forwards takes the host emulator half a
    # minute, and what it leaves out (the 3e-2 tail, the final parameters) is arithmetic of the device code that the gpu leg checks
    steps = 3 if mode == "emul" else 6
    got, g, eng, _ = run_recipe(steps)
    ref = g["meta_losses"][:steps]
    thr_iter = int(g["meta_hyper"][0])
    assert np.all(got[:thr_iter, 2:] == 0) and np.all(np.isfinite(got))
    rel = np.abs(got[:, :2] - ref[:, :2]) / np.abs(ref[:, :2])
    relu = np.abs(got[thr_iter:, 2] - ref[thr_iter:, 2]) / np.abs(ref[thr_iter:, 2])
    dn = np.abs(got[:, 3] - g["meta_n_u"][:steps]).astype(int)
    summary_line(f"S2L-CURVE [{mode}]: loss rel. error per step {np.array2string(rel[:, 0], precision=2)}, ce_u "
                 f"{np.array2string(relu, precision=2)}; |n_u - reference| {dn.tolist()} (allowed {[0] * thr_iter + g['meta_near_thr'][thr_iter - 1:steps - 1].tolist()})")
    assert np.max(rel[:2]) < 1e-4, (got, ref)
    assert np.max(rel) < 3e-2 and np.max(relu) < 3e-2, (got, ref)
    for s in range(thr_iter, steps):
        assert dn[s] <= int(g["meta_near_thr"][s - 1]), (s, got[s, 3], g["meta_n_u"][s], g["meta_near_thr"][s - 1])
    if steps == 6:
        sd = eng.model.state_dict()
        for k in [k[6:] for k in g.files if k.startswith("final:")]:
            assert rel_err(sd[k].cpu().numpy().ravel()[:256], g["final:" + k]) < 5e-2, k


def small_run():
    """one fused step (N 3, 16 x 16) and a reference-mode update of two slices with library-drawn dropout, everything seeded"""
    from wsl4mis_amd.dataloaders.dataset_s2l import BaseDataSets_s2l
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import scribble_labels
    rng = np.random.default_rng(9)
    N, S = 3, 16
    ds = BaseDataSets_s2l.from_slices([{"image": rng.random(s, dtype=np.float32), "mask": rng.integers(0, 4, s).astype(np.uint8),
                                        "scribble": np.full(s, 4, np.uint16)} for s in ((21, 17), (16, 30))])
    eng = TrainEngine("unet", 1, 4, loss="s2l", thr_iter=0, thr_conf=0.5)
    load_det(eng.model, 23)
    torch.manual_seed(77)
    w = rng.random((N, S, S, 4)).astype(np.float32)
    eng.step(T(rng.random((N, 1, S, S), dtype=np.float32)), T(scribble_labels(N, S, S, 4, share=0.08)), weight=T(w))
    eng.update_ensemble(ds, patch_size=(S, S))
    return (np.array(list(eng.losses().values())), eng.model.flat_params().clone(), eng.model.flat_grads().clone(), eng.loss_out.clone(),
            [ds.images[i]["weight"].clone() for i in range(len(ds))])


def test_whole_step_is_bit_reproducible(mode):
    """two runs give the same bits in losses, parameters, gradients, BatchNorm buffers' consumers (the stores): every reduction of the
    head is order-fixed, the update has none, and library-drawn dropout is a function of torch's seed.  On the GPU also the
    recipe through the first fused step (two updates in between)."""
    runs = [small_run(), small_run()]
    if mode == "hip":
        for _ in range(2):
            got, _, eng, ds = run_recipe(3)
            runs.append((got.ravel(), eng.model.flat_params().clone(), eng.model.flat_grads().clone(), eng.loss_out.clone(),
                         [ds.images[i]["weight"].clone() for i in range(len(ds))]))
    for a, b in zip(runs[0::2], runs[1::2]):
        assert np.all(np.isfinite(a[0])) and float(a[0][-1]) > 0
        assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3][:5], b[3][:5])
        assert all(torch.equal(x, y) for x, y in zip(a[4], b[4])) and all(float(x.abs().sum()) > 0 for x in a[4])


def test_update_ensemble_eval_mode_leaves_the_model_untouched(mode):
    from wsl4mis_amd.engine import TrainEngine
    g = golden("g13_s2l_curve")
    ds = curve_dataset(g)
    eng = TrainEngine("unet", 1, 4, loss="s2l", s2l_alpha=0.25)
    load_det(eng.model, 31)
    before = (eng.model._param_arena.clone(), eng.model._buf_arena.clone(), eng.model._nbt.clone())
    eng.update_ensemble(ds, mode="eval", patch_size=(32, 32), batch_size=4)
    assert torch.equal(before[0], eng.model._param_arena) and torch.equal(before[1], eng.model._buf_arena)
    assert torch.equal(before[2], eng.model._nbt) and eng.model.training
    for i in range(len(ds)):
        w = ds.images[i]["weight"].cpu().numpy()
        s = w.sum(-1)                        # alpha * softmax + 0.75 * 0: every pixel sums to alpha (scipy's fill pixels to 0)
        assert np.all((np.abs(s - 0.25) < 1e-6) | (s == 0)) and (s == 0).mean() < 0.1, i
    # the eval forward differs from the train-mode one (batch statistics, dropout): another store
    ds2 = curve_dataset(g)
    torch.manual_seed(3)
    eng.update_ensemble(ds2, mode="reference", patch_size=(32, 32))
    assert not torch.equal(before[1], eng.model._buf_arena) and int(eng.model._nbt[0]) == int(before[2][0]) + len(ds2)
    assert rel_err(ds2.images[0]["weight"].cpu().numpy(), ds.images[0]["weight"].cpu().numpy()) > 1e-3
    with pytest.raises(ValueError):
        eng.update_ensemble(ds, mode="fast")
    with pytest.raises(Exception, match="masks"):
        eng.update_ensemble(ds, mode="eval", masks=[None] * len(ds))


def test_s2l_is_single_decoder_only(mode):
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    with pytest.raises(_lib.WslError, match="single-decoder"):
        TrainEngine("unet_cct", 1, 4, loss="s2l")
    eng = TrainEngine("pnet", 1, 4, loss="s2l", thr_iter=0, period_iter=7)
    assert not eng.ensemble_due()
    eng.it = 14
    assert eng.ensemble_due()
