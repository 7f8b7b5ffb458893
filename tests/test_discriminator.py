"""networks/discriminator.py FCDiscriminator: state_dict and default initialisation, eval / train logits, parameter gradients and the
gradient with respect to `map` against the reference's own class (fixture g16_dan_module, tests/golden/make_golden_dan.py) and against the
float64 restatement tests/dan_ref.py, and the autograd contract of the module.

`mode` = emul runs the Python layer against the host-emulation library with CPU tensors; `mode` = hip (gpu mark) is the real thing.
Criterion: conftest.close() / grad_tol at 1e-4 of each tensor's scale.  Element-wise gradient parity is only defined where no
pre-activation sits within fp32 noise of the LeakyReLU kink: every case asserts its margin (MARGIN, against pre-activations of order 1
whose fp32 error is some 1e-6)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dan_ref as R
from conftest import close, get_backend, golden, grad_tol

TOL = 1e-4
MARGIN = 2e-5


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


rand_state = R.rand_state


def reference_pass(sd, map_, feat, masks, pool, target):
    """float64: logits, loss, d loss / d map, parameter gradients, kink margin"""
    sd64 = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    m64 = map_.double().clone().requires_grad_()
    margins = []
    logits = R.forward(sd64, m64, feat.double(), masks, pool, margins)
    loss = F.cross_entropy(logits, target.long())
    loss.backward()
    return logits.detach().numpy(), float(loss.detach()), m64.grad.numpy(), {k: v.grad.numpy() for k, v in sd64.items()}, min(margins)


def module_pass(D, map_, feat, masks, target, train):
    D.train(train)
    if masks is not None:
        D.set_dropout_masks([T(m) for m in masks])
    mt = T(map_).clone().requires_grad_()
    D.zero_grad()
    logits = D(mt, T(feat))
    D.set_dropout_masks(None)
    loss = F.cross_entropy(logits, T(target).long())
    loss.backward()
    return logits.detach().cpu().numpy(), float(loss.detach()), mt.grad.cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in D.named_parameters()}


def check_against(ref, got, what):
    lr, loss_r, dm_r, g_r, margin = ref
    lg, loss_g, dm_g, g_g = got
    assert margin >= MARGIN, (what, "kink margin", margin)
    print(f"{what}: kink margin {margin:.2e}; logits err {np.abs(lg - lr).max():.2e}; dmap err {np.abs(dm_g - dm_r).max():.2e} of {np.abs(dm_r).max():.2e}")
    assert close(lg, lr, TOL), (what, lg, lr)
    assert abs(loss_g - loss_r) <= TOL * abs(loss_r)
    assert close(dm_g, dm_r, TOL), what
    bad = [(k, float(np.abs(g_g[k] - g_r[k]).max()), grad_tol(k, g_r[k], TOL)) for k in g_r if np.abs(g_g[k] - g_r[k]).max() > grad_tol(k, g_r[k], TOL)]
    assert not bad, (what, bad)


def make_masks(rng, N, ndf):
    return [torch.from_numpy(((rng.random((N, c * ndf)) > 0.5) * 2.0).astype(np.float32)) for c in (2, 4)]


# ------------------------------------------------------------------------------------------------ (a) state_dict and initialisation
def test_state_dict_and_default_init(mode):
    """keys, shapes, order and -- under torch.manual_seed -- the initial values of nn.Conv2d / nn.Linear built in the reference's order"""
    from wsl4mis_amd.networks.discriminator import FCDiscriminator
    torch.manual_seed(2022)
    D = FCDiscriminator(4, ndf=8, n_channel=1)
    sd = D.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_shapes(4, 8, 1)
    assert [k for k, _ in D.named_parameters()] == [k for k, _ in R.state_shapes(4, 8, 1)]
    torch.manual_seed(2022)
    mods = [nn.Conv2d(4, 8, 4, 2, 1), nn.Conv2d(1, 8, 4, 2, 1), nn.Conv2d(8, 16, 4, 2, 1), nn.Conv2d(16, 32, 4, 2, 1), nn.Conv2d(32, 64, 4, 2, 1),
            nn.Linear(256, 2)]
    for name, m in zip(R.KEYS, mods):
        assert torch.equal(sd[name + ".weight"].cpu(), m.weight.detach()) and torch.equal(sd[name + ".bias"].cpu(), m.bias.detach()), name
    assert D.cuda() is D and D.flat_params().numel() == sum(v.numel() for v in sd.values())
    g = golden("g16_dan_module")                           # the reference's own class under the same seed
    assert [k for k in sd] == [str(k) for k in g["init_keys"]]
    for k in sd:
        assert np.array_equal(sd[k].cpu().numpy().ravel(), g["init:" + k]), k


# ------------------------------------------------------------------------------------------------ (b) the reference's own class
@pytest.mark.parametrize("tag", ["sq", "wide"])
def test_against_the_reference_class(mode, tag):
    """FCDiscriminator(4, ndf=8) of the reference at N = 2, 224 x 224 and 112 x 448: eval logits, train logits with the recorded Dropout2d
    masks replayed, all parameter gradients, and the gradient with respect to `map` on the stored subset (all four borders 4 pixels deep
    and interior rows of both parities)"""
    from wsl4mis_amd.networks.discriminator import FCDiscriminator
    g = golden("g16_dan_module")
    seed = int(g[f"{tag}_seed"][0])
    map_, feat, target, (H, W) = R.module_inputs(tag, seed)
    assert float(g[f"{tag}_margin"][0]) >= MARGIN
    D = FCDiscriminator(4, ndf=8, n_channel=1)
    D.load_state_dict({k: torch.from_numpy(g["state:" + k]).reshape(v.shape) for k, v in D.state_dict().items()})
    D.eval()
    with torch.no_grad():
        assert close(D(T(map_), T(feat)).cpu().numpy(), g[f"{tag}_logits_eval"], TOL)
    masks = [torch.from_numpy(g[f"{tag}_m2"]), torch.from_numpy(g[f"{tag}_m3"])]
    lg, loss, dm, grads = module_pass(D, map_, feat, masks, target, True)
    assert close(lg, g[f"{tag}_logits_train"], TOL)
    assert abs(loss - float(g[f"{tag}_loss"][0])) <= TOL * abs(float(g[f"{tag}_loss"][0]))
    for k in grads:
        ref = g[f"{tag}_g:{k}"].reshape(grads[k].shape)
        assert np.abs(grads[k] - ref).max() <= grad_tol(k, ref, TOL), k
    rows, cols = R.map_rows(H), R.map_rows(W)
    scale = float(g[f"{tag}_dmap_max"][0])
    ref_r, ref_c = g[f"{tag}_dmap_rows"], g[f"{tag}_dmap_cols"]
    assert np.abs(dm[:, :, rows, :] - ref_r).max() <= TOL * scale + 1e-7
    assert np.abs(dm[:, :, :, cols] - ref_c).max() <= TOL * scale + 1e-7
    assert close(dm[:, :, rows, :], ref_r, TOL) and close(dm[:, :, :, cols], ref_c, TOL)


# ------------------------------------------------------------------------------------------------ (c) full width on the device
@pytest.mark.gpu
def test_full_width_against_float64(hip):
    """ndf = 64, N = 4, 224 x 224: train-mode forward with replayed masks, loss, d / d map and every parameter gradient"""
    from wsl4mis_amd.networks.discriminator import FCDiscriminator
    rng = np.random.default_rng(7)
    N, S = 4, 224
    map_ = torch.softmax(torch.from_numpy(rng.standard_normal((N, 4, S, S)).astype(np.float32)) * 2, 1)
    feat = torch.from_numpy(rng.random((N, 1, S, S)).astype(np.float32))
    target = torch.tensor([1, 1, 0, 0])
    sd = rand_state(11, 4, 64, 1, calibrate=(map_, feat))
    masks = make_masks(rng, N, 64)
    D = FCDiscriminator(4, ndf=64, n_channel=1)
    D.load_state_dict(sd)
    check_against(reference_pass(sd, map_, feat, masks, 7, target), module_pass(D, map_, feat, masks, target, True), "ndf64")


# ------------------------------------------------------------------------------------------------ (e) pool = 1 at 32 x 32
@pytest.mark.parametrize("train", [False, True])
def test_pool1_small_against_float64(mode, train):
    from wsl4mis_amd.networks.discriminator import FCDiscriminator
    rng = np.random.default_rng(3)
    N, S, ndf = 3, 32, 8
    map_ = torch.softmax(torch.from_numpy(rng.standard_normal((N, 4, S, S)).astype(np.float32)) * 2, 1)
    feat = torch.from_numpy(rng.random((N, 1, S, S)).astype(np.float32))
    target = torch.tensor([1, 0, 1])
    sd = rand_state(5, 4, ndf, 1)
    masks = make_masks(rng, N, ndf) if train else None
    D = FCDiscriminator(4, ndf=ndf, n_channel=1, pool=1)
    D.load_state_dict(sd)
    check_against(reference_pass(sd, map_, feat, masks, 1, target), module_pass(D, map_, feat, masks, target, train), f"pool1 train={train}")


# ------------------------------------------------------------------------------------------------ (d) autograd contract
def test_autograd_contract(mode):
    from wsl4mis_amd import _lib
    from wsl4mis_amd.networks.discriminator import FCDiscriminator
    torch.manual_seed(1)
    D = FCDiscriminator(4, ndf=8, n_channel=1, pool=1)
    map_ = T(torch.softmax(torch.randn(2, 4, 32, 32), 1)).requires_grad_()
    feat = T(torch.rand(2, 1, 32, 32))
    # eval mode still differentiates into the map (the generator update runs the adversary in eval mode)
    D.eval()
    out = D(map_, feat)
    assert out.requires_grad and tuple(out.shape) == (2, 2)
    out.sum().backward()
    assert map_.grad is not None and tuple(map_.grad.shape) == tuple(map_.shape) and float(map_.grad.abs().max()) > 0
    assert all(p.grad is not None for p in D.parameters())
    # train() / eval() switch the dropout: eval is deterministic, train with drawn masks differs from it
    with torch.no_grad():
        e1, e2 = D(map_, feat), D(map_, feat)
        D.train()
        t1 = D(map_, feat)
    assert torch.equal(e1, e2) and not torch.equal(e1, t1)
    assert set(np.unique(D._last_masks[0].cpu().numpy())) <= {0.0, 2.0}
    # feature.requires_grad is refused
    with pytest.raises(NotImplementedError):
        D(map_, feat.clone().requires_grad_())
    # a backward after a newer forward of the same module is refused
    a = D(map_, feat)
    D(map_, feat)
    with pytest.raises(_lib.WslError, match="newer forward"):
        a.sum().backward()
    # a pooled map without 4 positions is refused (pool = 1 at 48 x 48 gives 3 x 3; the default pool = 7 at 32 x 32 gives 0 x 0)
    with pytest.raises(_lib.WslError, match="4 positions"):
        D(T(torch.rand(1, 4, 48, 48)), T(torch.rand(1, 1, 48, 48)))
    with pytest.raises(_lib.WslError, match="4 positions"):
        FCDiscriminator(4, ndf=8)(T(torch.rand(1, 4, 32, 32)), T(torch.rand(1, 1, 32, 32)))
    # parameters frozen: the backward computes the gradient to the map only
    for p in D.parameters():
        p.requires_grad_(False)
    m2 = map_.detach().clone().requires_grad_()
    D(m2, feat).sum().backward()
    assert m2.grad is not None
