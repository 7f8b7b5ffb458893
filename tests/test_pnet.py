"""PNet2D (ref: networks/pnet.py; net_factory("pnet")) end to end: the default initialisation, and the module's logits, loss, every
parameter gradient, BatchNorm buffers and eval logits against the reference module's (fixtures g12_*, tests/golden/make_golden_pnet.py).
The emulator runs the small non-square configuration (class_num 3, odd dilations), the GPU the factory configuration."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import close, get_backend, golden
from detinit import det_state

TOL = 1e-4


@pytest.fixture
def mode():
    from wsl4mis_amd import _lib, runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    _lib.use_library_for_tests(get_backend("emul").lib)
    yield "emul"
    _lib._reset_for_tests()
    runtime._ws_cache.clear()


def T(a):
    from wsl4mis_amd import runtime
    return torch.from_numpy(np.ascontiguousarray(a)).to(runtime.device())


def test_net_factory_pnet_default_init_is_the_reference_init():
    """torch.manual_seed(s); net_factory("pnet", 1, 4) draws upstream's initial weights bit for bit, in registration order"""
    from wsl4mis_amd import _lib
    from wsl4mis_amd.networks import PNet2D
    from wsl4mis_amd.networks.net_factory import net_factory
    _lib._reset_for_tests()
    _lib.use_library_for_tests(get_backend("emul").lib)      # host-only: the arenas live in CPU tensors
    try:
        g = golden("g12_pnet_init")
        for build in (lambda: net_factory("pnet", 1, 4), lambda: PNet2D(1, 4, 64, [1, 2, 4, 8, 16])):
            torch.manual_seed(1337)
            m = build()
            sd = m.state_dict()
            assert list(sd.keys()) == list(g["keys"]) and len(sd) == 78
            assert [str(tuple(v.shape)) for v in sd.values()] == list(g["shapes"])
            sums = np.array([float(v.double().sum()) for v in sd.values()])
            assert np.array_equal(sums, g["sum"])
            heads = np.stack([np.resize(v.double().cpu().numpy().ravel(), 4) for v in sd.values()])
            assert np.array_equal(heads, g["head"])
            params = list(m.named_parameters())
            assert [k for k, _ in params] == [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
            assert len(params) == 48 and sum(p.numel() for _, p in params) == 486596
            assert m.n_enc_param == 334272 and m.n_param == 486596
        with pytest.raises(NotImplementedError):
            net_factory("pnet", 1, 4, conv_precision="split_f16x3")
    finally:
        _lib._reset_for_tests()


def _against_fixture(name, build):
    g = golden(name)
    model = build()
    sd = model.state_dict()
    vals = det_state({k: tuple(v.shape) for k, v in sd.items()}, 2022)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    model.train()
    model.set_dropout_masks([T(g["io_m1"]), T(g["io_m2"])])
    x, lab = T(g["io_x"]), T(g["io_label"]).long()
    z = model(x)
    assert close(z.detach().cpu().numpy(), g["io_logits"], TOL), "train logits"
    loss = F.cross_entropy(z, lab, ignore_index=4)
    model.zero_grad()
    loss.backward()
    assert abs(float(loss.detach()) - float(g["io_loss"])) <= TOL * abs(float(g["io_loss"]))
    for k, p in model.named_parameters():
        key = [f for f in g.files if f.endswith(f"_grad:{k}")][0]
        ref = g[key]
        got = p.grad.detach().cpu().numpy()
        if k.endswith(("conv1.bias", "conv2.bias")) and k.startswith("block"):   # feeds a BatchNorm: mathematically zero
            assert np.max(np.abs(got - ref)) <= TOL * np.max(np.abs(ref)) + 1e-5, k
        else:
            assert close(got, ref, TOL), k
    for k, b in model.named_buffers():
        ref = g[[f for f in g.files if f.endswith(f"_buf:{k}")][0]]
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(ref), k
        else:
            assert close(b.detach().cpu().numpy(), ref, TOL), k
    model.eval()
    with torch.no_grad():
        ze = model(x)
    assert close(ze.cpu().numpy(), g["io_eval"], TOL), "eval logits"
    # state_dict round trip into a fresh module (reference checkpoints load both ways)
    m2 = build()
    m2.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    m2.eval()
    with torch.no_grad():
        assert torch.equal(m2(x), ze)


def test_pnet_small_matches_reference_emul(mode):
    """host emulator: the small configuration (the GPU tier runs both, test_pnet_factory_matches_reference)"""
    from wsl4mis_amd.networks import PNet2D
    _against_fixture("g12_pnet_small", lambda: PNet2D(1, 3, 16, [1, 2, 3, 5, 8]))


@pytest.mark.gpu
def test_pnet_factory_matches_reference():
    from wsl4mis_amd import _lib
    from wsl4mis_amd.networks.net_factory import net_factory
    _lib._reset_for_tests()
    _against_fixture("g12_pnet32", lambda: net_factory("pnet", 1, 4))
    from wsl4mis_amd.networks import PNet2D
    _against_fixture("g12_pnet_small", lambda: PNet2D(1, 3, 16, [1, 2, 3, 5, 8]))


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["pce", "pce_gatedcrf", "ce_dice", "mean_teacher"])
def test_train_engine_pnet(loss):
    """TrainEngine(net_type="pnet") runs the single-branch compositions; two runs of a whole step from the same state are bit-identical"""
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.synthetic import batch
    _lib._reset_for_tests()
    dev = torch.device("cuda:0")
    x, lab = batch(2, 32, 32, 3, dev)
    res = []
    for _ in range(2):
        torch.manual_seed(7)
        eng = TrainEngine("pnet", 1, 4, loss=loss)
        torch.manual_seed(8)
        eng.step(x, lab)
        torch.cuda.synchronize()
        res.append((eng.losses()["loss"], eng.model.flat_params().clone()))
    assert np.isfinite(res[0][0])
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
