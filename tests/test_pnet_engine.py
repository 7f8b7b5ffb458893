"""PNet2D through TrainEngine(net_type="pnet") and at full resolution (GPU tier):

  * one engine step equals the module path -- PNet2D -> softmax -> the loss pieces -> autograd -> torch.optim.SGD -- for pce,
    pce_gatedcrf, ce_dice and mean_teacher (loss terms, every parameter gradient, parameters after the step);
  * five steps of pCE + GatedCRF follow the reference module's curve (fixture g12_pnet_curve, tests/golden/make_golden_pnet.py);
  * force_dp=True in a 1-rank RCCL group gives the parameters of the plain route bit for bit;
  * the factory network at N = 2, 256 x 256: every parameter gradient against an fp64 torch-CPU restatement of PNet written here,
    evaluated on the LeakyReLU decisions the HIP forward took (netutil.DecisionReplay)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import close, golden, mixed_err, rel_err, summary_line
from detinit import det_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
FILT, RATIOS = 64, (1, 2, 4, 8, 16)


def _dev():
    return torch.device("cuda:0")


def _det(model, seed):
    vals = det_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})


def _grad_ok(k, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if k.startswith("block") and k.endswith(("conv1.bias", "conv2.bias")):    # feeds a BatchNorm: mathematically zero
        return float(np.max(np.abs(got - ref))) <= TOL * float(np.max(np.abs(ref))) + 1e-5
    return close(got, ref, TOL)


def _masks(N, gen):
    m1 = ((torch.rand((N, 2 * FILT), generator=gen) >= 0.3).float() / 0.7).float()
    m2 = ((torch.rand((N, FILT), generator=gen) >= 0.3).float() / 0.7).float()
    return [m1.to(_dev()), m2.to(_dev())]


@pytest.mark.parametrize("kind", ["pce", "pce_gatedcrf", "ce_dice", "mean_teacher"])
def test_engine_step_matches_module_path(kind):
    from oracle import torch_ref as R
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    from wsl4mis_amd.networks.net_factory import net_factory
    from wsl4mis_amd.synthetic import scribble_labels
    _lib._reset_for_tests()
    N, S = 2, 32
    gen = torch.Generator().manual_seed(17)
    x = torch.rand((N, 1, S, S), generator=gen).to(_dev())
    if kind == "ce_dice":                                       # dense labels (fully supervised / random-walker pseudo labels)
        lab = torch.randint(0, 4, (N, S, S), generator=gen).to(torch.uint8)
    else:
        lab = torch.from_numpy(scribble_labels(N, S, S, 4, share=0.08))
    lab = lab.to(_dev())
    ms, mt = _masks(N, gen), _masks(N, gen)
    noise = torch.clamp(torch.randn((N, 1, S, S), generator=gen) * 0.1, -0.2, 0.2).to(_dev())
    # ---- engine
    eng = TrainEngine("pnet", 1, 4, loss=kind)
    _det(eng.model, 31)
    eng.model.set_dropout_masks(ms)
    if eng.teacher is not None:
        eng.teacher.load_state_dict(eng.model.state_dict())
        eng.teacher.set_dropout_masks(mt)
    eng.forward_backward(x, lab, 0.5, noise if kind == "mean_teacher" else None)
    o = eng.losses()
    g_eng = eng.model.flat_grads().clone()
    eng.optimizer_step()
    # ---- module path
    model = net_factory("pnet", 1, 4)
    _det(model, 31)
    model.train()
    model.set_dropout_masks(ms)
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    z = model(x)
    s = torch.softmax(z, 1)
    ce = R.ce_ignore(z, lab)
    if kind == "pce":
        loss, ref = ce, [ce]
        got = [o["loss"]]
    elif kind == "pce_gatedcrf":
        crf = R.gatedcrf(s.cpu(), x.cpu(), 5)[0].to(_dev())       # (the oracle builds its position features on the host)
        loss, ref, got = ce + 0.1 * crf, [ce, crf], [o["ce"], o["crf"]]
    elif kind == "ce_dice":
        dice = R.dice(s, lab.long().unsqueeze(1))
        loss, ref, got = 0.5 * (ce + dice), [ce, dice], [o["ce"], o["dice"]]
    else:
        teacher = net_factory("pnet", 1, 4)
        teacher.load_state_dict(model.state_dict())
        teacher.train()
        teacher.set_dropout_masks(mt)
        with torch.no_grad():
            zt = teacher(x + noise)
        loss, ce, tv, cons = R.mean_teacher_loss(z, zt, lab, 0)
        ref, got = [ce, tv, cons], [o["ce"], o["tv"], o["cons"]]
    opt.zero_grad()
    loss.backward()
    assert rel_err(got, [float(t.detach()) for t in ref]) < TOL and abs(o["loss"] - float(loss.detach())) <= TOL * abs(float(loss.detach())), (kind, o)
    off = 0
    for k, p in model.named_parameters():
        n = p.numel()
        assert _grad_ok(k, g_eng[off:off + n].view(p.shape).cpu().numpy(), p.grad.cpu().numpy()), (kind, k)
        off += n
    opt.step()
    got_p = eng.model.state_dict()
    for k, p in model.named_parameters():
        assert rel_err(got_p[k].cpu(), p.detach().cpu()) < 1e-6, (kind, k)
    if kind == "mean_teacher":       # update_ema_variables at iteration 0: alpha = min(1 - 1/1, 0.99) = 0, the teacher takes the student
        got_t = eng.teacher.state_dict()
        for k, p in model.named_parameters():
            assert rel_err(got_t[k].cpu(), p.detach().cpu()) < 1e-6, (kind, k)


def test_engine_gatedcrf_curve_against_reference():
    """5 steps of pCE + 0.1 GatedCRF (r = 5) with SGD + poly LR against the reference module's run (g12_pnet_curve), at the
    g9_crf_curve tolerance: the first two steps to 1e-4, the tail to 3e-2"""
    from wsl4mis_amd import _lib
    from wsl4mis_amd.engine import TrainEngine
    _lib._reset_for_tests()
    g = golden("g12_pnet_curve")
    eng = TrainEngine("pnet", 1, 4, base_lr=0.01, max_iterations=60000, loss="pce_gatedcrf", crf_radius=5)
    _det(eng.model, 2022)
    got = []
    for it in range(g["losses"].shape[0]):
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())  # noqa: E731
        eng.model.set_dropout_masks([T(g[f"s{it}_m1"]), T(g[f"s{it}_m2"])])
        eng.step(T(g[f"s{it}_x"]), T(g[f"s{it}_label"]), 0.5)
        o = eng.losses()
        got.append([o["loss"], o["ce"], o["crf"]])
    got, ref = np.array(got), g["losses"]
    rel = np.abs(got - ref) / np.abs(ref)
    assert np.max(rel[:2]) < 1e-4, (got, ref)
    assert np.max(rel) < 3e-2, (got, ref)
    sd = dict(eng.model.named_parameters())
    for k, s, a in zip(g["keys"], g["psum"], g["pabs"]):
        assert abs(float(sd[str(k)].detach().double().sum()) - s) <= 1e-4 * a + 1e-7, k


def test_single_rank_rccl_group_dp_route_equals_plain_route():
    """force_dp=True in a 1-rank RCCL group: split backward (catblock + out bucket, then the blocks' bucket) and the all-reduce on
    the side stream -- bit-identical to the plain step"""
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    code = r"""
import sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from wsl4mis_amd.engine import TrainEngine
from wsl4mis_amd.synthetic import batch
outs = []
for force in (False, True):
    torch.manual_seed(5)
    eng = TrainEngine("pnet", 1, 4, loss="pce_gatedcrf", force_dp=force)
    assert eng.dp == force and (eng.comm is not None) == force
    x, lab = batch(2, 64, 64, 11, torch.device("cuda", 0))
    for _ in range(3):
        eng.step(x, lab)
    outs.append((eng.model.flat_params().clone(), eng.losses()))
assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], (outs[0][1], outs[1][1])
dist.destroy_process_group()
print("PNET_DP_ROUTE_OK")
""" % (ROOT, port)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "PNET_DP_ROUTE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- full resolution, fp64 restatement
def _pnet_fp64(sd, x, m1, m2, ratios=RATIOS):
    """PNet2D in functional form (DeepIGeoS P-Net as the reference builds it): five blocks of two dilated 3x3 conv + BatchNorm
    (batch statistics) + LeakyReLU, concat, two 1x1 + LeakyReLU, Dropout2d multipliers, two 1x1.  F.leaky_relu is called once per
    activation site, in forward order, so DecisionReplay can substitute the decisions of another implementation."""
    feats, h = [], x
    for k, d in enumerate(ratios, start=1):
        p = f"block{k}."
        for c, b in (("conv1", "in1"), ("conv2", "in2")):
            h = F.conv2d(h, sd[p + c + ".weight"], sd[p + c + ".bias"], padding=d, dilation=d)
            h = F.batch_norm(h, None, None, sd[p + b + ".weight"], sd[p + b + ".bias"], training=True, eps=1e-5)
            h = F.leaky_relu(h, 0.01)
        feats.append(h)
    h = torch.cat(feats, 1)
    h = F.leaky_relu(F.conv2d(h, sd["catblock.conv1.weight"], sd["catblock.conv1.bias"]), 0.01)
    h = F.leaky_relu(F.conv2d(h, sd["catblock.conv2.weight"], sd["catblock.conv2.bias"]), 0.01)
    h = h * m1[:, :, None, None]
    h = F.leaky_relu(F.conv2d(h, sd["out.conv1.weight"], sd["out.conv1.bias"]), 0.01)
    h = h * m2[:, :, None, None]
    return F.conv2d(h, sd["out.conv2.weight"], sd["out.conv2.bias"])


def _hip_decisions(model, N, H, W):
    """The 13 LeakyReLU decisions of the last training forward, read from the module's workspace in the order of
    wsl_pnet.hip's plan (raw conv outputs and BatchNorm coefficients are kept there for the backward): the sign of
    y * scale + shift per BatchNorm site (the loader's fmaf: its sign is that of the exact value, which fp64 holds), then
    catblock.conv1, catblock.conv2, out.conv1 outputs."""
    from wsl4mis_amd import runtime
    ws = runtime._ws_cache[(str(runtime.device()), ("pnet", id(model), "train"))].view(torch.float32)
    F_ = FILT
    u = N * F_ * H * W
    r64 = lambda n: (n + 63) // 64 * 64  # noqa: E731
    cat, y1 = 0, [(5 + k) * u for k in range(5)]
    st1 = [10 * u + k * r64(4 * F_) for k in range(5)]
    st2 = 10 * u + 5 * r64(4 * F_)
    zc1 = st2 + r64(20 * F_)
    zc2, zo1 = zc1 + 5 * u, zc1 + 7 * u
    t = lambda off, C: ws[off:off + N * C * H * W].view(N, C, H, W)  # noqa: E731
    catt = t(cat, 5 * F_)
    signs = []
    for k in range(5):
        sc, sh = ws[st1[k] + 2 * F_:st1[k] + 3 * F_], ws[st1[k] + 3 * F_:st1[k] + 4 * F_]
        signs.append((t(y1[k], F_).double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None] > 0).cpu())
        sc, sh = ws[st2 + 10 * F_ + k * F_:st2 + 11 * F_ + k * F_], ws[st2 + 15 * F_ + k * F_:st2 + 16 * F_ + k * F_]
        y2 = catt[:, k * F_:(k + 1) * F_]
        signs.append((y2.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None] > 0).cpu())
    signs += [(t(zc1, 5 * F_) > 0).cpu(), (t(zc2, 2 * F_) > 0).cpu(), (t(zo1, F_) > 0).cpu()]
    return signs


def test_fullres_gradients_against_fp64_restatement():
    from netutil import DecisionReplay
    from wsl4mis_amd import _lib
    from wsl4mis_amd.networks.net_factory import net_factory
    from wsl4mis_amd.synthetic import scribble_labels
    _lib._reset_for_tests()
    N, S = 2, 256
    gen = torch.Generator().manual_seed(256)
    x = torch.rand((N, 1, S, S), generator=gen)
    lab = torch.from_numpy(scribble_labels(N, S, S, 4, share=0.08)).long()
    m1, m2 = [m.cpu() for m in _masks(N, gen)]
    model = net_factory("pnet", 1, 4)
    _det(model, 2022)
    model.train()
    model.set_dropout_masks([m1.to(_dev()), m2.to(_dev())])
    z = model(x.to(_dev()))
    loss = F.cross_entropy(z, lab.to(_dev()), ignore_index=4)
    model.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    signs = _hip_decisions(model, N, S, S)
    hip_grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    # ---- fp64 restatement on the host, on the HIP forward's decisions
    vals = det_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2022)
    sd = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for k, v in vals.items() if not k.endswith(
        ("running_mean", "running_var", "num_batches_tracked"))}
    with DecisionReplay(signs=signs):
        z64 = _pnet_fp64(sd, x.double(), m1.double(), m2.double())
    with DecisionReplay(record=True) as free:        # how many decisions a free-running fp64 forward takes differently
        with torch.no_grad():
            _pnet_fp64({k: v.detach() for k, v in sd.items()}, x.double(), m1.double(), m2.double())
    flips = int(sum(int((a != b).sum()) for a, b in zip(free.signs, signs)))
    assert close(z.detach().cpu().numpy(), z64.detach().numpy(), TOL), "logits"
    loss64 = F.cross_entropy(z64, lab, ignore_index=4)
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) <= TOL * abs(float(loss64.detach()))
    worst, bad = (0.0, ""), []
    for k, t in sd.items():
        ref = t.grad.numpy()
        if not _grad_ok(k, hip_grads[k], ref):
            bad.append((k, rel_err(hip_grads[k], ref), mixed_err(hip_grads[k], ref)))
        elif not (k.startswith("block") and k.endswith(("conv1.bias", "conv2.bias"))):
            worst = max(worst, (mixed_err(hip_grads[k], ref), k))
    summary_line(f"PNet2D full resolution (N = {N}, {S} x {S}), decisions replayed: all {len(sd)} gradient tensors vs fp64, worst "
                 f"{worst[0]:.3f} of the element-wise 1e-4 budget ({worst[1]}); free-running fp64 decisions differing: {flips}")
    assert not bad, bad
