"""Golden vectors of PNet2D (fixtures g12_*), from the reference's own module (code/networks/pnet.py).  Runs only where the reference
checkout exists, like make_golden.py (whose save / load_det it reuses); the tests read the .npz files it leaves.

  python tests/golden/make_golden_pnet.py [init] [small] [net32] [curve]
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, load_det, save  # noqa: E402

sys.path.insert(0, REF)
from networks.pnet import PNet2D  # noqa: E402
from utils.gate_crf_loss import ModelLossSemsegGatedCRF  # noqa: E402

DET_SEED = 2022


class _Mult(nn.Module):
    """stands in for one nn.Dropout2d of OutPutBlock with a recorded channel multiplier (0 or 1/(1-p)) in training mode"""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask[:, :, None, None] if self.training else x


def _tag(key):
    """the fixture's case tag of a state_dict key (save() splits files by the prefix before the first '_'): one per block"""
    head = key.split(".")[0]
    return head if head.startswith("block") else "head"


def gen_init():
    torch.manual_seed(1337)
    sd = PNet2D(1, 4, 64, [1, 2, 4, 8, 16]).state_dict()
    save("g12_pnet_init", keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]),
         sum=np.array([float(v.double().sum()) for v in sd.values()]),
         head=np.stack([np.resize(v.double().numpy().ravel(), 4) for v in sd.values()]))


def gen_case(name, n_class, F_, ratios, N, H, W, seed):
    net = PNet2D(1, n_class, F_, ratios)
    load_det(net, DET_SEED)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, 1, H, W), generator=g)
    lab = torch.randint(0, n_class, (N, H, W), generator=g)
    lab[torch.rand((N, H, W), generator=g) < 0.7] = 4        # scribbles: most pixels unlabelled (ignore_index 4)
    m1 = ((torch.rand((N, 2 * F_), generator=g) >= 0.3).float() / 0.7).float()
    m2 = ((torch.rand((N, F_), generator=g) >= 0.3).float() / 0.7).float()
    net.out.drop1, net.out.drop2 = _Mult(m1), _Mult(m2)
    net.train()
    z = net(x)
    loss = F.cross_entropy(z, lab, ignore_index=4)
    loss.backward()
    out = {"io_x": x.numpy(), "io_label": lab.numpy().astype(np.uint8), "io_m1": m1.numpy(), "io_m2": m2.numpy(),
           "io_logits": z.detach().numpy(), "io_loss": np.array(float(loss))}
    for k, p in net.named_parameters():
        out[f"{_tag(k)}_grad:{k}"] = p.grad.numpy().copy()
    for k, b in net.named_buffers():
        out[f"{_tag(k)}_buf:{k}"] = b.numpy().copy()
    net.eval()
    with torch.no_grad():
        out["io_eval"] = net(x).numpy()
    save(name, **out)


def gen_curve():
    """5 steps of pCE + 0.1 * GatedCRF(softmax, r = 5) (train_weakly_supervised_pCE_GatedCRFLoss_2D.py) on the factory PNet2D with torch
    SGD (lr 0.01, momentum 0.9, wd 1e-4) and poly LR, N = 2, 32 x 32, recorded Dropout2d multipliers: loss terms per step, final
    per-tensor parameter sums"""
    N, H, W, steps, F_ = 2, 32, 32, 5, 64
    net = PNet2D(1, 4, F_, [1, 2, 4, 8, 16])
    load_det(net, DET_SEED)
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    crf = ModelLossSemsegGatedCRF()
    g = torch.Generator().manual_seed(55)
    out, losses = {}, []
    for it in range(steps):
        x = torch.rand((N, 1, H, W), generator=g)
        lab = torch.randint(0, 4, (N, H, W), generator=g)
        lab[torch.rand((N, H, W), generator=g) < 0.7] = 4
        m1 = ((torch.rand((N, 2 * F_), generator=g) >= 0.3).float() / 0.7).float()
        m2 = ((torch.rand((N, F_), generator=g) >= 0.3).float() / 0.7).float()
        net.out.drop1, net.out.drop2 = _Mult(m1), _Mult(m2)
        z = net(x)
        loss_ce = F.cross_entropy(z, lab, ignore_index=4)
        loss_crf = crf(torch.softmax(z, 1), [{"weight": 1, "xy": 6, "rgb": 0.1}], 5, x, H, W)["loss"]
        loss = loss_ce + 0.1 * loss_crf
        opt.zero_grad()
        loss.backward()
        opt.step()
        for pg in opt.param_groups:
            pg["lr"] = 0.01 * (1.0 - it / 60000) ** 0.9
        losses.append([loss.item(), loss_ce.item(), loss_crf.item()])
        out.update({f"s{it}_x": x.numpy(), f"s{it}_label": lab.numpy().astype(np.uint8), f"s{it}_m1": m1.numpy(),
                    f"s{it}_m2": m2.numpy()})
    sd = [(k, p.detach().double()) for k, p in net.named_parameters()]
    out.update(losses=np.array(losses), keys=np.array([k for k, _ in sd]), psum=np.array([float(p.sum()) for _, p in sd]),
               pabs=np.array([float(p.abs().sum()) for _, p in sd]))
    save("g12_pnet_curve", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["init", "small", "net32", "curve"]
    for w in which:
        print(w)
        if w == "init":
            gen_init()
        elif w == "small":
            gen_case("g12_pnet_small", 3, 16, [1, 2, 3, 5, 8], 2, 24, 40, 12)
        elif w == "net32":
            gen_case("g12_pnet32", 4, 64, [1, 2, 4, 8, 16], 2, 32, 32, 32)
        elif w == "curve":
            gen_curve()
