"""Golden vectors of the inter/intra-class variance recipe (fixtures g14_interintra*), from the reference's own code
(code/train_weakly_supervised_pCE_Inter&Intra_Class_2D.py).  Runs only where the reference checkout exists, like make_golden_s2l.py (it
reuses save / load_det / DropoutRecorder of make_golden.py); the tests read the .npz files it leaves.

The trainer does not import here (tensorboardX, torchvision, an argparse at module level), so its two functions
intra_class_variance / inter_class_variance are lifted with ast at generation time; the loop body (lines 107-127) is restated with the
same torch calls in the same order, on the reference's own UNet.  No reference text is stored.

  python tests/golden/make_golden_interintra.py [ops] [curve]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import CrossEntropyLoss

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import DropoutRecorder, lift, load_det, save, scribble_labels  # noqa: E402
from networks.unet import UNet  # noqa: E402  (make_golden put the reference on sys.path)

TRAINER = "train_weakly_supervised_pCE_Inter&Intra_Class_2D.py"
intra_class_variance = lift(TRAINER, "intra_class_variance", {"torch": torch})
inter_class_variance = lift(TRAINER, "inter_class_variance", {"torch": torch})


def gen_ops():
    """two (p, img) pairs at C = 4; inter, intra and d(inter - intra)/dp from the reference's functions in fp32 and in fp64"""
    out = {}
    for tag, (N, H, W), seed in (("a", (2, 24, 20), 1), ("b", (3, 16, 16), 2)):
        g = torch.Generator().manual_seed(140 + seed)
        z = torch.randn((N, 4, H, W), generator=g) * 2 + torch.arange(4.0).view(1, 4, 1, 1)
        p32 = torch.softmax(z, 1)
        img = torch.rand((N, 1, H, W), generator=g)
        out.update({f"{tag}_p": p32.numpy(), f"{tag}_img": img.numpy()})
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            p = p32.detach().clone().to(dt).requires_grad_()
            inter, intra = inter_class_variance(p, img.to(dt)), intra_class_variance(p, img.to(dt))
            (inter - intra).backward()
            out[f"{tag}_{name}_values"] = np.array([inter.item(), intra.item()], dtype=np.float64)
            out[f"{tag}_{name}_dp"] = p.grad.numpy().copy()
        print("   ", tag, out[f"{tag}_f32_values"], out[f"{tag}_f64_values"])
    save("g14_interintra", **out)


class DropoutReplay:
    """F.dropout that takes its keep masks from a recorded list (the fp64 run repeats the fp32 run's draws)"""

    def __init__(self, masks):
        self.masks = list(masks)

    def __enter__(self):
        self._d = F.dropout
        me = self

        def dropout(x, p=0.5, training=True, inplace=False):
            if not training or p == 0.0:
                return x
            keep = torch.from_numpy(me.masks.pop(0)).to(x.dtype)
            return x * (keep * (np.float32(1.0 / (1.0 - p)) if x.dtype == torch.float32 else 1.0 / (1.0 - p)))

        F.dropout = torch.nn.functional.dropout = dropout
        return self

    def __exit__(self, *a):
        F.dropout = torch.nn.functional.dropout = self._d


def gen_curve(torch_seed=0):
    """UNet(1, 4), batches of 4 x 32 x 32, six steps of the trainer's loop body (SGD 0.01 / 0.9 / 1e-4 + poly LR) with the constant weight
    0.1 (--consistency 0.1 --consistency_rampup 0: the default ramp starts at 0.1 e^-5, which would leave the regulariser invisible in
    six steps), every dropout mask recorded.  Run in fp32 and, on the same inputs, initial values and masks, in fp64."""
    torch.manual_seed(torch_seed)
    N, P, steps, w = 4, 32, 6, 0.1
    gen = torch.Generator().manual_seed(14)
    xs = torch.rand(steps, N, 1, P, P, generator=gen)
    labs = np.stack([scribble_labels(N, P, P, seed=140 + s) for s in range(steps)])
    out = {"meta_hyper": np.array([w, 0.0]), "in_xs": xs.numpy(), "in_labels": labs}
    masks = []
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        model = UNet(1, 4)
        load_det(model, 41)
        model = model.to(dt).train()
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        ce_loss = CrossEntropyLoss(ignore_index=4)
        losses, iter_num = [], 0
        for it in range(steps):
            volume_batch, label_batch = xs[it].to(dt), torch.from_numpy(labs[it])
            if name == "f32":
                with DropoutRecorder() as rec:
                    outputs = model(volume_batch)
                masks.append([m for m, _ in rec.elem])
                for l, m in enumerate(masks[-1]):
                    out[f"s{it}_em{l}"] = np.packbits(m.ravel())
            else:
                with DropoutReplay(masks[it]):
                    outputs = model(volume_batch)
            outputs_soft = torch.softmax(outputs, dim=1)
            inter, intra = inter_class_variance(outputs_soft, volume_batch), intra_class_variance(outputs_soft, volume_batch)
            consistency_loss = inter - intra
            loss_ce = ce_loss(outputs, label_batch[:].long())
            loss = loss_ce + w * consistency_loss
            opt.zero_grad()
            loss.backward()
            opt.step()
            lr_ = 0.01 * (1.0 - iter_num / 30000) ** 0.9
            for pg in opt.param_groups:
                pg["lr"] = lr_
            iter_num += 1
            losses.append([loss.item(), loss_ce.item(), inter.item(), intra.item()])
        out[f"meta_losses_{name}"] = np.array(losses, dtype=np.float64)
        sd = model.state_dict()
        for k in ("encoder.in_conv.conv_conv.0.weight", "decoder.out_conv.weight", "encoder.down4.maxpool_conv.1.conv_conv.5.running_var"):
            out[f"final_{name}:{k}"] = sd[k].numpy().ravel()[:256].copy()
        print("   ", name, np.array(losses))
    save("g14_interintra_curve", **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["ops", "curve"]:
        print(w)
        {"ops": gen_ops, "curve": gen_curve}[w]()
