"""Golden vectors of the semi-supervised recipes (fixtures g15_semi_mt / g15_semi_uamt / g15_semi_entmin), from the reference's own code:
its networks/unet.py, utils/losses.py (DiceLoss, softmax_mse_loss, entropy_loss) and utils/ramps.py.  Runs only where the reference
checkout exists, like make_golden_interintra.py (it reuses save / load_det / DropoutRecorder / DropoutReplay); the tests read the .npz
files it leaves.

The trainers do not import here (tensorboardX, torchvision, an argparse at module level), so the loop bodies of
train_mean_teacher_2D.py:141-180, train_uncertainty_aware_mean_teacher_2D.py:141-199 and train_entropy_minimization_2D.py:125-152 are
restated line by line with the same calls in the same order, on the reference's own UNet, losses and ramps.  No reference text is stored.
As in the scripts, update_ema_variables is never called: the teacher keeps its initial weights (TrainEngine(teacher_update="frozen")).
--consistency 0.1 --consistency_rampup 0 (ramps.sigmoid_rampup(., 0) = 1: the constant weight; the default ramp starts at 0.1 e^-5, which
would leave the unsupervised term invisible in a handful of steps).

Each recipe runs in float32 and, on the same inputs, initial values, noises and dropout masks, in float64.  The generator asserts that the
inputs are usable and moves to the next teacher initialisation if not: the reference's own fp32-vs-fp64 spread stays below a third of each
bound of the test (1e-4 on the first two steps, 3e-2 on the tail, 5e-2 on the final tensors), and for semi_uamt between 10 % and 90 % of
the pixels are certain at every step with no pixel's uncertainty within 1e-3 (relative) of the threshold -- a mask flip is a discrete change
no tolerance covers.

  python tests/golden/make_golden_semi.py [semi_mt] [semi_uamt] [semi_entmin]
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
from make_golden import DropoutRecorder, load_det, save  # noqa: E402
from make_golden_interintra import DropoutReplay  # noqa: E402
from networks.unet import UNet  # noqa: E402  (make_golden put the reference on sys.path)
from utils import losses, ramps  # noqa: E402

STEPS = {"semi_mt": 6, "semi_uamt": 4, "semi_entmin": 4}
N, P, NUM_CLASSES, MAX_IT, BASE_LR = 2, 32, 4, 30000, 0.01
CONSISTENCY, RAMPUP = 0.1, 0.0
STUDENT_SEED, SHARP = 51, 60.0          # SHARP: the semi_uamt teacher's out_conv scaled, so that the uncertainty threshold splits the pixels
FINAL = ("encoder.in_conv.conv_conv.0.weight", "decoder.out_conv.weight", "encoder.down4.maxpool_conv.1.conv_conv.5.running_var")
BOUNDS = (1e-4, 3e-2, 5e-2)


def get_current_consistency_weight(epoch):
    return CONSISTENCY * ramps.sigmoid_rampup(epoch, RAMPUP)


def inputs(kind):
    steps = STEPS[kind]
    gen = torch.Generator().manual_seed(150 + len(kind))
    d = {"xl": torch.rand(steps, N, 1, P, P, generator=gen), "xu": torch.rand(steps, N, 1, P, P, generator=gen),
         "lab": torch.randint(0, NUM_CLASSES, (steps, N, P, P), generator=gen).to(torch.uint8)}
    if kind != "semi_entmin":
        d["noise0"] = torch.clamp(torch.randn(steps, N, 1, P, P, generator=gen) * 0.1, -0.2, 0.2)
    if kind == "semi_uamt":
        d["noiseT"] = torch.clamp(torch.randn(steps, 4, 2 * N, 1, P, P, generator=gen) * 0.1, -0.2, 0.2)
    return d


def forward(model, x, name, rec_masks, key):
    """one forward of the reference's UNet: the fp32 run draws and records its dropout masks, the fp64 run replays them"""
    if name == "f32":
        with DropoutRecorder() as rec:
            out = model(x)
        rec_masks[key] = [m for m, _ in rec.elem]
    else:
        with DropoutReplay(rec_masks[key]):
            out = model(x)
    return out


def run(kind, d, teacher_seed, rec_masks, name, dt):
    steps = STEPS[kind]
    model = UNet(1, NUM_CLASSES)
    load_det(model, STUDENT_SEED)
    model = model.to(dt).train()
    ema_model = None
    if kind != "semi_entmin":
        ema_model = UNet(1, NUM_CLASSES)
        load_det(ema_model, teacher_seed)
        if kind == "semi_uamt":
            with torch.no_grad():
                ema_model.decoder.out_conv.weight.mul_(SHARP)
        for param in ema_model.parameters():
            param.detach_()
        ema_model = ema_model.to(dt).train()                 # the scripts never put it in eval()
    optimizer = torch.optim.SGD(model.parameters(), lr=BASE_LR, momentum=0.9, weight_decay=0.0001)
    ce_loss = CrossEntropyLoss()
    dice_loss = losses.DiceLoss(NUM_CLASSES)
    rows, certain, margin, iter_num = [], [], [], 0
    for it in range(steps):
        volume_batch, label_batch = d["xl"][it].to(dt), d["lab"][it]
        unlabeled_volume_batch = d["xu"][it].to(dt)
        if ema_model is not None:
            ema_inputs = unlabeled_volume_batch + d["noise0"][it].to(dt)
        outputs = forward(model, volume_batch, name, rec_masks, (it, "l"))
        outputs_soft = torch.softmax(outputs, dim=1)
        outputs_unlabeled = forward(model, unlabeled_volume_batch, name, rec_masks, (it, "u"))
        outputs_unlabeled_soft = torch.softmax(outputs_unlabeled, dim=1)
        extra = 0.0
        if ema_model is not None:
            with torch.no_grad():
                ema_output = forward(ema_model, ema_inputs, name, rec_masks, (it, "t0"))
                ema_output_soft = torch.softmax(ema_output, dim=1)
        if kind == "semi_uamt":
            T = 8
            _, _, w, h = unlabeled_volume_batch.shape
            volume_batch_r = unlabeled_volume_batch.repeat(2, 1, 1, 1)
            stride = volume_batch_r.shape[0] // 2
            preds = torch.zeros([stride * T, NUM_CLASSES, w, h], dtype=dt)
            for i in range(T // 2):
                ema_inputs = volume_batch_r + d["noiseT"][it, i].to(dt)
                with torch.no_grad():
                    preds[2 * stride * i:2 * stride * (i + 1)] = forward(ema_model, ema_inputs, name, rec_masks, (it, f"t{i + 1}"))
            preds = F.softmax(preds, dim=1)
            preds = preds.reshape(T, stride, NUM_CLASSES, w, h)
            preds = torch.mean(preds, dim=0)
            uncertainty = -1.0 * torch.sum(preds * torch.log(preds + 1e-6), dim=1, keepdim=True)
        loss_ce = ce_loss(outputs, label_batch[:].long())
        loss_dice = dice_loss(outputs_soft, label_batch.unsqueeze(1))
        supervised_loss = 0.5 * (loss_dice + loss_ce)
        consistency_weight = get_current_consistency_weight(iter_num // 300)
        if kind == "semi_mt":
            consistency_loss = torch.mean((outputs_unlabeled_soft - ema_output_soft) ** 2)
        elif kind == "semi_uamt":
            consistency_dist = losses.softmax_mse_loss(outputs_unlabeled, ema_output)
            threshold = (0.75 + 0.25 * ramps.sigmoid_rampup(iter_num, MAX_IT)) * np.log(2)
            mask = (uncertainty < threshold).to(dt)
            consistency_loss = torch.sum(mask * consistency_dist) / (2 * torch.sum(mask) + 1e-16)
            extra = float(mask.sum())
            certain.append(float(mask.mean()))
            margin.append(float(((uncertainty - threshold).abs() / threshold).min()))
        else:
            # (losses.entropy_loss moves its log(C) constant with .cuda(); the generator runs on the CPU, so that one call is a no-op here)
            _cuda, torch.Tensor.cuda = torch.Tensor.cuda, lambda self, *a, **k: self
            try:
                consistency_loss = losses.entropy_loss(outputs_unlabeled_soft, C=4)
            finally:
                torch.Tensor.cuda = _cuda
        loss = supervised_loss + consistency_weight * consistency_loss
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        lr_ = BASE_LR * (1.0 - iter_num / MAX_IT) ** 0.9
        for param_group in optimizer.param_groups:
            param_group["lr"] = lr_
        iter_num = iter_num + 1
        rows.append([loss.item(), loss_ce.item(), loss_dice.item(), consistency_loss.item(), extra])
    sd = model.state_dict()
    return np.array(rows, dtype=np.float64), {k: sd[k].double().numpy().ravel()[:256].copy() for k in FINAL}, certain, margin


def usable(kind, r32, r64):
    """the generator's own checks of its inputs"""
    l32, f32, c32, m32 = r32
    l64, f64, c64, m64 = r64
    cols = slice(0, 4)
    spread = np.abs(l32[:, cols] - l64[:, cols]) / np.abs(l64[:, cols])
    fin = max(float(np.max(np.abs(f32[k] - f64[k])) / (np.max(np.abs(f64[k])) + 1e-6)) for k in FINAL)
    ok = spread[:2].max() < BOUNDS[0] / 3 and spread.max() < BOUNDS[1] / 3 and fin < BOUNDS[2] / 3
    why = f"spread first two {spread[:2].max():.2e}, all {spread.max():.2e}, finals {fin:.2e}"
    if kind == "semi_uamt":
        ok = ok and all(0.1 < c < 0.9 for c in c32 + c64) and min(m32 + m64) > 1e-3 and np.array_equal(l32[:, 4], l64[:, 4])
        why += f"; certain {min(c32):.2f} .. {max(c32):.2f}, closest to the threshold {min(m32 + m64):.2e}"
    return ok, why


def prescreen(d, teacher_seed):
    """semi_uamt: the teacher never changes, so its uncertainty maps do not depend on the training run -- the two mask conditions are
    checked on teacher forwards alone (masks drawn here, not the recorded ones: a screen, the full runs are asserted again)"""
    ema_model = UNet(1, NUM_CLASSES)
    load_det(ema_model, teacher_seed)
    with torch.no_grad():
        ema_model.decoder.out_conv.weight.mul_(SHARP)
    ema_model.train()
    torch.manual_seed(15)
    threshold = (0.75 + 0.25 * ramps.sigmoid_rampup(0, MAX_IT)) * np.log(2)
    for it in range(STEPS["semi_uamt"]):
        with torch.no_grad():
            p = torch.cat([F.softmax(ema_model(d["xu"][it].repeat(2, 1, 1, 1) + d["noiseT"][it, i]), dim=1) for i in range(4)], 0)
        p = p.reshape(8, N, NUM_CLASSES, P, P).mean(0)
        unc = -1.0 * torch.sum(p * torch.log(p + 1e-6), dim=1)
        if not (0.15 < float((unc < threshold).float().mean()) < 0.85) or float(((unc - threshold).abs() / threshold).min()) < 3e-3:
            return False
    return True


def gen(kind):
    d = inputs(kind)
    for teacher_seed in range(52, 2000):
        if kind == "semi_uamt" and not prescreen(d, teacher_seed):
            continue
        torch.manual_seed(15)
        masks = {}
        r32 = run(kind, d, teacher_seed, masks, "f32", torch.float32)
        r64 = run(kind, d, teacher_seed, masks, "f64", torch.float64)
        ok, why = usable(kind, r32, r64)
        print("   ", kind, "teacher seed", teacher_seed, "usable" if ok else "NOT usable", "--", why)
        if ok:
            break
    else:
        raise SystemExit(f"{kind}: no usable teacher initialisation found")
    out = {"meta_hyper": np.array([CONSISTENCY, RAMPUP, MAX_IT, BASE_LR, STUDENT_SEED, teacher_seed, SHARP if kind == "semi_uamt" else 1.0]),
           "in_xl": d["xl"].numpy(), "in_xu": d["xu"].numpy(), "in_lab": d["lab"].numpy(),
           "meta_losses_f32": r32[0], "meta_losses_f64": r64[0]}
    if "noise0" in d:
        out["in_noise0"] = d["noise0"].numpy()
    if "noiseT" in d:
        out["in_noiseT"] = d["noiseT"].numpy()
    for (it, which), ms in masks.items():
        for l, m in enumerate(ms):
            out[f"s{it}_{which}_em{l}"] = np.packbits(m.ravel())
    for k in FINAL:
        out[f"final_f32:{k}"], out[f"final_f64:{k}"] = r32[1][k].astype(np.float32), r64[1][k]
    print("   ", kind, "f32\n", r32[0], "\n    f64\n", r64[0])
    save("g15_" + kind, **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or list(STEPS):
        print(w)
        gen(w)
