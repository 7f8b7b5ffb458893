"""Golden vectors of the Scribble2Label recipe (fixtures g13_s2l_*), from the reference's own code (code/train_s2l.py,
code/dataloaders/dataset_s2l.py).  Runs only where the reference checkout exists, like make_golden_pnet.py (it reuses save / load_det /
DropoutRecorder of make_golden.py); the tests read the .npz files it leaves.

dataset_s2l.py does not import here (h5py, torchvision), so random_rot_flip / random_rotate / RandomGenerator_s2l are lifted with ast;
the loss lines (train_s2l.py:123-147) and the update lines (:221-243) are restated with the same torch / scipy calls in the same
order, on the reference's own UNet.

  python tests/golden/make_golden_s2l.py [aug] [head] [update] [curve]
"""
import ast
import os
import random
import sys

import numpy as np
import torch
from scipy import ndimage
from scipy.ndimage import zoom
from torch.nn import CrossEntropyLoss

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import REF, DropoutRecorder, load_det, save  # noqa: E402
from networks.unet import UNet  # noqa: E402  (make_golden put the reference on sys.path)

from wsl4mis_amd.dataloaders import h5lite  # noqa: E402  (h5py is not installed: the project's reader, data only)


def lift_s2l():
    src = open(os.path.join(REF, "dataloaders/dataset_s2l.py")).read()
    env = {"np": np, "random": random, "ndimage": ndimage, "zoom": zoom, "torch": torch}
    want = ("random_rot_flip", "random_rotate", "RandomGenerator_s2l")
    body = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert len(body) == 3
    exec(compile(ast.Module(body=body, type_ignores=[]), "dataloaders/dataset_s2l.py", "exec"), env)
    return env["RandomGenerator_s2l"]


RandomGenerator_s2l = lift_s2l()
ACDC = os.path.join(HERE, "acdc", "ACDC_training_slices")


def weight_map(h, w, seed):
    """a random [h, w, 4] store with 8 bits of entropy per value (the tests rebuild it from the seed)"""
    return (np.random.default_rng([seed, 13]).integers(0, 256, (h, w, 4)).astype(np.float32) / np.float32(255)).astype(np.float32)


def classify(seed):
    """what RandomGenerator_s2l will draw after seeding both generators with `seed`"""
    random.seed(seed)
    np.random.seed(seed)
    if random.random() > 0.5:
        return ("rf", int(np.random.randint(0, 4)), int(np.random.randint(0, 2)))
    if random.random() > 0.5:
        return ("rot", int(np.random.randint(-20, 20)))
    return ("none",)


def gen_aug():
    files = sorted(os.listdir(ACDC))
    want = [("rf", k, a) for k in range(4) for a in range(2)] + [("none",)]
    seeds, angles = {}, {}
    for s in range(4000):
        c = classify(s)
        if c in want and c not in seeds:
            seeds[c] = s
        if c[0] == "rot" and c[1] not in angles and len(angles) < 40:
            angles[c[1]] = s
    assert len(seeds) == len(want)
    rot = [angles[a] for a in (-20, -7, -1, 0, 3, 11, 19)]
    cases = [(seeds[c], (64, 48)) for c in want] + [(s, (64, 48)) for s in rot] + [(seeds[("rf", 1, 0)], (256, 256)), (angles[-13], (256, 256))]
    out = {"meta_files": np.array(files), "meta_n": np.array(len(cases))}
    for i, (seed, size) in enumerate(cases):
        fname = files[i % len(files)]
        with h5lite.File(os.path.join(ACDC, fname)) as f:
            img, mask, scr = f["image"][:], f["label"][:], f["scribble"][:]
        w = weight_map(img.shape[0], img.shape[1], seed)
        random.seed(seed)
        np.random.seed(seed)
        r = RandomGenerator_s2l(size)({"image": img, "mask": mask, "scribble": scr, "weight": w})
        t = f"c{i:02d}"
        out.update({f"{t}_file": np.array(i % len(files)), f"{t}_seed": np.array(seed), f"{t}_size": np.array(size),
                    f"{t}_draw": np.array([{"none": 0, "rf": 1, "rot": 2}[classify(seed)[0]]] + list(classify(seed)[1:])),
                    f"{t}_image": r["image"].numpy(), f"{t}_mask": r["mask"].numpy(), f"{t}_scribble": r["scribble"].numpy(),
                    f"{t}_weight": r["weight"].numpy()})
        # the state of both generators afterwards, probed by their next draws
        random.seed(seed)
        np.random.seed(seed)
        RandomGenerator_s2l(size)({"image": img, "mask": mask, "scribble": scr, "weight": w})
        out[f"{t}_next"] = np.array([random.random(), float(np.random.randint(0, 1 << 30))])
    save("g13_s2l_aug", **out)


def s2l_loss_lines(outputs, scribble, store, thr_conf, classes=4, ignore=4):
    """The loss of train_s2l.py:124-147 from thr_iter on, restated class by class with the reference's torch calls in the reference's
    order (where / zeros_like + c / ones_like per class, then the masked writes in rising class order, so the highest class wins)."""
    ce = CrossEntropyLoss(ignore_index=ignore)
    loss_ce = ce(outputs, scribble.long())
    scr = scribble.long().cpu()
    unlabelled, nothing = scr == ignore, float(ignore) * torch.ones_like(scr)
    per_class = [torch.where((store[..., c] > thr_conf) & unlabelled, torch.zeros_like(store[..., c]) + c, nothing) for c in range(classes)]
    u_labels = torch.ones_like(per_class[0]).long() * ignore
    for c, cand in enumerate(per_class):
        u_labels[cand == c] = c
    loss_u = CrossEntropyLoss(ignore_index=ignore)(outputs, u_labels)
    return loss_ce + 0.5 * loss_u, loss_ce, loss_u, u_labels


def gen_head():
    N, H, W, C = 3, 24, 20, 4
    out = {}
    for tag, thr, seed in (("a", 0.8, 1), ("b", 0.3, 2), ("c", 0.8, 3)):
        g = torch.Generator().manual_seed(100 + seed)
        z = (torch.randn((N, C, H, W), generator=g) * 2).requires_grad_()
        scr = torch.randint(0, 4, (N, H, W), generator=g)
        scr[torch.rand((N, H, W), generator=g) < 0.8] = 4
        w = torch.rand((N, H, W, C), generator=g)
        if tag == "a":        # mostly low, some confident; planted: float32(thr) and one ulp either side, on unlabelled pixels
            w = w * 0.7
            hot = torch.rand((N, H, W), generator=g) < 0.3
            cls = torch.randint(0, 4, (N, H, W), generator=g)
            w[hot] = w[hot] * 0.1
            w[hot, cls[hot]] = 0.9
            t32 = np.float32(thr)
            scr[0, 0, 0:6] = 4
            w[0, 0, 0:6] = 0.1
            w[0, 0, 0, 1], w[0, 0, 1, 2], w[0, 0, 2, 3] = float(t32), float(np.nextafter(t32, np.float32(1))), float(np.nextafter(t32, np.float32(0)))
            w[0, 0, 3, 0], w[0, 0, 4, 0] = float(np.nextafter(t32, np.float32(1))), float(t32)
        elif tag == "b":      # thr 0.3: two classes over the threshold on many pixels -- the highest class wins
            w = w * 0.5
            w[..., 1][torch.rand((N, H, W), generator=g) < 0.5] = 0.45
            w[..., 3][torch.rand((N, H, W), generator=g) < 0.3] = 0.31
        else:                 # no confident pixel: the second CE and the loss are NaN
            w = w * 0.79
        loss, ce, cu, u = s2l_loss_lines(z, scr.to(torch.uint8), w, thr)
        loss.backward()
        out.update({f"{tag}_z": z.detach().numpy(), f"{tag}_scribble": scr.numpy().astype(np.uint8), f"{tag}_weight": w.numpy(),
                    f"{tag}_thr": np.array(thr), f"{tag}_losses": np.array([loss.item(), ce.item(), cu.item()], dtype=np.float32),
                    f"{tag}_counts": np.array([int((scr != 4).sum()), int((u != 4).sum())]), f"{tag}_u": u.numpy().astype(np.uint8),
                    f"{tag}_dz": z.grad.numpy().copy()})
        print("   ", tag, out[f"{tag}_losses"], out[f"{tag}_counts"], "dz finite:", bool(np.isfinite(out[f"{tag}_dz"]).all()))
    assert np.isnan(out["c_losses"][0]) and np.isnan(out["c_losses"][2]) and out["c_counts"][1] == 0
    u, w, s = out["b_u"], out["b_weight"], out["b_scribble"]
    assert int((((w > np.float32(0.3)).sum(-1) >= 2) & (s == 4)).sum()) > 20
    assert out["a_u"][0, 0, 0] == 4 and out["a_u"][0, 0, 1] == 2 and out["a_u"][0, 0, 2] == 4 and out["a_u"][0, 0, 3] == 0 and out["a_u"][0, 0, 4] == 4
    save("g13_s2l_head", **out)


def update_lines(store, logits, alpha, patch):
    """The update of train_s2l.py:228-243 for one slice, restated as a loop over the classes: `logits` [1,C,P,P] is model(img);
    softmax, order-0 zoom back to the store's size, then per class alpha * pred + (1 - alpha) * old in fp32 tensors with Python-double
    factors, as the reference computes it.  Returns the new store."""
    h, w, classes = store.shape
    pred = torch.nn.functional.softmax(logits, dim=1).squeeze(0).cpu().numpy()
    pred = torch.from_numpy(zoom(pred, (1, h / patch, w / patch), order=0))
    new = torch.from_numpy(store)
    for c in range(classes):
        new[..., c] = alpha * pred[c] + (1 - alpha) * new[..., c]
    return new.numpy()


def gen_update():
    sizes, alpha, P = [(45, 38), (20, 25), (50, 17)], 0.2, 32
    g = torch.Generator().manual_seed(77)
    out = {"meta_sizes": np.array(sizes), "meta_alpha": np.array(alpha)}
    stores = [np.zeros((h, w, 4), dtype=np.float32) for h, w in sizes]
    for r in range(2):
        z = torch.randn((len(sizes), 4, P, P), generator=g) * 3
        out[f"z{r}"] = z.numpy()
        for i in range(len(sizes)):
            stores[i] = update_lines(stores[i].copy(), z[i:i + 1], alpha, P)
            assert stores[i].shape == sizes[i] + (4,) and stores[i].dtype == np.float32
            out[f"w{r}_{i}"] = stores[i].copy()
    save("g13_s2l_update", **out)


def synth_slices():
    sizes = [(40, 36), (33, 44), (32, 32), (50, 34), (36, 48), (45, 39)]
    rng = np.random.default_rng(2024)
    sl = []
    for h, w in sizes:
        img = rng.random((h, w), dtype=np.float32)
        mask = rng.integers(0, 4, (h, w)).astype(np.uint8)
        scr = np.full((h, w), 4, dtype=np.uint16)
        lab = rng.random((h, w)) < 0.1
        scr[lab] = mask[lab]
        sl.append({"image": img, "mask": mask, "scribble": scr, "weight": np.zeros((h, w, 4), dtype=np.float32)})
    return sl


def packed(rec):
    return [np.packbits(m.ravel()) for m, _ in rec.elem]


def gen_curve(aug_seed=500, torch_seed=0):
    """UNet(1,4), six synthetic slices, patch 32 x 32, N = 4, thr_iter 2, period_iter 1, alpha 0.6, thr_conf 0.4, six steps of
    train_s2l.py's loop (SGD + poly LR), with every dropout mask recorded.  torch_seed fixes the dropout draws, so the fixture can be
    regenerated; both seeds are ones for which the asserts on near_thr below hold."""
    torch.manual_seed(torch_seed)
    P, N, steps, thr_iter, period, alpha, thr = 32, 4, 6, 2, 1, 0.6, 0.4
    sl = synth_slices()
    model = UNet(1, 4)
    load_det(model, 31)
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    tf = RandomGenerator_s2l([P, P])
    out = {"meta_sizes": np.array([s["image"].shape for s in sl]), "meta_aug_seed": np.array(aug_seed)}
    for i, s in enumerate(sl):
        out.update({f"in{i}_image": s["image"], f"in{i}_mask": s["mask"], f"in{i}_scribble": s["scribble"]})
    losses, n_u, near_store, near_batch, idx_all = [], [], [], [], []
    iter_num, n_store = 0, sum(s["image"].size for s in sl)
    for it in range(steps):
        idxs = [(it * N + j) % len(sl) for j in range(N)]
        idx_all.append(idxs)
        random.seed(aug_seed + it)
        np.random.seed(aug_seed + it)
        batch = [tf(sl[i]) for i in idxs]
        volume = torch.stack([b["image"] for b in batch])
        label = torch.stack([b["scribble"] for b in batch])
        weight = torch.stack([b["weight"] for b in batch])
        with DropoutRecorder() as rec:
            outputs = model(volume)
        if iter_num < thr_iter:
            loss = loss_ce = CrossEntropyLoss(ignore_index=4)(outputs, label.long())
            loss_u, nu, nb = torch.zeros(()), 0, 0
        else:
            loss, loss_ce, loss_u, u = s2l_loss_lines(outputs, label, weight, thr)
            nu = int((u != 4).sum())
            nb = int(((np.abs(weight.numpy() - thr) <= 1e-4 * thr).any(-1) & (label.numpy() == 4)).sum())
        opt.zero_grad()
        loss.backward()
        opt.step()
        lr_ = 0.01 * (1.0 - iter_num / 60000) ** 0.9
        for pg in opt.param_groups:
            pg["lr"] = lr_
        iter_num += 1
        losses.append([loss.item(), loss_ce.item(), float(loss_u)])
        n_u.append(nu)
        near_batch.append(nb)
        for l, m in enumerate(packed(rec)):
            out[f"s{it}_em{l}"] = m
        if iter_num > 0 and iter_num % period == 0:
            for idx, images in enumerate(sl):
                img = images["image"]
                img = zoom(img, (P / img.shape[0], P / img.shape[1]), order=0)
                img = torch.from_numpy(img).unsqueeze(0).unsqueeze(0)
                with torch.no_grad(), DropoutRecorder() as rec:
                    logits = model(img)
                images["weight"] = update_lines(images["weight"], logits, alpha, P)
                for l, m in enumerate(packed(rec)):
                    out[f"u{it}_{idx}_em{l}"] = m
            near_store.append(sum(int((np.abs(s["weight"] - thr) <= 1e-4 * thr).any(-1).sum()) for s in sl))
            if it == 0:
                for idx, s in enumerate(sl):
                    out[f"store0_{idx}"] = s["weight"].copy()
                for k, b in model.named_buffers():
                    out[f"buf0:{k}"] = b.numpy().copy()
    near_store, near_batch = np.array(near_store), np.array(near_batch)
    print("    losses", np.array(losses), "n_u", n_u, "near_thr", near_store, "in the batches", near_batch)
    assert near_store.max() <= 1e-3 * n_store, (near_store, n_store)
    # a batch pixel can only flip if it came from a store pixel near the threshold: the bound the test applies is the store's count
    assert all(near_batch[s] <= near_store[s - 1] for s in range(thr_iter, steps)), (near_batch, near_store)
    assert all(n > 0 for n in n_u[thr_iter:])
    out.update(meta_losses=np.array(losses, dtype=np.float32), meta_n_u=np.array(n_u), meta_near_thr=near_store,
               meta_near_thr_batch=near_batch, meta_idxs=np.array(idx_all), meta_hyper=np.array([thr_iter, period, alpha, thr]))
    sd = model.state_dict()
    for k in ("encoder.in_conv.conv_conv.0.weight", "decoder.out_conv.weight", "encoder.down4.maxpool_conv.1.conv_conv.5.running_var"):
        out[f"final:{k}"] = sd[k].numpy().ravel()[:256].copy()
    save("g13_s2l_curve", **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["aug", "head", "update", "curve"]:
        print(w)
        {"aug": gen_aug, "head": gen_head, "update": gen_update, "curve": gen_curve}[w]()
