"""Scribble2Label data path (ref: code/dataloaders/dataset_s2l.py:19-153).

`BaseDataSets_s2l` holds every slice of the fold's training patients in memory, each with a `weight` store [h, w, 4] float32 that
starts as zeros: the running average of the network's predictions at the slice's native size, which the trainer refreshes every
`period_iter` steps (`TrainEngine.update_ensemble`) and the loss head thresholds into pseudo labels.  `RandomGenerator_s2l`
draws exactly like `RandomGenerator` (`random.random()`, then `np.random.randint(0, 4)` and `randint(0, 2)`, or `random.random()`
and `randint(-20, 20)`) and carries all four arrays -- image, mask, scribble, weight -- through the same index map.  Unlike
`dataset_semi.py` the reference calls `ndimage.rotate` without `cval` here, so rotated-in corners are 0 in every array, the
scribble included: they become labelled background.  The pixels come from ONE gather launch for a whole batch
(`wsl_augment_batch_s2l`, csrc/wsl_s2l.hip) and equal numpy / scipy bit for bit (tests/test_s2l_ops.py).  No CPU fallback.

Extension: the `weight` arrays in `.images[idx]` are DEVICE tensors, not numpy arrays -- the update pass writes them and the
augmentation reads them on the GPU, so the store never crosses PCIe.  `.images[idx]['weight'].cpu().numpy()` gives the
reference's array."""
import os
from collections import defaultdict

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _lib
from .. import runtime as rt
from . import h5lite
from .dataset import _rotate_matrix, draw_params


class BaseDataSets_s2l(Dataset):
    """ref: dataset_s2l.py:19-100.  `num` is accepted and unused, like the reference's.  `class_num` (extension) is the last axis
    of the weight stores (the reference hard-codes 4)."""

    FOLDS = ("fold1", "fold2", "fold3", "fold4", "fold5")

    def __init__(self, base_dir=None, transform=None, fold="fold1", num=None, class_num=4):
        if fold not in self.FOLDS:
            raise ValueError(f"unknown fold {fold!r} (the reference returns 'ERROR KEY' here and fails later)")
        self._base_dir, self.transform, self.class_num = base_dir, transform, int(class_num)
        k = self.FOLDS.index(fold)
        test_ids = ["patient{:0>3}".format(i) for i in range(20 * k + 1, 20 * k + 21)]
        train_ids = [p for p in ("patient{:0>3}".format(i) for i in range(1, 101)) if p not in test_ids]
        sl = os.path.join(base_dir, "ACDC_training_slices")
        self.all_slices = os.listdir(sl)
        self.sample_list = [f for pid in train_ids for f in self.all_slices if f.startswith(pid)]     # per patient, listing order
        dev = rt.device()
        self.images = defaultdict(dict)
        self._dev = {}
        for idx, case in enumerate(self.sample_list):
            with h5lite.File(os.path.join(sl, case)) as f:
                e = self.images[idx]
                e["id"] = case
                e["image"], e["mask"], e["scribble"] = f["image"][:], f["label"][:], f["scribble"][:]
            h, w = e["mask"].shape
            e["weight"] = torch.zeros((h, w, self.class_num), dtype=torch.float32, device=dev)

    @classmethod
    def from_slices(cls, slices, transform=None, class_num=4):
        """(extension) a dataset over in-memory slices -- dicts with 'image', 'mask', 'scribble' [h, w] arrays and optionally 'id' --
        instead of the ACDC directory layout: same samples, same zero-initialised stores"""
        self = cls.__new__(cls)
        self._base_dir, self.transform, self.class_num = None, transform, int(class_num)
        self.all_slices = self.sample_list = [str(s.get("id", f"slice{i}")) for i, s in enumerate(slices)]
        self.images, self._dev = defaultdict(dict), {}
        for idx, s in enumerate(slices):
            h, w = np.asarray(s["mask"]).shape
            self.images[idx].update(id=self.sample_list[idx], image=np.asarray(s["image"]), mask=np.asarray(s["mask"]),
                                    scribble=np.asarray(s["scribble"]),
                                    weight=torch.zeros((h, w, self.class_num), dtype=torch.float32, device=rt.device()))
        return self

    def __len__(self):
        return len(self.sample_list)

    def staged(self, idx):
        """(image f32, mask u8, scribble u8) of slice idx as device tensors, staged on first use and kept (they never change)"""
        hit = self._dev.get(idx)
        if hit is None:
            e, dev = self.images[idx], rt.device()
            hit = self._dev[idx] = (torch.as_tensor(np.asarray(e["image"]), dtype=torch.float32).to(dev).contiguous(),
                                    torch.as_tensor(np.asarray(e["mask"]).astype(np.uint8)).to(dev).contiguous(),
                                    torch.as_tensor(np.asarray(e["scribble"]).astype(np.uint8)).to(dev).contiguous())
        return hit

    def __getitem__(self, idx):
        e = self.images[idx]
        sample = {"image": e["image"], "mask": e["mask"], "scribble": e["scribble"], "weight": e["weight"]}
        if self.transform is not None:
            sample = self.transform(sample)
        else:      # (extension) the raw sample for BatchRandomGenerator_s2l, with the device copies of the three fixed arrays
            sample["staged"] = self.staged(idx)
        sample["id"] = e["id"]
        return sample


def augment_batch_s2l(images, masks, scribbles, weights, params, output_size):
    """images: list of [h,w] float32, masks / scribbles: lists of [h,w] integer arrays (masks may be None), weights: list of
    [h,w,C] float32 (arrays or tensors on any device; moved to the GPU), params: list of dicts from dataset.draw_params.
    Returns (image [N,1,Ho,Wo] f32, mask [N,Ho,Wo] u8 or None, scribble [N,Ho,Wo] u8, weight [N,Ho,Wo,C] f32) on the device."""
    L = _lib.lib()
    dev = rt.device()
    n = len(images)
    Ho, Wo = int(output_size[0]), int(output_size[1])
    keep = []
    arr = (_lib.WslAugSampleS2l * n)()
    C_ = None

    def u8(a):
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8)))      # the scribble is uint16 on disk
        return a.to(dev, torch.uint8).contiguous()

    for i, p in enumerate(params):
        im = torch.as_tensor(images[i], dtype=torch.float32).to(dev).contiguous()
        sc = u8(scribbles[i])
        mk = u8(masks[i]) if masks is not None and masks[i] is not None else None
        wt = torch.as_tensor(weights[i], dtype=torch.float32).to(dev).contiguous()
        if im.dim() != 2 or sc.shape != im.shape or (mk is not None and mk.shape != im.shape) or wt.dim() != 3 or \
                tuple(wt.shape[:2]) != tuple(im.shape) or (C_ is not None and wt.shape[2] != C_):
            raise ValueError(f"augment_batch_s2l: sample {i}: image {tuple(im.shape)}, scribble {tuple(sc.shape)}, weight "
                             f"{tuple(wt.shape)} do not fit")
        C_ = wt.shape[2]
        keep += [im, sc, mk, wt]
        s = arr[i]
        s.img, s.mask, s.scr, s.weight, s.h, s.w = rt.ptr(im), rt.ptr(mk), rt.ptr(sc), rt.ptr(wt), im.shape[0], im.shape[1]
        s.op, s.k, s.axis = p["op"], p.get("k", 0), p.get("axis", 0)
        if p["op"] == 2:
            m, off = _rotate_matrix(p["angle"], im.shape)
            s.m00, s.m01, s.m10, s.m11, s.off0, s.off1 = m[0, 0], m[0, 1], m[1, 0], m[1, 1], off[0], off[1]
    with_mask = masks is not None and any(m is not None for m in masks)
    out_img = torch.empty((n, 1, Ho, Wo), dtype=torch.float32, device=dev)
    out_mask = torch.empty((n, Ho, Wo), dtype=torch.uint8, device=dev) if with_mask else None
    out_scr = torch.empty((n, Ho, Wo), dtype=torch.uint8, device=dev)
    out_w = torch.empty((n, Ho, Wo, C_), dtype=torch.float32, device=dev)
    _lib.check(L.wsl_augment_batch_s2l(arr, n, C_, rt.ptr(out_img), rt.ptr(out_mask), rt.ptr(out_scr), rt.ptr(out_w), Ho, Wo,
                                       rt.stream()))
    return out_img, out_mask, out_scr, out_w


def _draw():
    """RandomGenerator_s2l's random decisions for one sample: RandomGenerator's draw order (dataset_s2l.py:132-137); no fill value
    to pick, so the scribble is not inspected"""
    return draw_params(None, has_ignore=False)


class RandomGenerator_s2l(object):
    """Same call contract as the reference class: {'image', 'mask', 'scribble', 'weight'} of one slice in, {'image': [1,H,W]
    float32, 'mask': [H,W] uint8, 'scribble': [H,W] uint8, 'weight': [H,W,4] float32} out, as device tensors."""

    def __init__(self, output_size):
        self.output_size = output_size

    def __call__(self, sample):
        img, mk, sc, wt = augment_batch_s2l([sample["image"]], [sample["mask"]], [sample["scribble"]], [sample["weight"]], [_draw()],
                                            self.output_size)
        return {"image": img[0], "mask": mk[0], "scribble": sc[0], "weight": wt[0]}


class BatchRandomGenerator_s2l(object):
    """The batched form the engine wants: a list of raw samples (a BaseDataSets_s2l built with transform=None) in, the device batch
    (image [N,1,H,W], mask [N,H,W], scribble [N,H,W], weight [N,H,W,4]) out of one launch; draws per sample in list order."""

    def __init__(self, output_size):
        self.output_size = output_size

    def __call__(self, samples):
        params = [_draw() for _ in samples]
        st = [s.get("staged") or (s["image"], s["mask"], s["scribble"]) for s in samples]
        return augment_batch_s2l([t[0] for t in st], [t[1] for t in st], [t[2] for t in st], [s["weight"] for s in samples], params,
                                 self.output_size)
