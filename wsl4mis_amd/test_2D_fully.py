"""The offline test stage of the reference (ref: code/test_2D_fully.py:74-165 for `unet`, code/test_2D_fully_sps.py:74-168 for
`unet_cct`): load a checkpoint, segment every test volume of a fold, compute Dice, HD95 and ASD in MILLIMETRES from the voxel
spacing of the case's NIfTI file, write prediction / image / ground truth as NIfTI and print the per-class and mean table.

Names and semantics are the reference's (`calculate_metric_percase`, `test_single_volume`, `Inference`); medpy, SimpleITK and
h5py are replaced by `val_2D` (surfaces and nearest-surface distances on the device), `niilite` and `h5lite`.  What differs:
  * the forward is batched over the slices (`val_2D._predict_volume`; bit-equality of a batch and its parts is tested);
  * a dual-branch net (`unet_cct`) is read at its FIRST output, as test_2D_fully_sps.py:97-101 does -- one module serves both;
  * each label volume is uploaded once and the pred -> gt distances are shared between ASD and HD95;
  * where the reference hard-codes paths, FLAGS carries them: `ckpt`, `nii_dir`, `spacing`, `save_path`, `patch_size`
    (all optional: the reference's `../model/{exp}_{fold}/{sup_type}` layout and `iter_60000.pth` are the defaults)."""
import os
import shutil

import numpy as np
import torch

from . import runtime as rt
from . import val_2D
from .dataloaders import h5lite, niilite
from .dataloaders.dataset import BaseDataSets
from .networks.net_factory import net_factory


def calculate_metric_percase(pred, gt, spacing):
    """ref: test_2D_fully.py:74-80 -> (dice, hd95, asd) of one class; medpy's dc / hd95 / asd with voxelspacing=spacing.
    An empty mask raises medpy's RuntimeError (asd and hd95 do there); nothing is hidden.  Masks: numpy arrays or device tensors."""
    pred = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(pred) > 0)).to(rt.device())
    gt = gt if isinstance(gt, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(gt) > 0)).to(rt.device())
    pred, gt = pred != 0, gt != 0
    inter, total = int((pred & gt).sum()), int(pred.sum()) + int(gt.sum())
    dice = 2.0 * inter / float(total) if total else 0.0         # medpy.metric.binary.dc
    hd95, asd = val_2D.hd95_asd_percase(pred, gt, voxelspacing=spacing)
    return dice, hd95, asd


def _case_spacing(case, FLAGS):
    """(spacing_xyz, header or None): the case's NIfTI under FLAGS.nii_dir, else FLAGS.spacing, else unit voxels"""
    nii_dir = getattr(FLAGS, "nii_dir", None)
    if nii_dir:
        for ext in (".nii.gz", ".nii"):
            p = os.path.join(nii_dir, case + ext)
            if os.path.exists(p):
                h = niilite.read_header(p)
                return tuple(float(v) for v in h["pixdim"][1:4]), h
        print("warning: no {}.nii.gz under {}: falling back to --spacing / unit voxels for this case".format(case, nii_dir))
    sp = getattr(FLAGS, "spacing", None)
    return (tuple(float(v) for v in sp) if sp is not None else (1.0, 1.0, 1.0)), None


def test_single_volume(case, net, test_save_path, FLAGS):
    """ref: test_2D_fully.py:83-124 / test_2D_fully_sps.py:83-126.  -> one (dice, hd95, asd) per class 1 .. num_classes-1.

    The spacing handed to the metrics is (s[2], s[0], s[1]) with s = the NIfTI's (x, y, z) spacing, EXACTLY as the reference
    passes it (:108-113).  The arrays are [z, y, x], so this gives the array's y axis the file's x spacing and the array's x axis
    the file's y spacing -- swapped in plane.  ACDC is isotropic in plane, so the published numbers do not depend on it; the
    quirk is kept (and pinned by a test with x != y) so that results stay comparable with the reference's."""
    with h5lite.File(os.path.join(FLAGS.root_path, "ACDC_training_volumes", case)) as f:
        image, label = f["image"][:], f["label"][:]
    patch = tuple(getattr(FLAGS, "patch_size", None) or (256, 256))
    prediction = val_2D._predict_volume(image, net, patch, first_output=True).astype(label.dtype)
    case = case.replace(".h5", "")
    s, like = _case_spacing(case, FLAGS)
    spacing = (s[2], s[0], s[1])
    # (the files are written BEFORE the metrics, unlike :108-123: when a class is empty and medpy's error ends the run, the
    #  prediction that caused it is on disk)
    for arr, tag in ((prediction, "_pred"), (image, "_img"), (label, "_gt")):
        out = os.path.join(test_save_path, case + tag + ".nii.gz")
        if like is not None:
            niilite.write_volume(out, arr.astype(np.float32), like=like)
        else:
            niilite.write_volume(out, arr.astype(np.float32), spacing_xyz=s)
    pred_d, lab_d = torch.from_numpy(prediction).to(rt.device()), torch.from_numpy(np.ascontiguousarray(label)).to(rt.device())
    return tuple(calculate_metric_percase(pred_d == c, lab_d == c, spacing) for c in range(1, int(getattr(FLAGS, "num_classes", 4))))


test_single_volume.__test__ = False        # (name kept from the reference; not a pytest case)


def Inference(FLAGS, return_table=False):
    """ref: test_2D_fully.py:127-165.  Prints the per-class mean (dice, hd95, asd) over the fold's test volumes and the mean over
    the classes; returns the mean Dice like the reference, or with return_table the whole table
    {"cases", "per_case", "per_class", "mean"}."""
    image_list = BaseDataSets(base_dir=FLAGS.root_path, split="val", fold=FLAGS.fold).sample_list      # the reference's fold split
    if not image_list:
        raise RuntimeError(f"no test volume of {FLAGS.fold} under {FLAGS.root_path}/ACDC_training_volumes")
    snapshot_path = "../model/{}_{}/{}".format(FLAGS.exp, FLAGS.fold, FLAGS.sup_type)
    test_save_path = getattr(FLAGS, "save_path", None)
    if not test_save_path:                                       # the reference's own directory is emptied first, as it does;
        test_save_path = "../model/{}_{}/{}/{}_predictions/".format(FLAGS.exp, FLAGS.fold, FLAGS.sup_type, FLAGS.model)
        if os.path.exists(test_save_path):                       # a directory the caller names is never wiped
            shutil.rmtree(test_save_path)
    os.makedirs(test_save_path, exist_ok=True)
    if not getattr(FLAGS, "nii_dir", None) and getattr(FLAGS, "spacing", None) is None:
        print("warning: neither --nii_dir nor --spacing is given: the spacing is 1 1 1, HD95 and ASD are in VOXELS, not millimetres")
    net = net_factory(net_type=FLAGS.model, in_chns=1, class_num=FLAGS.num_classes)
    save_mode_path = getattr(FLAGS, "ckpt", None) or os.path.join(snapshot_path, "iter_60000.pth")
    net.load_state_dict(torch.load(save_mode_path, map_location="cpu"))
    print("init weight from {}".format(save_mode_path))
    net.eval()
    per_case = []
    for case in image_list:
        print(case)
        per_case.append(np.asarray(test_single_volume(case, net, test_save_path, FLAGS), dtype=np.float64))
    avg_metric = sum(per_case) / len(image_list)                 # [class][dice, hd95, asd]
    mean = avg_metric.sum(axis=0) / avg_metric.shape[0]
    print([row for row in avg_metric])
    print(mean)
    if return_table:
        return {"cases": list(image_list), "per_case": per_case, "per_class": avg_metric, "mean": mean}
    return mean[0]
