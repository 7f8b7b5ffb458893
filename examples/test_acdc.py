#!/usr/bin/env python3
"""The reference's final step (code/test_2D_fully.py for unet / pnet, code/test_2D_fully_sps.py for unet_cct): load a checkpoint,
segment the test volumes of a fold, print Dice / HD95 / ASD (millimetres) per class and their mean, write the NIfTI files.

    python examples/test_acdc.py --root_path <.../data/ACDC> --nii_dir <.../data/ACDC_training> --model unet_cct \\
        --fold fold1 --ckpt <snapshot>/unet_cct_best_model.pth --save_path <out dir>
    python examples/test_acdc.py ... --fold all         # the five folds (one checkpoint per fold: --ckpt with {fold} in it)

--nii_dir holds the original `<case>.nii.gz` files whose headers give the voxel spacing (the reference hard-codes
../data/ACDC_training); --spacing X Y Z is the fallback where there is none.  With neither, distances are in voxels."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsl4mis_amd.test_2D_fully import Inference  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    # the reference's flags (test_2D_fully.py:19-31)
    ap.add_argument("--root_path", type=str, default="../data/ACDC")
    ap.add_argument("--exp", type=str, default="ACDC/WeaklySeg_pCE_MumfordShah_Loss")
    ap.add_argument("--model", type=str, default="unet", choices=["unet", "unet_cct", "pnet"])
    ap.add_argument("--fold", type=str, default="fold5", help="fold1 .. fold5, or all")
    ap.add_argument("--num_classes", type=int, default=4)
    ap.add_argument("--sup_type", type=str, default="scribble")
    # ours
    ap.add_argument("--ckpt", default=None, help="state_dict .pth (default: ../model/{exp}_{fold}/{sup_type}/iter_60000.pth); "
                    "'{fold}' in it is replaced by the fold's name")
    ap.add_argument("--nii_dir", default=None, help="directory of the original <case>.nii.gz files (voxel spacing, geometry)")
    ap.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="spacing in mm where no NIfTI exists")
    ap.add_argument("--save_path", default=None, help="where the *_pred / _img / _gt.nii.gz go; '{fold}' is replaced "
                    "(default: ../model/{exp}_{fold}/{sup_type}/{model}_predictions/)")
    ap.add_argument("--patch_size", type=int, nargs=2, default=[256, 256])
    FLAGS = ap.parse_args(argv)
    folds = ["fold{}".format(i) for i in range(1, 6)] if FLAGS.fold == "all" else [FLAGS.fold]
    ckpt, save_path = FLAGS.ckpt, FLAGS.save_path
    if len(folds) > 1 and ckpt and "{fold}" not in ckpt:           # one checkpoint for five folds would test four of them on
        ap.error("--fold all needs one checkpoint per fold: put {fold} into --ckpt")      # patients it was trained on
    if len(folds) > 1 and save_path and "{fold}" not in save_path:
        save_path = os.path.join(save_path, "{fold}")             # five folds never share (and wipe) one directory
    tables, total = {}, 0.0
    for fold in folds:
        FLAGS.fold = fold
        FLAGS.ckpt = ckpt.replace("{fold}", fold) if ckpt else None
        FLAGS.save_path = save_path.replace("{fold}", fold) if save_path else None
        print("Inference {}".format(fold))
        tables[fold] = Inference(FLAGS, return_table=True)
        total += tables[fold]["mean"][0]
    if len(folds) > 1:
        print(total / len(folds))                                 # test_2D_fully.py:168-177: the mean Dice of the folds
    return tables


if __name__ == "__main__":
    main()
