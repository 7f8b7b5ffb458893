#!/usr/bin/env python3
"""End-to-end trainer on the reference's ACDC layout, built only from this package's pieces -- the flow of
code/train_weakly_supervised_pCE_WSL4MIS (ours_proposed) / ..._pCE_GatedCRFLoss_2D.py, one process per GPU:

    BaseDataSets(h5lite) -> BatchRandomGenerator (device augmentation) -> TrainEngine.step -> val_2D metrics

--loss s2l is the flow of code/train_s2l.py (Scribble2Label): BaseDataSets_s2l keeps a running prediction average per training slice,
BatchRandomGenerator_s2l carries it through the augmentation, the engine reads it from --thr_iter on and refreshes it after every
--period_iter steps (TrainEngine.update_ensemble).
--loss pce_interintra is the flow of code/train_weakly_supervised_pCE_Inter&Intra_Class_2D.py: pCE + w(t) * (inter-class variance -
intra-class variance of image * softmax), w(t) = --consistency * sigmoid_rampup(iteration // 150, --consistency_rampup), on unet (or pnet).
--loss semi_mt | semi_uamt | semi_entmin is the flow of code/train_mean_teacher_2D.py, train_uncertainty_aware_mean_teacher_2D.py and
train_entropy_minimization_2D.py (code/train_semi.sh): two datasets (labeled_type "labeled" with dense labels, "unlabeled"), two loaders of
--batch_size // 2 each, zip(cycle(labeled), unlabeled); the student runs on both halves, 0.5 * (CE + Dice) on the labeled one and
w(t) * the consistency / entropy term on the unlabeled one, w(t) = --consistency * sigmoid_rampup(iteration // 300, --consistency_rampup).
--teacher_update frozen is the reference's scripts to the letter (they never call update_ema_variables); the default ema is the method.
--loss semi_dan is the flow of code/train_deep_adversarial_network_2D.py on the same two datasets and loaders: 0.5 * (CE + Dice) on the
labeled half plus w(t) * CE(DAN(softmax(z_u), x_u), 1) on the unlabeled one, w(t) = --consistency * sigmoid_rampup(iteration // 150,
--consistency_rampup), then the adversary's own Adam step (FCDiscriminator, --dan_ndf filters; --dan_pool 7 needs a 224 .. 335 patch).
(train_partially_fully_supervised.py is --loss ce_dice --sup_type label --labeled_type labeled.)

    python examples/train_acdc_scribble.py --root_path <.../data/ACDC> --fold fold1 --max_iterations 60000
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_acdc_scribble.py ...

Each rank draws its own batches (independent shuffles), gradients are averaged by the engine."""
import argparse
import os
import random
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before HIP loads: keeps RCCL's streams off the decoder side stream's queue (bench.py)

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsl4mis_amd import _lib, val_2D  # noqa: E402
from wsl4mis_amd.dataloaders.dataset import BaseDataSets, BatchRandomGenerator  # noqa: E402
from wsl4mis_amd.dataloaders.dataset_s2l import BaseDataSets_s2l, BatchRandomGenerator_s2l  # noqa: E402
from wsl4mis_amd.engine import TrainEngine  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_path", required=True)
    ap.add_argument("--fold", default="fold1")
    ap.add_argument("--sup_type", default="scribble")
    ap.add_argument("--model", default=None, choices=["unet_cct", "unet", "pnet"], help="default: unet_cct, and unet for --loss s2l / "
                    "pce_interintra (single-decoder compositions: unet or pnet)")
    ap.add_argument("--loss", default="ours_proposed", choices=["ours_proposed", "pce", "pce_gatedcrf", "pce_tv", "pce_ms", "pce_entropy", "ce_dice", "mean_teacher", "ustm", "s2l", "pce_interintra",
                                                                     "semi_mt", "semi_uamt", "semi_entmin", "semi_dan"])
    # inter/intra-class variance (train_weakly_supervised_pCE_Inter&Intra_Class_2D.py:62-65)
    ap.add_argument("--consistency", type=float, default=0.1, help="pce_interintra / semi_*: the weight's plateau")
    ap.add_argument("--consistency_rampup", type=float, default=200.0, help="pce_interintra / semi_*: length of the sigmoid ramp in units of "
                    "150 (semi_mt / semi_uamt / semi_entmin: 300) iterations (0 = constant weight)")
    # semi-supervised trainers (train_mean_teacher_2D.py:60-66)
    ap.add_argument("--ema_decay", type=float, default=0.99)
    ap.add_argument("--teacher_update", default="ema", choices=["ema", "frozen"], help="semi_mt / semi_uamt: 'frozen' = the reference's "
                    "scripts literally (update_ema_variables is defined and never called: the teacher keeps its initial weights)")
    # the adversary of semi_dan (train_deep_adversarial_network_2D.py:117-123)
    ap.add_argument("--dan_lr", type=float, default=1e-4)
    ap.add_argument("--dan_ndf", type=int, default=64)
    ap.add_argument("--dan_pool", type=int, default=7, help="semi_dan: window of the adversary's AvgPool2d (the reference's 7 fits patches of "
                    "224 .. 335; the pooled map must have 4 positions)")
    # Scribble2Label (train_s2l.py:62-65)
    ap.add_argument("--period_iter", type=int, default=100)
    ap.add_argument("--thr_iter", type=int, default=6000)
    ap.add_argument("--thr_conf", type=float, default=0.8)
    ap.add_argument("--alpha", type=float, default=0.2)
    ap.add_argument("--ensemble_mode", default="reference", choices=["reference", "eval"], help="s2l: 'reference' = the reference's update "
                    "pass (one train-mode forward per slice), 'eval' = batched eval-mode forwards (a departure: TrainEngine.update_ensemble)")
    ap.add_argument("--num_classes", type=int, default=4)
    ap.add_argument("--max_iterations", type=int, default=60000)
    ap.add_argument("--stop_iterations", type=int, default=0, help="stop after this many iterations while keeping the poly schedule "
                    "of --max_iterations (short-schedule comparisons against the oracle: tests/acdc_oracle_arm/oracle_acdc_short.py)")
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--base_lr", type=float, default=0.01)
    ap.add_argument("--patch_size", type=int, nargs=2, default=[256, 256])
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--val_every", type=int, default=200)
    ap.add_argument("--labeled_type", default="all", help="'all' = every training patient of the fold (upstream WSL4MIS's weakly-"
                    "supervised runs), 'labeled' / 'unlabeled' = the subsets of dataset_semi.py")
    ap.add_argument("--snapshot_path", default=None, help="write the reference's checkpoints here (state_dict .pth files)")
    ap.add_argument("--save_every", type=int, default=3000)
    ap.add_argument("--val_path", default="host", choices=["host", "device"], help="validation: 'host' = scipy zoom and numpy masks per "
                    "slice (the reference's loop); 'device' = val_2D.VolumeValidator (zoom, argmax and Dice counts in HIP kernels, the "
                    "volumes uploaded once; equal label maps and Dice)")
    ap.add_argument("--no_hd95", action="store_true", help="validation: Dice only (the model-selection metric), skip HD95")
    ap.add_argument("--log_every", type=int, default=20)
    ap.add_argument("--quiet", action="store_true", help="no per-iteration lines (validation lines stay)")
    ap.add_argument("--curve_json", default=None, help="write the loss / validation curve here (rank 0)")
    ap.add_argument("--oracle_stream", action="store_true", help="draw the nn.Dropout masks on the CPU generator in the order "
                    "tests/acdc_oracle_arm/oracle_acdc_short.py draws them (with --resume of its initial state and the same --seed, the two arms then "
                    "run the SAME trajectory up to fp32 round-off: profiles/r3_acdc_short_schedule.md)")
    ap.add_argument("--resume", default=None, help="a state_dict .pth (the reference's or ours: same keys) to start from")
    args = ap.parse_args(argv)
    if args.model is None:
        args.model = "unet" if args.loss in ("s2l", "pce_interintra") or args.loss.startswith("semi_") else "unet_cct"

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if not _lib.is_test_emulation():          # (the test-suite can run this loop against the host-emulation library on CPU tensors)
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
    random.seed(args.seed), np.random.seed(args.seed + rank), torch.manual_seed(args.seed)
    s2l, semi = args.loss == "s2l", args.loss.startswith("semi_")
    unlabeled = None
    if semi:     # train_mean_teacher_2D.py:106-115: the labeled patients with their dense masks, the unlabeled ones for their images
        train = BaseDataSets(base_dir=args.root_path, split="train", fold=args.fold, sup_type="label", labeled_type="labeled", cache=True)
        unlabeled = BaseDataSets(base_dir=args.root_path, split="train", fold=args.fold, sup_type="label", labeled_type="unlabeled", cache=True)
        if len(unlabeled) == 0:
            raise SystemExit("no unlabeled training slices for this fold under " + args.root_path)
    elif s2l:      # every slice of the fold's training patients, held in memory with its weight store (train_s2l.py:86-87)
        train = BaseDataSets_s2l(base_dir=args.root_path, fold=args.fold, class_num=args.num_classes)
    else:
        train = BaseDataSets(base_dir=args.root_path, split="train", fold=args.fold, sup_type=args.sup_type,
                             labeled_type=args.labeled_type, cache=True)
    val = BaseDataSets(base_dir=args.root_path, split="val", fold=args.fold, cache=True)
    if len(train) == 0:
        raise SystemExit("no training slices for this fold under " + args.root_path)
    if not s2l and args.sup_type == "random_walker":     # ..._pCE_random_walker_2D.py: dense pseudo labels from the scribbles, solved once
        import time as _time
        from wsl4mis_amd.dataloaders.random_walker import precompute
        t_rw = _time.time()
        info = precompute(train, n_class=args.num_classes)
        torch.cuda.synchronize()
        if rank == 0:
            print("random walker: %d slices labelled in %.2f s (%d zeroed by the class rule)"
                  % (info["slices"], _time.time() - t_rw, info["zeroed_by_class_rule"]), flush=True)
    aug = BatchRandomGenerator_s2l(args.patch_size) if s2l else BatchRandomGenerator(args.patch_size, device_cache=True)
    eng = TrainEngine(args.model, 1, args.num_classes, base_lr=args.base_lr, max_iterations=args.max_iterations,
                      loss=args.loss, thr_iter=args.thr_iter, thr_conf=args.thr_conf, s2l_alpha=args.alpha, period_iter=args.period_iter,
                      var_consistency=args.consistency, var_rampup=args.consistency_rampup, consistency=args.consistency,
                      consistency_rampup=args.consistency_rampup, ema_decay=args.ema_decay, teacher_update=args.teacher_update,
                      dan_lr=args.dan_lr, dan_ndf=args.dan_ndf, dan_pool=args.dan_pool)
    if args.resume:
        eng.model.load_state_dict(torch.load(args.resume, map_location="cpu"))
    if args.snapshot_path and rank == 0:
        os.makedirs(args.snapshot_path, exist_ok=True)
    torch.manual_seed(args.seed + 1000 * rank)          # dropout masks differ per rank; beta is shared (python RNG)
    order = np.random.RandomState(args.seed + rank)
    it, best, history = 0, 0.0, []
    validator = None
    if args.val_path == "device" and len(val):
        # The fold's volumes, uploaded once and kept across the passes.  Every rank keeps ALL of them although it validates only its share
        # (run(indices=range(rank, len(val), world)) below): the indices then are the dataset's own on every rank, and the cost is small --
        # a fold of ACDC is about 110 MB of fp32 images + uint8 labels on the device, read from files the dataset caches anyway.
        validator = val_2D.VolumeValidator([val[i] for i in range(len(val))], args.num_classes, args.patch_size)
    log = [] if (args.curve_json and rank == 0) else None
    import time
    t_start = time.time()
    last = args.stop_iterations if 0 < args.stop_iterations < args.max_iterations else args.max_iterations
    half = args.batch_size // 2
    if semi and (half < 2 or len(train) < 2):
        raise SystemExit("--loss semi_*: needs --batch_size >= 4 (two loaders of batch_size // 2 >= 2 slices: BatchNorm) and at least two "
                         "labeled slices; got batch_size %d, %d labeled slices" % (args.batch_size, len(train)))

    def labeled_batches():      # cycle(trainloader_labeled), reshuffled on every pass (a pass always yields: checked above)
        while True:
            pl = order.permutation(len(train))
            for b in range(0, len(pl), half):
                if len(pl[b:b + half]) >= 2:
                    yield pl[b:b + half]

    def batches():
        """index batches of one epoch: (labeled or whole-batch indices, unlabeled indices or None)"""
        if semi:                # zip(cycle(labeled), unlabeled): an epoch is one pass over the unlabeled slices
            perm = order.permutation(len(unlabeled))
            for b in range(0, len(perm), half):
                yield next(lab_iter), perm[b:b + half]
        else:
            perm = order.permutation(len(train))
            for b in range(0, len(perm), args.batch_size):
                yield perm[b:b + args.batch_size], None

    def train_step(idx, idx_u):
        if semi:
            image_u, _ = aug([unlabeled[int(i)] for i in idx_u])
            image, label = aug([train[int(i)] for i in idx])
            eng.step(image, label, unlabeled=image_u)
            return
        weight = None
        if s2l:
            image, _, label, weight = aug([train[int(i)] for i in idx])
        else:
            image, label = aug([train[int(i)] for i in idx])
        if args.oracle_stream:
            from wsl4mis_amd.networks.unet import _DROP, _FT
            n, (ph, pw) = len(idx), args.patch_size
            em = [(torch.rand((n, _FT[l], ph >> l, pw >> l)) >= _DROP[l]).to(torch.uint8).cuda() for l in range(5)]
            eng.model.set_dropout_masks(em, None)
        eng.step(image, label, random.random() + 1e-10, weight=weight)
        if args.oracle_stream:
            eng.model.set_dropout_masks(None, None)

    lab_iter = labeled_batches() if semi else None
    while it < last:
        for idx, idx_u in batches():
            if len(idx) < 2 or (idx_u is not None and len(idx_u) < 2):      # BatchNorm needs more than one slice
                continue
            train_step(idx, idx_u)
            it += 1
            if s2l and eng.ensemble_due():              # train_s2l.py:214-243; every rank refreshes its own full store
                eng.update_ensemble(train, mode=args.ensemble_mode, patch_size=tuple(args.patch_size))
            if rank == 0 and (it % args.log_every == 0 or it == 1):
                o = eng.losses()
                history.append((it, o["loss"]))
                if log is not None:
                    log.append(dict(o, iteration=it, lr=eng.lr))
                if not args.quiet:
                    print("iteration %d : " % it + ", ".join(f"{k} {v:.4f}" for k, v in o.items()), flush=True)
            if len(val) and it % args.val_every == 0:
                # every rank validates its share of the volumes, then one all-reduce of the sums: nobody sits blocked in the next
                # step's gradient all-reduce while rank 0 works through the whole set.  Parameters are bit-identical on all ranks
                # (all-reduced gradients); the BatchNorm running statistics are NOT -- every rank saw other batches -- so rank 0's
                # buffers are broadcast first (what DistributedDataParallel(broadcast_buffers=True) does before every forward):
                # the Dice that is reported and written into the checkpoint's file name then belongs to the state_dict rank 0
                # saves
                if world > 1:
                    dist.broadcast(eng.model._buf_arena, src=0)
                    dist.broadcast(eng.model._nbt, src=0)
                volume_fn = val_2D.test_single_volume_cct if args.model == "unet_cct" else val_2D.test_single_volume
                acc = np.zeros(2 * (args.num_classes - 1) + 1)
                if validator is not None:
                    per_volume = validator.run(eng.model, first_output=args.model == "unet_cct", with_hd95=not args.no_hd95,
                                               indices=range(rank, len(val), world))
                else:
                    per_volume = [np.array(volume_fn(val[i]["image"], val[i]["label"], eng.model, args.num_classes, args.patch_size,
                                                     with_hd95=not args.no_hd95), dtype=np.float64) for i in range(rank, len(val), world)]
                for m in per_volume:
                    acc += np.concatenate([m[:, 0], m[:, 1], [1.0]])
                if world > 1:
                    t = torch.from_numpy(acc).cuda()
                    dist.all_reduce(t)
                    acc = t.cpu().numpy()
                nc = args.num_classes - 1
                dice_c, hd_c = acc[:nc] / acc[-1], acc[nc:2 * nc] / acc[-1]
                mean_dice, mean_hd95 = float(dice_c.mean()), float(hd_c.mean())
                if rank == 0:
                    if mean_dice > best and args.snapshot_path:      # ..._ours_proposed.py:174-182
                        for name in ("iter_{}_dice_{}.pth".format(it, round(mean_dice, 4)), "{}_best_model.pth".format(args.model)):
                            torch.save(eng.model.state_dict(), os.path.join(args.snapshot_path, name))
                    print("iteration %d : mean_dice %.4f mean_hd95 %.3f (best %.4f)" % (it, mean_dice, mean_hd95, max(best, mean_dice)),
                          flush=True)
                    if log is not None:
                        log.append({"iteration": it, "mean_dice": mean_dice, "mean_hd95": mean_hd95,
                                    "dice_per_class": [float(x) for x in dice_c]})
                best = max(best, mean_dice)
                eng.model.train()
            if rank == 0 and args.snapshot_path and it % args.save_every == 0:     # ..._ours_proposed.py:194-198
                torch.save(eng.model.state_dict(), os.path.join(args.snapshot_path, "iter_" + str(it) + ".pth"))
            if it >= last:
                break
    if log is not None:
        import json
        with open(args.curve_json, "w") as fh:
            json.dump({"args": vars(args), "train_slices": len(train), "val_volumes": len(val), "best_mean_dice": best,
                       "wall_seconds": round(time.time() - t_start, 1), "world": world, "curve": log}, fh)
    return history


if __name__ == "__main__":
    main()
