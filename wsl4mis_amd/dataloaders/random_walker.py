"""Random-walker pseudo labels from scribbles (ref: code/dataloaders/acdc_pseudo_label_random_walker.py:9-26,
code/dataloaders/dataset_scribblevc.py:20-36, used by train_weakly_supervised_pCE_random_walker_2D.py with --sup_type random_walker).

The reference calls skimage.segmentation.random_walker(..., beta=100, mode='bf') -- a sparse direct solve per slice on the CPU --
inside `__getitem__`, on every read.  Here the same linear systems (include/wsl_hip.h, "random-walker pseudo labels") are solved on
the GPU for a whole batch of equal-sized slices by `wsl_random_walker` (csrc/wsl_rw.hip: Jacobi-preconditioned conjugate gradients,
one workgroup per slice and class), and because the labels are deterministic they are computed ONCE per slice: `precompute(dataset)`
fills the cache `BaseDataSets` serves `sup_type="random_walker"` from.  No CPU fallback: without the HIP library these calls raise.

One deliberate difference: a constant image (std == 0) gets the limit weights 1 + 1e-6; skimage divides by zero and returns NaN."""
from collections import defaultdict

import numpy as np
import torch

from .. import _lib
from .. import runtime as rt

MAX_BATCH_BYTES = 1 << 30       # workspace per solver call: larger groups of equal-sized slices are solved in chunks


def _solve(images, seeds, n_class, beta, tol, max_iter, want_prob):
    """-> (labels u8 [N,H,W], prob f32 [N,K,H,W] or None, iters i32 [N,K], resid f32 [N,K]), all on the device, no host sync"""
    dev = rt.device()
    img = torch.as_tensor(images, dtype=torch.float32).to(dev).contiguous()
    if torch.is_tensor(seeds):
        sd = seeds.to(dev)
        sd = sd if sd.dtype == torch.uint8 else sd.clamp(0, 255).to(torch.uint8)
    else:                                                    # (the scribble is uint16 on disk)
        sd = torch.from_numpy(np.ascontiguousarray(np.clip(np.asarray(seeds), 0, 255).astype(np.uint8))).to(dev)
    sd = sd.contiguous()
    if img.dim() != 3 or sd.shape != img.shape:
        raise ValueError(f"random_walker_labels: images {tuple(img.shape)} and seeds {tuple(sd.shape)} must be equal [N, H, W] shapes")
    N, H, W = (int(v) for v in img.shape)
    L = _lib.lib()
    nbytes = L.wsl_random_walker_ws_bytes(N, H, W, n_class)
    ws = rt.workspace("random_walker", nbytes)
    label = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    prob = torch.empty((N, n_class, H, W), dtype=torch.float32, device=dev) if want_prob else None
    iters = torch.empty((N, n_class), dtype=torch.int32, device=dev)
    resid = torch.empty((N, n_class), dtype=torch.float32, device=dev)
    _lib.check(L.wsl_random_walker(rt.ptr(img), rt.ptr(sd), rt.ptr(label), rt.ptr(prob), rt.ptr(iters), rt.ptr(resid), N, H, W, n_class,
                                   beta, tol, max_iter, rt.ptr(ws), nbytes, rt.stream()))
    return label, prob, iters, resid


def _check_converged(iters, resid, tol, first=0):
    """raises WslError naming the first slice one of whose systems ended above tol (one device-to-host copy)"""
    r, it = resid.cpu().numpy(), iters.cpu().numpy()
    bad = np.argwhere(~(r <= tol))
    if bad.size:
        n, k = (int(v) for v in bad[0])
        raise _lib.WslError(f"random_walker_labels: slice {first + n}, class {k}: relative residual {r[n, k]:.3e} > tol {tol:.1e} after "
                            f"{it[n, k]} iterations ({len(set(bad[:, 0].tolist()))} slices did not converge; raise max_iter)")
    return it


def random_walker_labels(images, seeds, n_class=4, beta=100.0, tol=1e-5, max_iter=10000, return_prob=False):
    """images [N, H, W] float in [0, 1], seeds [N, H, W] integer (classes 0 .. n_class-1, n_class = unlabelled): tensors on any device
    or arrays.  Returns the dense labels [N, H, W] uint8 on the device (all zeros for a slice whose seeds lack a foreground class), and
    with return_prob the probabilities [N, n_class, H, W] float32 as well.  Raises WslError naming the slice if any system ends above
    `tol`."""
    label, prob, iters, resid = _solve(images, seeds, int(n_class), float(beta), float(tol), int(max_iter), return_prob)
    _check_converged(iters, resid, tol)
    return (label, prob) if return_prob else label


def _generator(data, seed, n_class, beta):
    seed = np.asarray(seed)
    lab = random_walker_labels(np.asarray(data, dtype=np.float32)[None], seed[None], n_class=n_class, beta=beta)
    return lab[0].cpu().numpy().astype(seed.dtype)


def pseudo_label_generator_acdc(data, seed):
    """ref: acdc_pseudo_label_random_walker.py:9-26 -- numpy in, numpy out (the seed's dtype): 4 classes, 4 = unlabelled"""
    return _generator(data, seed, 4, 100.0)


def pseudo_label_generator_prostate(data, seed, beta=100):
    """ref: dataset_scribblevc.py:20-36 -- the same rule with 3 classes, 3 = unlabelled"""
    return _generator(data, seed, 3, float(beta))


def precompute(dataset, n_class=4, beta=100.0, tol=1e-5, max_iter=10000):
    """One pass over a BaseDataSets(split="train", sup_type="random_walker"), like TrainEngine.update_ensemble over a Scribble2Label
    dataset: slices are grouped by shape, each group is solved in batches, and the labels go into the dataset's pseudo-label cache,
    which `__getitem__` then serves.  Files that carry a `random_walker` dataset of their own are left to it.  Returns a dict with the
    slice count, the iteration counts of the solved systems and the number of slices the class rule zeroed."""
    todo = defaultdict(list)
    for case in dataset.sample_list:
        if case in dataset._rw_cache:
            continue
        arrays = dataset._rw_inputs(case)
        if arrays is None:                                   # the file has its own labels
            continue
        image, scribble = arrays
        todo[tuple(image.shape)].append((case, image, scribble))
    iters_all, n_done, n_zero = [], 0, 0
    for (h, w), group in todo.items():
        per = max(1, int(MAX_BATCH_BYTES // max(1, _lib.lib().wsl_random_walker_ws_bytes(1, h, w, n_class))))
        for b in range(0, len(group), per):
            part = group[b:b + per]
            seeds = np.stack([np.clip(s, 0, 255).astype(np.uint8) for _, _, s in part])
            label, _, iters, resid = _solve(np.stack([np.asarray(i, dtype=np.float32) for _, i, _ in part]), seeds, n_class, beta, tol,
                                            max_iter, False)
            it = _check_converged(iters, resid, tol, first=n_done)
            lab = label.cpu().numpy()
            for j, (case, _, s) in enumerate(part):
                dataset._rw_cache[case] = lab[j].astype(s.dtype)
            solved = np.array([all(k in s for k in range(1, n_class)) for s in seeds])      # the class rule
            n_zero += int((~solved).sum())
            iters_all += it[solved].reshape(-1).tolist()
            n_done += len(part)
    return {"slices": n_done, "zeroed_by_class_rule": n_zero, "iterations": iters_all}
