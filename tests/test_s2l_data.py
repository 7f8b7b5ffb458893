"""Scribble2Label data path on the ACDC fixture files (tests/golden/acdc): BaseDataSets_s2l (fold selection, keys, dtypes,
zero-initialised device stores), the two generators, and the example trainer with --loss s2l across one update and the threshold."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, get_backend

ACDC = os.path.join(GOLDEN, "acdc")


@pytest.fixture(params=[pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)])
def mode(request):
    from wsl4mis_amd import _lib, runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    if request.param == "emul":
        _lib.use_library_for_tests(get_backend("emul").lib)
    yield request.param
    _lib._reset_for_tests()
    runtime._ws_cache.clear()


def test_dataset_fold_selection_keys_and_stores(mode):
    from wsl4mis_amd import runtime
    from wsl4mis_amd.dataloaders.dataset_s2l import BaseDataSets_s2l
    # the fixture holds slices of patients 010, 030, 094 (two): a fold trains on every patient outside its block of 20
    want = {"fold1": ["patient030", "patient094", "patient094"], "fold2": ["patient010", "patient094", "patient094"],
            "fold3": ["patient010", "patient030", "patient094", "patient094"], "fold5": ["patient010", "patient030"]}
    for fold, pats in want.items():
        ds = BaseDataSets_s2l(base_dir=ACDC, fold=fold)
        assert [f.split("_")[0] for f in ds.sample_list] == pats and len(ds) == len(pats), fold
    ds = BaseDataSets_s2l(base_dir=ACDC, fold="fold3")
    for idx in range(len(ds)):
        e = ds.images[idx]
        assert set(e) == {"id", "image", "mask", "scribble", "weight"} and e["id"] == ds.sample_list[idx]
        h, w = e["mask"].shape
        assert e["image"].shape == e["scribble"].shape == (h, w) and e["image"].dtype == np.float32
        assert e["scribble"].dtype == np.uint16 and e["mask"].dtype == np.uint8      # as on disk (ref: np.array(h5f[...]))
        assert set(np.unique(e["scribble"]).tolist()) <= {0, 1, 2, 3, 4}
        wt = e["weight"]                                                             # (extension) a device tensor
        assert torch.is_tensor(wt) and wt.device == runtime.device() and wt.dtype == torch.float32 and tuple(wt.shape) == (h, w, 4)
        assert float(wt.abs().sum()) == 0.0
    raw = ds[1]
    assert set(raw) == {"image", "mask", "scribble", "weight", "staged", "id"} and raw["weight"] is ds.images[1]["weight"]
    with pytest.raises(ValueError):
        BaseDataSets_s2l(base_dir=ACDC, fold="fold9")


def test_generators_single_and_batched_agree(mode):
    from wsl4mis_amd.dataloaders.dataset_s2l import BaseDataSets_s2l, BatchRandomGenerator_s2l, RandomGenerator_s2l
    one = BaseDataSets_s2l(base_dir=ACDC, fold="fold3", transform=RandomGenerator_s2l((48, 40)))
    raw = BaseDataSets_s2l(base_dir=ACDC, fold="fold3")
    rng = np.random.default_rng(4)
    for idx in range(len(one)):
        w = torch.from_numpy(rng.random(tuple(one.images[idx]["weight"].shape)).astype(np.float32))
        one.images[idx]["weight"].copy_(w)
        raw.images[idx]["weight"].copy_(w)
    ops = set()
    for seed in range(6):
        random.seed(seed), np.random.seed(seed)
        singles = [one[i] for i in range(len(one))]
        random.seed(seed), np.random.seed(seed)
        img, mask, scr, wt = BatchRandomGenerator_s2l((48, 40))([raw[i] for i in range(len(raw))])
        assert tuple(img.shape) == (4, 1, 48, 40) and tuple(wt.shape) == (4, 48, 40, 4) and scr.dtype == mask.dtype == torch.uint8
        for i, s in enumerate(singles):
            assert s["id"] == raw.sample_list[i] and tuple(s["image"].shape) == (1, 48, 40)
            assert torch.equal(s["image"], img[i]) and torch.equal(s["mask"], mask[i]) and torch.equal(s["scribble"], scr[i])
            assert torch.equal(s["weight"], wt[i])
        ops.add(float(wt.sum()))
    assert len(ops) > 3                                   # the seeds drew different transforms


@pytest.mark.gpu
def test_example_trainer_runs_s2l_across_an_update_and_the_threshold(tmp_path):
    """--loss s2l end to end on the fixture files: pCE steps, an update of the stores, then steps with the pseudo-label term.
    No emulator leg: the example is a device program (torch.cuda.set_device, .cuda() tensors, nccl), so it cannot run against the host
    emulation library; the same loop on CPU tensors is test_s2l_engine.py::test_engine_follows_the_reference_recipe[emul]."""
    import importlib.util
    import json
    from wsl4mis_amd import _lib, runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_acdc_s2l", os.path.join(root, "examples", "train_acdc_scribble.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    curve = os.path.join(str(tmp_path), "curve.json")
    hist = mod.main(["--root_path", ACDC, "--fold", "fold3", "--loss", "s2l", "--max_iterations", "12", "--batch_size", "2",
                     "--patch_size", "64", "64", "--val_every", "1000", "--log_every", "1", "--period_iter", "3", "--thr_iter", "6",
                     "--thr_conf", "0.3", "--alpha", "0.6", "--quiet", "--curve_json", curve])
    assert len(hist) == 12 and all(np.isfinite(l) for _, l in hist)
    log = json.load(open(curve))["curve"]
    assert all(r["n_u"] == 0 and r["ce_u"] == 0 for r in log[:6])                       # iter_num < thr_iter: pCE alone
    assert all(r["n_u"] > 0 and r["ce_u"] > 0 and abs(r["loss"] - (r["ce"] + 0.5 * r["ce_u"])) < 1e-5 for r in log[6:])
