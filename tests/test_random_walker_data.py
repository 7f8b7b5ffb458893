"""The random-walker data path: the reference-named generators, BaseDataSets(sup_type="random_walker") with its per-case cache and
random_walker.precompute, the other sup_types untouched, and one ce_dice training step on such a batch (gpu).

The fixture's four slice files lack class 1, so the class rule zeroes all of them: test_committed_slices_go_through_the_hook runs the
dataset on them as they are.  For labels that are actually solved the dataset is also run on a temporary ACDC tree whose extra slice
"files" are 48 x 40 crops of the committed volume's slices 2 and 3 (all four classes present).  The project has no HDF5 writer, so
those crops are served from memory by a stand-in for h5lite.File installed with monkeypatch; every other path, the one committed
slice file in that tree included, goes to the real reader."""
import os

import numpy as np
import pytest
import torch

import rw_ref
from conftest import GOLDEN, get_backend
from wsl4mis_amd.dataloaders import h5lite

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


def crops():
    """{file name: {'image', 'label', 'scribble'}}: 48 x 40 crops of slices 2 and 3 of the committed volume that keep all four classes
    (two of one shape, so precompute batches them), named like slice files of patient041 (a training patient of fold1)"""
    img, scr = rw_ref.volume()
    from wsl4mis_amd.dataloaders import h5lite as h
    with h.File(rw_ref.VOLUME) as f:
        lab = f["label"][:]
    out = {}
    for z in (2, 3):
        found = None
        for y0 in range(0, 224 - 48 + 1, 4):
            for x0 in range(0, 154 - 40 + 1, 4):
                s = scr[z, y0:y0 + 48, x0:x0 + 40]
                if all(k in s for k in range(4)):
                    found = (y0, x0)
                    break
            if found:
                break
        assert found, f"no 48 x 40 crop of slice {z} holds all four classes"
        y0, x0 = found
        out[f"patient041_frame11_slice_{z}.h5"] = {"image": img[z, y0:y0 + 48, x0:x0 + 40].copy(), "label": lab[z, y0:y0 + 48, x0:x0 + 40].copy(),
                                                  "scribble": scr[z, y0:y0 + 48, x0:x0 + 40].astype(np.uint16)}
    return out


class _MemFile:
    """what BaseDataSets uses of h5lite.File, over in-memory arrays; real paths go to the real reader"""
    store = {}

    def __new__(cls, path, mode="r"):
        name = os.path.basename(path)
        if name not in cls.store:
            return _REAL_FILE(path, mode)
        self = object.__new__(cls)
        self.d = cls.store[name]
        return self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def __contains__(self, k):
        return k in self.d

    def __getitem__(self, k):
        return self.d[k]                                    # KeyError for a missing dataset, like the file reader


_REAL_FILE = h5lite.File


@pytest.fixture
def tree(monkeypatch, tmp_path):
    """an ACDC tree whose training slices are the crops (served from memory) plus one committed slice file (read from disk)"""
    d = crops()
    sl = tmp_path / "ACDC_training_slices"
    sl.mkdir()
    (tmp_path / "ACDC_training_volumes").mkdir()
    for name in d:
        (sl / name).write_bytes(b"")                         # listed by os.listdir; content comes from _MemFile
    real = sorted(f for f in os.listdir(os.path.join(ACDC, "ACDC_training_slices")) if f.startswith("patient030"))[0]
    os.symlink(os.path.join(ACDC, "ACDC_training_slices", real), sl / real)
    _MemFile.store = d
    monkeypatch.setattr(h5lite, "File", _MemFile)
    return str(tmp_path), d, real


def test_generators_keep_the_dtype_and_agree_with_the_batched_call(mode):
    from wsl4mis_amd.dataloaders.random_walker import pseudo_label_generator_acdc, pseudo_label_generator_prostate, random_walker_labels
    img, seed = rw_ref.synthetic()[(24, 20)]
    want = random_walker_labels(img, seed).cpu().numpy()
    assert want.max() == 3
    for dt in (np.uint8, np.uint16, np.int64):
        got = pseudo_label_generator_acdc(img[0], seed[0].astype(dt))
        assert isinstance(got, np.ndarray) and got.dtype == dt and np.array_equal(got, want[0])
    s3 = np.minimum(seed[0], 3)                              # K = 3: 3 is the unlabelled mark, so the class-3 seeds are dropped as well
    got = pseudo_label_generator_prostate(img[0], s3, beta=100)
    assert np.array_equal(got, random_walker_labels(img[:1], s3[None], n_class=3).cpu().numpy()[0]) and got.max() == 2
    no3 = seed[0].copy()
    no3[no3 == 3] = 4
    assert not pseudo_label_generator_acdc(img[0], no3).any()               # the class rule


def test_dataset_serves_dense_labels_computed_once(mode, tree):
    from wsl4mis_amd.dataloaders import random_walker as rw
    from wsl4mis_amd.dataloaders.dataset import BaseDataSets
    root, d, real = tree
    calls = []
    orig = rw.pseudo_label_generator_acdc

    def counted(data, seed):
        calls.append(1)
        return orig(data, seed)

    rw.pseudo_label_generator_acdc = counted
    try:
        ds = BaseDataSets(root, split="train", sup_type="random_walker", labeled_type="all", fold="fold1")
        assert sorted(ds.sample_list) == sorted(list(d) + [real])
        first = [ds[i] for i in range(len(ds))]
        n_calls = len(calls)
        assert n_calls == len(ds)
        second = [ds[i] for i in range(len(ds))]
        assert len(calls) == n_calls                                           # served from the cache
    finally:
        rw.pseudo_label_generator_acdc = orig
    for a, b in zip(first, second):
        assert np.array_equal(a["label"], b["label"]) and a["case"] == b["case"] and a["source"][2] == "random_walker"
    for s in first:
        lab = s["label"]
        assert lab.shape == s["image"].shape and set(np.unique(lab).tolist()) <= {0, 1, 2, 3}
        if s["case"] in d:
            assert lab.dtype == np.uint16 and set(np.unique(lab).tolist()) == {0, 1, 2, 3}          # dense: no 4 left
            ref = rw_ref.cached(("crop", s["case"]), d[s["case"]]["image"][None], d[s["case"]]["scribble"][None].astype(np.uint8), 4)[0]
            sure = ref["gap"] >= 1e-2
            assert np.array_equal(lab[sure], ref["label"][sure])
        else:
            assert not lab.any()                                               # the committed slice lacks class 1
    # precompute on a fresh dataset: the same labels, no per-read solve afterwards
    ds2 = BaseDataSets(root, split="train", sup_type="random_walker", labeled_type="all", fold="fold1", cache=True)
    info = rw.precompute(ds2)
    assert info["slices"] == len(ds2) and info["zeroed_by_class_rule"] == 1 and len(info["iterations"]) == 4 * len(d)
    rw.pseudo_label_generator_acdc = None                                      # a solve in __getitem__ would raise
    try:
        third = [ds2[i] for i in range(len(ds2))]
    finally:
        rw.pseudo_label_generator_acdc = orig
    for a, b in zip(first, third):
        assert a["case"] == b["case"] and np.array_equal(a["label"], b["label"]) and a["label"].dtype == b["label"].dtype
    assert rw.precompute(ds2)["slices"] == 0                                   # nothing left to do


def test_a_file_with_its_own_random_walker_dataset_is_read(mode, tree):
    from wsl4mis_amd.dataloaders import random_walker as rw
    from wsl4mis_amd.dataloaders.dataset import BaseDataSets
    root, d, real = tree
    name = sorted(d)[0]
    own = np.full(d[name]["image"].shape, 2, np.uint8)
    d[name]["random_walker"] = own
    ds = BaseDataSets(root, split="train", sup_type="random_walker", labeled_type="all", fold="fold1")
    assert rw.precompute(ds)["slices"] == len(ds) - 1
    assert np.array_equal(ds[ds.sample_list.index(name)]["label"], own)


@pytest.mark.parametrize("sup", ["scribble", "label"])
def test_other_sup_types_are_untouched(sup):
    """byte-identical to the arrays read directly with h5lite, and the missing-key behaviour stays a KeyError"""
    from wsl4mis_amd.dataloaders.dataset import BaseDataSets
    ds = BaseDataSets(ACDC, split="train", sup_type=sup, labeled_type="all", fold="fold3")
    assert len(ds) == 4
    for i in range(len(ds)):
        s = ds[i]
        with h5lite.File(os.path.join(ACDC, "ACDC_training_slices", s["case"])) as f:
            img, lab = f["image"][:], f[sup][:]
        assert s["image"].dtype == img.dtype and s["label"].dtype == lab.dtype
        assert s["image"].tobytes() == img.tobytes() and s["label"].tobytes() == lab.tobytes()
        assert s["source"][2] == sup and set(s) == {"image", "label", "idx", "case", "source"}
    with pytest.raises(KeyError):
        BaseDataSets(ACDC, split="train", sup_type="no_such_labels", labeled_type="all", fold="fold3")[0]


def test_committed_slices_go_through_the_hook(mode):
    """the fixture tree itself: sup_type="random_walker" no longer ends in a KeyError; all four slices lack class 1 -> zeros"""
    from wsl4mis_amd.dataloaders.dataset import BaseDataSets
    ds = BaseDataSets(ACDC, split="train", sup_type="random_walker", labeled_type="all", fold="fold3")
    assert len(ds) == 4
    from wsl4mis_amd.dataloaders.random_walker import precompute
    for i in range(len(ds)):
        s = ds[i]
        assert s["label"].shape == s["image"].shape and s["label"].dtype == np.uint16 and not s["label"].any()
        assert ds[i]["label"] is s["label"]                                    # the second read: the cached array
    ds2 = BaseDataSets(ACDC, split="train", sup_type="random_walker", labeled_type="all", fold="fold3")
    assert precompute(ds2) == {"slices": 4, "zeroed_by_class_rule": 4, "iterations": []}
    assert all(np.array_equal(ds2[i]["label"], ds[i]["label"]) and ds2[i]["label"].dtype == np.uint16 for i in range(4))


@pytest.mark.gpu
def test_one_ce_dice_step_on_a_random_walker_batch_gpu(tree):
    from wsl4mis_amd import _lib, runtime
    from wsl4mis_amd.dataloaders import random_walker as rw
    from wsl4mis_amd.dataloaders.dataset import BaseDataSets, BatchRandomGenerator
    from wsl4mis_amd.engine import TrainEngine
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    root, d, real = tree
    ds = BaseDataSets(root, split="train", sup_type="random_walker", labeled_type="all", fold="fold1", cache=True)
    rw.precompute(ds)
    image, label = BatchRandomGenerator((64, 64))([ds[i] for i in range(len(ds))])
    assert int(label.max()) == 3
    eng = TrainEngine("unet", 1, 4, loss="ce_dice")
    eng.step(image, label, 0.5)
    torch.cuda.synchronize()
    loss = eng.losses()["loss"]
    assert np.isfinite(loss) and loss > 0
