"""On-device validation at the module level (wsl4mis_amd/val_2D.py: predict_volume_device, VolumeValidator, on_device=True) against
the host path of the same module (scipy zoom per slice, numpy masks), which stays the reference: label maps and Dice EQUAL, HD95 within
the bound the validation tests use (1e-12 * max(1, ref))."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from conftest import get_backend
from detinit import det_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACDC = os.path.join(ROOT, "tests", "golden", "acdc")
P16 = (16, 16)


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


def load_det(model, seed):
    sd = model.state_dict()
    vals = det_state({k: tuple(v.shape) for k, v in sd.items()}, seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})


def det_net(net_type, seed=5):
    from wsl4mis_amd.networks.net_factory import net_factory
    m = net_factory(net_type, 1, 4)
    load_det(m, seed)
    return m


def host(t):
    return t.detach().cpu().numpy()


def check_metrics(got, ref, what):
    """Dice ==; |HD95 - ref| <= 1e-12 * max(1, ref), the bound of tests/test_offline_test_stage.py::check_row (HD95 here is 0 or >= 1)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    print(what, "device", got.tolist(), "host", ref.tolist())
    assert got.shape == ref.shape, what
    assert np.array_equal(got[..., 0], ref[..., 0]), what
    assert (np.abs(got[..., 1] - ref[..., 1]) <= 1e-12 * np.maximum(1.0, ref[..., 1])).all(), what


def fill_happens_at_the_sizes_used_here():
    """32 -> 16 columns and 16 -> 30 rows end in scipy's fill value, 20 x 24 <-> 16 x 16 do not: the volumes below cover both"""
    ones = np.ones((30, 32), np.float32)
    zi = zoom(ones, (16 / 30, 16 / 32), order=0)
    assert (zi[:, -1] == 0).all() and (zi[:, :-1] == 1).all()
    zb = zoom(np.ones(P16, np.uint8), (30 / 16, 32 / 16), order=0)
    assert (zb[-1] == 0).all() and (zb[:-1] == 1).all()
    assert (zoom(np.ones((20, 24), np.float32), (16 / 20, 16 / 24), order=0) == 1).all()
    assert (zoom(np.ones(P16, np.uint8), (20 / 16, 24 / 16), order=0) == 1).all()


@pytest.mark.parametrize("net_type,first", [("unet", False), ("unet_cct", True)])
def test_device_path_equals_host_path(mode, net_type, first):
    from wsl4mis_amd import runtime as rt
    from wsl4mis_amd import val_2D
    fill_happens_at_the_sizes_used_here()
    rng = np.random.default_rng(3)
    net = det_net(net_type)
    seen = set()
    for shape in ((3, 30, 32), (2, 20, 24)):
        vol = rng.random(shape).astype(np.float32)
        ref = val_2D._predict_volume(vol, net, P16, first_output=first, slices_per_forward=2)
        got = val_2D.predict_volume_device(vol, net, P16, first_output=first, slices_per_forward=2)
        assert got.dtype == torch.uint8 and got.device == rt.device() and tuple(got.shape) == shape
        assert np.array_equal(host(got), ref), (net_type, shape)
        seen |= set(np.unique(ref).tolist())
        if shape == (3, 30, 32):
            assert (ref[:, -1] == 0).all()                           # the filled last row of the zoom back
    assert len(seen) >= 2                                            # the weights give more than one class: the comparison sees the argmax


class Stub(torch.nn.Module):
    """intensity -> logits: class c wins where the pixel is nearest to 0.1 + 0.2 c, so both paths see prescribed predictions"""

    def __init__(self, n_class=4):
        super().__init__()
        self.n_class = n_class

    def forward(self, x):
        centres = torch.arange(self.n_class, dtype=torch.float32, device=x.device) * 0.2 + 0.1
        return -(x - centres.view(1, -1, 1, 1)).abs()


def blobs(shape, classes, shift):
    """label volume with one box per class; `shift` moves the boxes (image and ground truth overlap in part)"""
    D, h, w = shape
    lab = np.zeros(shape, np.uint8)
    for c in classes:                                                # a class always sits in the same quadrant
        k = c - 1
        y0, x0 = 1 + shift + (k % 2) * (h // 2), 1 + shift + (k // 2) * (w // 2)
        lab[:, y0:y0 + h // 2 - 3, x0:x0 + w // 2 - 3] = c
    return lab


def stub_volume(shape, img_classes, lab_classes):
    return {"image": (0.1 + 0.2 * blobs(shape, img_classes, 0)).astype(np.float32), "label": blobs(shape, lab_classes, 2)}


def host_metrics(v, net, classes, with_hd95=True, spf=4):
    from wsl4mis_amd import val_2D
    pred = val_2D._predict_volume(v["image"], net, P16, first_output=False, slices_per_forward=spf)
    return pred, [val_2D.metric_percase(pred == c, v["label"] == c, with_hd95) for c in range(1, classes)]


def test_volume_validator_with_a_stub_net(mode):
    from wsl4mis_amd import val_2D
    net = Stub()
    vols = [stub_volume((3, 30, 32), (1, 2, 3), (1, 2, 3)), stub_volume((2, 20, 24), (1, 2), (1, 2, 3)),
            stub_volume((4, 26, 22), (1, 2, 3), (1, 2, 3))]
    ref_pred, ref = zip(*[host_metrics(v, net, 4) for v in vols])
    ref = np.array(ref, np.float64)
    assert all(r[0] > 0 and r[1] > 0 for i in (0, 2) for r in ref[i]) and ref[1, 0, 0] > 0      # values, not only the empty case
    val = val_2D.VolumeValidator(vols, 4, patch_size=P16, slices_per_forward=4)                 # 9 slices: both batches straddle volumes
    assert len(val) == 3
    got = val.run(net)
    assert got.dtype == np.float64 and got.shape == (3, 3, 2)
    check_metrics(got, ref, f"stub ({mode})")
    assert tuple(got[1, 2]) == (0.0, 0.0) and not (ref_pred[1] == 3).any()                      # class 3 is never predicted in volume 1
    from wsl4mis_amd import runtime as rt
    on_dev = torch.from_numpy(vols[0]["image"]).to(rt.device())      # a tensor already on the device is used in place
    assert np.array_equal(host(val_2D.predict_volume_device(on_dev, net, P16, first_output=False, slices_per_forward=2)), ref_pred[0])
    preds = val.predictions()
    assert sorted(preds) == [0, 1, 2] and all(np.array_equal(host(preds[i]), ref_pred[i]) for i in range(3))
    # Dice only: the same Dice, HD95 0
    d_only = val.run(net, with_hd95=False)
    assert np.array_equal(d_only[..., 0], ref[..., 0]) and (d_only[..., 1] == 0).all()
    # a rank's share and the rest reproduce the full run
    a, b = val.run(net, indices=[0, 2]), val.run(net, indices=[1])
    assert sorted(val.predictions()) == [1]
    assert np.array_equal(np.stack([a[0], b[0], a[1]]), got)
    assert val.run(net, indices=[]).shape == (0, 3, 2)


def test_prediction_without_ground_truth(mode):
    """class 2 is predicted, the ground truth has none: medpy's RuntimeError with HD95 (the host path's, word for word), Dice 0.0 without"""
    from wsl4mis_amd import val_2D
    net = Stub()
    vols = [stub_volume((2, 20, 24), (1, 2, 3), (1, 2, 3)), stub_volume((3, 26, 22), (1, 2, 3), (1, 3))]
    with pytest.raises(RuntimeError) as host_err:
        host_metrics(vols[1], net, 4)
    val = val_2D.VolumeValidator(vols, 4, patch_size=P16, slices_per_forward=4)
    with pytest.raises(RuntimeError) as dev_err:
        val.run(net)
    assert str(dev_err.value) == str(host_err.value) and "second supplied array" in str(dev_err.value)
    got = val.run(net, with_hd95=False)
    ref = np.array([host_metrics(v, net, 4, with_hd95=False)[1] for v in vols], np.float64)
    assert np.array_equal(got, ref) and got[1, 1, 0] == 0.0 and (got[1, [0, 2], 0] > 0).all()


def test_packing_across_volumes_equals_per_volume_prediction(mode):
    """rests on the per-sample eval forward (tests/test_fullsize.py pins it at the benchmark size): a slice's logits do not depend on
    what else is in the batch"""
    from wsl4mis_amd import val_2D
    rng = np.random.default_rng(9)
    net = det_net("unet")
    shapes = ((2, 30, 32), (1, 20, 24), (2, 26, 22))                 # forwards of 2: [A0 A1] [B0 C0] [C1]
    vols = [{"image": rng.random(s).astype(np.float32), "label": rng.integers(0, 4, s).astype(np.uint8)} for s in shapes]
    val = val_2D.VolumeValidator(vols, 4, patch_size=P16, slices_per_forward=2)
    val.run(net, with_hd95=False)
    preds = val.predictions()
    for i, v in enumerate(vols):
        alone = val_2D.predict_volume_device(v["image"], net, P16, first_output=False, slices_per_forward=2)
        assert torch.equal(preds[i], alone), i


@pytest.mark.parametrize("fn,net_type", [("test_single_volume", "unet"), ("test_single_volume_cct", "unet_cct")])
def test_on_device_keyword_equals_the_default_call(mode, fn, net_type):
    from wsl4mis_amd import val_2D
    rng = np.random.default_rng(21)
    net = det_net(net_type)
    vol = rng.random((2, 20, 24)).astype(np.float32)
    lab = rng.integers(0, 4, vol.shape).astype(np.uint8)
    f = getattr(val_2D, fn)
    ref = f(vol, lab, net, 4, patch_size=P16)
    got = f(vol, lab, net, 4, patch_size=P16, on_device=True)
    assert isinstance(got, list) and len(got) == 3 and all(len(g) == 2 for g in got)
    check_metrics(got, ref, f"{fn} ({mode})")
    stub = Stub()                                                    # the DataLoader's batch dimension and host tensors, as the trainers pass them
    sv = stub_volume((2, 20, 24), (1, 2, 3), (1, 2, 3))
    got4 = f(torch.from_numpy(sv["image"])[None], torch.from_numpy(sv["label"])[None], stub, 4, patch_size=P16, on_device=True)
    check_metrics(got4, f(sv["image"], sv["label"], stub, 4, patch_size=P16), f"{fn}, batch dimension ({mode})")


@pytest.mark.gpu
def test_committed_acdc_volume_on_the_device(capsys):
    """the committed ACDC volume (6 x 224 x 154) at patch 256 x 256: label maps and metrics of the device path equal the host path's;
    the example trainer validates through --val_path device"""
    from wsl4mis_amd import _lib, runtime, val_2D
    from wsl4mis_amd.dataloaders import dataset
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    net = det_net("unet_cct", seed=7)
    v = dataset.BaseDataSets(base_dir=ACDC, split="val", fold="fold3")[0]
    vol, lab = v["image"], v["label"]
    assert vol.shape == (6, 224, 154)
    ref_pred = val_2D._predict_volume(vol, net, (256, 256), first_output=True)
    got_pred = val_2D.predict_volume_device(vol, net, (256, 256), first_output=True)
    assert np.array_equal(host(got_pred), ref_pred)
    ref = val_2D.test_single_volume_cct(vol, lab, net, 4, with_hd95=False)
    got = val_2D.test_single_volume_cct(vol, lab, net, 4, with_hd95=False, on_device=True)
    check_metrics(got, ref, "ACDC volume, Dice")
    val = val_2D.VolumeValidator([v], 4)
    try:
        ref_hd = val_2D.test_single_volume_cct(vol, lab, net, 4)
    except RuntimeError as e:                                        # an untrained net may predict a class the volume lacks
        with pytest.raises(RuntimeError) as ei:
            val.run(net, first_output=True)
        assert str(ei.value) == str(e)
    else:
        check_metrics(val.run(net, first_output=True)[0], ref_hd, "ACDC volume, Dice and HD95")
    assert np.array_equal(host(val.predictions()[0]), ref_pred)
    capsys.readouterr()
    spec = importlib.util.spec_from_file_location("train_acdc_val", os.path.join(ROOT, "examples", "train_acdc_scribble.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--root_path", ACDC, "--fold", "fold3", "--labeled_type", "unlabeled", "--batch_size", "3", "--patch_size", "64", "64",
              "--max_iterations", "20", "--val_every", "20", "--val_path", "device"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "mean_dice" in ln]
    assert len(lines) == 1, lines
    assert np.isfinite(float(lines[0].split("mean_dice")[1].split()[0]))
