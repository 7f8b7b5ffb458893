"""In-training validation of the reference (ref: code/val_2D.py:18-50 test_single_volume, :90-124
test_single_volume_cct): per-slice zoom to the patch size -> net in eval mode -> argmax over softmax -> zoom back, then
per-class metrics over the volume.  The forward runs on the HIP path; the zoom (scipy, order 0, like the reference) is
host-side glue.  medpy is not available offline: Dice is computed here, and HD95 follows medpy 0.4.0
`metric.binary.hd95` (surface = object minus its 6-neighbourhood erosion; both directed sets of nearest-surface
distances; 95th percentile with numpy's linear rule) with the two heavy pieces on the device (`wsl_surface_u8`,
`wsl_nearest_dist2`: exact integer squared distances) and `torch.nonzero` / `torch.sort` as plumbing.  With a
`voxelspacing` (the offline test stage, test_2D_fully.py: distances in millimetres) the nearest-surface search is
`wsl_nearest_dist2_sp` in fp64; `asd_percase` is medpy's directed `asd`.
Opt-in, the slice loop itself runs on the device (`predict_volume_device`, `VolumeValidator`, `on_device=True`: both zooms, the argmax
and the Dice counts in csrc/wsl_val.hip), with equal label maps and Dice; the host loop stays the default."""
import numpy as np
import torch
from scipy.ndimage import zoom

from . import runtime as rt


def dice_percase(pred, gt):
    """binary Dice of one class, medpy.metric.binary.dc semantics (ref: val_2D.py:7-15: 0 when nothing is predicted)."""
    pred, gt = pred.astype(bool), gt.astype(bool)
    if pred.sum() == 0:
        return 0.0
    inter = np.count_nonzero(pred & gt)
    denom = np.count_nonzero(pred) + np.count_nonzero(gt)
    return 2.0 * inter / denom if denom else 0.0


def _mask_u8(vol):
    """a binary array (numpy, or a tensor already on the device) as a contiguous uint8 device tensor"""
    if isinstance(vol, torch.Tensor):
        if vol.device != rt.device():
            raise rt._lib.WslError(f"mask lives on {vol.device}, expected {rt.device()}")
        return (vol != 0).to(torch.uint8).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(vol).astype(bool), dtype=np.uint8)).to(rt.device())


def _surface_points(vol_bool):
    v = _mask_u8(vol_bool)
    if v.dim() not in (2, 3):
        raise NotImplementedError(f"hd95 of a {v.dim()}-D array is not built (2-D masks and [D,H,W] volumes are)")
    depth = 0 if v.dim() == 2 else v.shape[0]          # D = 0: a 2-D array -> 4-neighbourhood erosion, like medpy
    if v.dim() == 2:
        v = v[None]
    border = torch.empty_like(v)
    rt.call("wsl_surface_u8", rt.ptr(v), rt.ptr(border), depth, v.shape[1], v.shape[2], rt.stream())
    return torch.nonzero(border).contiguous()          # [n, 3] int64 (z, y, x)


def _spacing(voxelspacing, ndim):
    """scipy.ndimage's _normalize_sequence, which medpy applies first: a scalar counts for every axis, a sequence must have
    one entry per axis (RuntimeError otherwise).  None stays None: the unit-spacing integer path."""
    if voxelspacing is None:
        return None
    if isinstance(voxelspacing, str) or not hasattr(voxelspacing, "__iter__") or np.ndim(voxelspacing) == 0:
        return (float(voxelspacing),) * ndim
    sp = tuple(float(v) for v in voxelspacing)
    if len(sp) != ndim:
        raise RuntimeError("sequence argument must have length equal to input rank")
    return sp


def _surfaces(pred, gt, voxelspacing):
    """medpy's __surface_distances up to the distance transform, in its order: spacing normalised, emptiness checked, both surfaces"""
    nd = pred.dim() if isinstance(pred, torch.Tensor) else np.ndim(pred)
    sp = _spacing(voxelspacing, nd)
    pred, gt = _mask_u8(pred), _mask_u8(gt)
    if not bool(pred.any()):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not bool(gt.any()):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return _surface_points(pred), _surface_points(gt), sp


def _nearest(p, q, sp):
    """fp64 distance from every point of p to the nearest point of q ([n, 3] surface lists); sp: None or one spacing per array axis"""
    if sp is None:                                      # exact integer squared distances
        out = torch.empty((p.shape[0],), dtype=torch.int64, device=p.device)
        rt.call("wsl_nearest_dist2", rt.ptr(p), p.shape[0], rt.ptr(q), q.shape[0], rt.ptr(out), rt.stream())
        return torch.sqrt(out.double())
    sz, sy, sx = sp if len(sp) == 3 else (1.0,) + tuple(sp)      # a 2-D array: z = 0 for every point
    out = torch.empty((p.shape[0],), dtype=torch.float64, device=p.device)
    rt.call("wsl_nearest_dist2_sp", rt.ptr(p), p.shape[0], rt.ptr(q), q.shape[0], sz, sy, sx, rt.ptr(out), rt.stream())
    return torch.sqrt(out)


def surface_distances(pred, gt, voxelspacing=None):
    """medpy 0.4.0 `__surface_distances(result, reference, voxelspacing)`: for every surface voxel of `pred` (C order) the
    distance to the nearest surface voxel of `gt`, as an fp64 tensor on the device.  voxelspacing: None (unit voxels, the exact
    integer kernel), a scalar or one value per array axis (`wsl_nearest_dist2_sp`: the expression scipy's
    distance_transform_edt(sampling=...) evaluates, so the values equal medpy's bit for bit unless scipy picked the other of two
    near-tied features).  Masks are numpy arrays or tensors already on the device."""
    a, b, sp = _surfaces(pred, gt, voxelspacing)
    return _nearest(a, b, sp)


def _percentile95(dist):
    dist, _ = torch.sort(dist)
    n = dist.numel()
    pos = 0.95 * (n - 1)                                # numpy.percentile(..., 95), method 'linear'
    lo = int(np.floor(pos))
    hi = min(lo + 1, n - 1)
    t = pos - lo
    lo_v, hi_v = float(dist[lo]), float(dist[hi])
    diff = hi_v - lo_v
    return hi_v - diff * (1 - t) if t >= 0.5 else lo_v + diff * t


def hd95_percase(pred, gt, voxelspacing=None):
    """medpy.metric.binary.hd95(result, reference, voxelspacing): None = isotropic unit voxels (what val_2D.py:12 passes)."""
    a, b, sp = _surfaces(pred, gt, voxelspacing)
    return _percentile95(torch.cat([_nearest(a, b, sp), _nearest(b, a, sp)]))


def asd_percase(pred, gt, voxelspacing=None):
    """medpy.metric.binary.asd(result, reference, voxelspacing): the mean of the DIRECTED pred -> gt surface distances (not assd)."""
    return float(surface_distances(pred, gt, voxelspacing).mean())


def hd95_asd_percase(pred, gt, voxelspacing=None):
    """(hd95, asd) of one mask pair from one evaluation of the surfaces and of the pred -> gt distances (the reference's
    calculate_metric_percase, test_2D_fully.py:74-80, computes them once per metric)."""
    a, b, sp = _surfaces(pred, gt, voxelspacing)
    d_ab = _nearest(a, b, sp)
    return _percentile95(torch.cat([d_ab, _nearest(b, a, sp)])), float(d_ab.mean())


def metric_percase(pred, gt, with_hd95=True):
    """ref: val_2D.py:7-15 calculate_metric_percase -> (dice, hd95), (0, 0) when nothing is predicted."""
    pred, gt = np.asarray(pred) > 0, np.asarray(gt) > 0
    if pred.sum() > 0:
        return dice_percase(pred, gt), (hd95_percase(pred, gt) if with_hd95 else 0.0)
    return 0, 0


def _predict_volume(image, net, patch_size, first_output, slices_per_forward=16):
    """The reference feeds one slice per forward (val_2D.py:22-37, 94-111); the eval forward is per-sample (BatchNorm uses its
    running statistics -- bit-equality of a batch and its parts is tested), so the zoomed slices go through in batches."""
    image = np.asarray(image, dtype=np.float32)
    prediction = np.zeros(image.shape, dtype=np.uint8)
    net.eval()
    x, y = image.shape[1:]
    for i0 in range(0, image.shape[0], slices_per_forward):
        inp = np.stack([zoom(slc, (patch_size[0] / x, patch_size[1] / y), order=0) for slc in image[i0:i0 + slices_per_forward]])
        t = torch.from_numpy(np.ascontiguousarray(inp, dtype=np.float32))[:, None].to(rt.device())
        with torch.no_grad():
            out = net(t)
            if first_output and isinstance(out, (tuple, list)):
                out = out[0]                      # val_2D.py:104: only the main branch is evaluated
            lab = torch.argmax(out, dim=1).cpu().numpy().astype(np.uint8)     # argmax(softmax(z)) == argmax(z)
        for k in range(lab.shape[0]):
            prediction[i0 + k] = zoom(lab[k], (x / patch_size[0], y / patch_size[1]), order=0)
    return prediction


def _squeeze(v):
    a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return a[0] if a.ndim == 4 else a            # DataLoader batch dimension of the reference (val_2D.py:19-20)


# ------------------------------------------------------------------------------------------------ the same on the device
# wsl_val_zoom_in -> eval forward -> wsl_val_labelmap (csrc/wsl_val.hip): both zooms are scipy's order-0 rule to the last pixel, the
# argmax is the first maximum, the Dice counts are integers -- label maps and Dice EQUAL the host path's; nothing crosses PCIe per
# slice.  The host path above stays as it is (and stays the default of every caller).

def _device_volume(vol, dtype, what):
    """a [D,h,w] volume (numpy or a host tensor: uploaded; a tensor already on the device: used in place when it has the dtype) as a
    contiguous device tensor"""
    if isinstance(vol, torch.Tensor):
        if vol.device != rt.device() and vol.device.type != "cpu":
            raise rt._lib.WslError(f"{what} lives on {vol.device}, expected {rt.device()}")
        t = vol.detach().to(dtype).to(rt.device()).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(vol), dtype={torch.float32: np.float32, torch.uint8: np.uint8}[dtype]))
        t = t.to(rt.device())
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]                                  # DataLoader batch dimension of the reference (val_2D.py:19-20)
    if t.dim() != 3:
        raise NotImplementedError(f"{what}: 2-D slices of a [D,H,W] volume are the built path, got {tuple(t.shape)}")
    return t


def _zoomed_logits(net, first_output, patch_size, jobs):
    """`jobs` = [(image volume, pred volume, label volume or None, slice index, group)]: their slices zoomed to the patch size and sent
    through ONE forward -> logits [n, C, Ho, Wo]"""
    n, (Ho, Wo) = len(jobs), patch_size
    src = (rt._lib.WslValSrc * n)()
    for k, (img, _, _, d, _) in enumerate(jobs):
        h, w = img.shape[1:]
        src[k].img, src[k].h, src[k].w = img.data_ptr() + 4 * d * h * w, h, w
    x = torch.empty((n, 1, Ho, Wo), dtype=torch.float32, device=rt.device())
    rt.call("wsl_val_zoom_in", src, n, rt.ptr(x), Ho, Wo, rt.stream())
    with torch.no_grad():
        out = net(x)
        if first_output and isinstance(out, (tuple, list)):
            out = out[0]                          # val_2D.py:104: only the main branch is evaluated
    return rt.f32c(out, "logits")


def _label_maps(z, jobs, counts=None):
    """the label bytes of the jobs' slices from their logits, into the pred volumes; counts [groups, C, 3] int64: the Dice counts, added"""
    n = len(jobs)
    dst = (rt._lib.WslValDst * n)()
    for k, (img, pred, lab, d, group) in enumerate(jobs):
        h, w = img.shape[1:]
        dst[k].pred, dst[k].h, dst[k].w, dst[k].group = pred.data_ptr() + d * h * w, h, w, group
        dst[k].label = None if lab is None else lab.data_ptr() + d * h * w
    rt.call("wsl_val_labelmap", rt.ptr(z), dst, n, z.shape[1], z.shape[2], z.shape[3], rt.ptr(counts),
            0 if counts is None else counts.shape[0], rt.stream())


def predict_volume_device(image, net, patch_size, first_output, slices_per_forward=16):
    """`_predict_volume` without the host: -> uint8 device tensor [D,h,w], equal to it byte for byte at the same slices_per_forward.
    `image`: numpy (uploaded once) or a tensor already on the device (used in place).  Like `_predict_volume` it puts `net` into eval
    mode and LEAVES it there: a training loop calls `net.train()` afterwards."""
    img = _device_volume(image, torch.float32, "image")
    pred = torch.empty(tuple(img.shape), dtype=torch.uint8, device=rt.device())
    net.eval()
    for i0 in range(0, img.shape[0], slices_per_forward):
        jobs = [(img, pred, None, d, 0) for d in range(i0, min(i0 + slices_per_forward, img.shape[0]))]
        _label_maps(_zoomed_logits(net, first_output, tuple(patch_size), jobs), jobs)
    return pred


class VolumeValidator:
    """The validation set of a fold kept on the device across validation passes: `volumes` is an iterable of
    {"image": [D,h,w], "label": [D,h,w]} (what BaseDataSets(split="val") yields), uploaded once as fp32 / uint8.  run() packs the
    slices of all selected volumes into forwards of `slices_per_forward`, across volume boundaries (the eval forward is per-sample),
    and reads the Dice counts back ONCE per pass."""

    def __init__(self, volumes, classes, patch_size=(256, 256), slices_per_forward=64):
        self.classes, self.patch_size, self.slices_per_forward = int(classes), tuple(int(p) for p in patch_size), int(slices_per_forward)
        self.images = [_device_volume(v["image"], torch.float32, "image") for v in volumes]
        self.labels = [_device_volume(v["label"], torch.uint8, "label") for v in volumes]
        for a, b in zip(self.images, self.labels):
            if a.shape != b.shape:
                raise ValueError(f"image {tuple(a.shape)} and label {tuple(b.shape)} differ in shape")
        self._pred = {}

    def __len__(self):
        return len(self.images)

    def run(self, net, first_output=False, with_hd95=True, indices=None):
        """-> np.float64 [len(indices), classes - 1, 2] of (dice, hd95): `metric_percase` per volume and class 1 .. classes - 1.
        `indices`: the volumes of this pass (a data-parallel rank takes range(rank, len, world)); default all.
        Puts `net` into eval mode and LEAVES it there, as the host path does: a training loop calls `net.train()` afterwards."""
        idx = list(range(len(self.images))) if indices is None else [int(i) for i in indices]
        res = np.zeros((len(idx), self.classes - 1, 2), dtype=np.float64)
        self._pred = {}
        if not idx:
            return res
        net.eval()
        jobs = []
        for g, i in enumerate(idx):
            self._pred[i] = torch.empty(tuple(self.images[i].shape), dtype=torch.uint8, device=rt.device())
            jobs += [(self.images[i], self._pred[i], self.labels[i], d, g) for d in range(self.images[i].shape[0])]
        counts = None
        for j0 in range(0, len(jobs), self.slices_per_forward):
            part = jobs[j0:j0 + self.slices_per_forward]
            z = _zoomed_logits(net, first_output, self.patch_size, part)
            if counts is None:                    # (the logits say how many classes the net has)
                counts = torch.zeros((len(idx), z.shape[1], 3), dtype=torch.int64, device=rt.device())
            _label_maps(z, part, counts)
        cnt = counts.cpu().numpy()                # the pass's one read: [volume, class, (|pred|, |gt|, |pred & gt|)]
        for g, i in enumerate(idx):
            for c in range(1, self.classes):
                n_pred, n_gt, inter = (int(v) for v in cnt[g, c]) if c < cnt.shape[1] else (0, 0, 0)
                if n_pred == 0:
                    continue                      # metric_percase: (0, 0) when nothing is predicted
                res[g, c - 1, 0] = 2.0 * inter / (n_pred + n_gt)
                if with_hd95:                     # (raises medpy's RuntimeError when the ground truth is empty, as the host path)
                    res[g, c - 1, 1] = hd95_percase(self._pred[i] == c, self.labels[i] == c)
        return res

    def predictions(self):
        """{volume index: uint8 device tensor [D,h,w]} of the last pass"""
        return dict(self._pred)


def _metrics_on_device(image, label, net, classes, patch_size, with_hd95, first_output):
    v = VolumeValidator([{"image": image, "label": label}], classes, patch_size, slices_per_forward=16)
    return [(float(dice), float(hd95)) for dice, hd95 in v.run(net, first_output=first_output, with_hd95=with_hd95)[0]]


def test_single_volume(image, label, net, classes, patch_size=(256, 256), with_hd95=True, on_device=False):
    if on_device:
        return _metrics_on_device(image, label, net, classes, patch_size, with_hd95, first_output=False)
    image, label = _squeeze(image), _squeeze(label)
    if image.ndim != 3:
        raise NotImplementedError("2-D slices of a [D,H,W] volume are the built path (the reference's else-branch "
                                  "feeds a single image)")
    prediction = _predict_volume(image, net, patch_size, first_output=False)
    return [metric_percase(prediction == i, label == i, with_hd95) for i in range(1, classes)]


def test_single_volume_cct(image, label, net, classes, patch_size=(256, 256), with_hd95=True, on_device=False):
    if on_device:
        return _metrics_on_device(image, label, net, classes, patch_size, with_hd95, first_output=True)
    image, label = _squeeze(image), _squeeze(label)
    if image.ndim != 3:
        raise NotImplementedError("2-D slices of a [D,H,W] volume are the built path (val_2D.py:116 unpacks four "
                                  "outputs in its else-branch, which no 2-D net returns)")
    prediction = _predict_volume(image, net, patch_size, first_output=True)
    return [metric_percase(prediction == i, label == i, with_hd95) for i in range(1, classes)]


test_single_volume.__test__ = False        # (names kept from the reference; not pytest cases)
test_single_volume_cct.__test__ = False
