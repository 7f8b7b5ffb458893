"""TEST INFRASTRUCTURE ONLY: CPU restatement of medpy 0.4.0 `metric.binary.__surface_distances` / `hd95` / `asd` WITH
`voxelspacing` (what code/test_2D_fully.py:74-80 calls), built from the scipy calls medpy itself makes.  oracle/metrics_ref.py
holds the unit-spacing form the in-training validation uses; medpy is not in the image.  Also the NumPy brute-force
evaluation of the exact expression `wsl_nearest_dist2_sp` is specified to compute (include/wsl_hip.h)."""
import numpy as np
from scipy.ndimage import _ni_support, binary_erosion, distance_transform_edt, generate_binary_structure


def surface_distances(result, reference, voxelspacing=None, connectivity=1):
    result, reference = np.atleast_1d(np.asarray(result).astype(bool)), np.atleast_1d(np.asarray(reference).astype(bool))
    if voxelspacing is not None:
        voxelspacing = _ni_support._normalize_sequence(voxelspacing, result.ndim)      # RuntimeError on a wrong length
        voxelspacing = np.asarray(voxelspacing, dtype=np.float64)
        if not voxelspacing.flags.contiguous:
            voxelspacing = voxelspacing.copy()
    footprint = generate_binary_structure(result.ndim, connectivity)
    if 0 == np.count_nonzero(result):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if 0 == np.count_nonzero(reference):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def hd95(result, reference, voxelspacing=None):
    hd1 = surface_distances(result, reference, voxelspacing)
    hd2 = surface_distances(reference, result, voxelspacing)
    return np.percentile(np.hstack((hd1, hd2)), 95)


def asd(result, reference, voxelspacing=None):
    return surface_distances(result, reference, voxelspacing).mean()


def dc(result, reference):
    result, reference = np.atleast_1d(np.asarray(result).astype(bool)), np.atleast_1d(np.asarray(reference).astype(bool))
    inter = np.count_nonzero(result & reference)
    s = np.count_nonzero(result) + np.count_nonzero(reference)
    try:
        return 2.0 * inter / float(s)
    except ZeroDivisionError:
        return 0.0


def calculate_metric_percase(pred, gt, spacing):              # code/test_2D_fully.py:74-80
    pred, gt = np.asarray(pred) > 0, np.asarray(gt) > 0
    dice = dc(pred, gt)
    a = asd(pred, gt, voxelspacing=spacing)
    h = hd95(pred, gt, voxelspacing=spacing)
    return dice, h, a


def nearest_dist2_sp(a_zyx, b_zyx, sz, sy, sx, chunk=512):
    """out[i] = min_j ((dz * sz)^2 + (dy * sy)^2) + (dx * sx)^2 in fp64: integer difference -> double, times the spacing (one
    rounding), squared (one rounding), added in the order z, y, x.  NumPy evaluates each ufunc on its own: nothing is fused."""
    a, b = np.asarray(a_zyx, dtype=np.int64), np.asarray(b_zyx, dtype=np.int64)
    out = np.empty(a.shape[0], np.float64)
    for i0 in range(0, a.shape[0], chunk):
        d = (a[i0:i0 + chunk, None, :] - b[None, :, :]).astype(np.float64)
        z, y, x = d[..., 0] * np.float64(sz), d[..., 1] * np.float64(sy), d[..., 2] * np.float64(sx)
        out[i0:i0 + chunk] = ((z * z + y * y) + x * x).min(axis=1)
    return out


def blobs(rng, shape, k):
    """a few anisotropic balls (same generator as tests/test_data.py::blobs)"""
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    v = np.zeros(shape, bool)
    for _ in range(k):
        c = [rng.uniform(0, n) for n in shape]
        r = rng.uniform(2, 0.35 * min(shape[1:]))
        v |= ((z - c[0]) * 2.5) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 < r * r
    return v
