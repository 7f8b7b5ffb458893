"""Spacing-aware surface metrics of the offline test stage (ref: code/test_2D_fully.py:74-80: medpy's hd95 / asd with
voxelspacing): the `wsl_nearest_dist2_sp` kernel through the C ABI against the NumPy evaluation of its specified expression
(bit-equal), `val_2D.surface_distances / hd95_percase / asd_percase` against the scipy restatement of medpy
(tests/metrics_sp_ref.py), and the dependency-free NIfTI-1 reader / writer."""
import functools
import gzip
import struct

import numpy as np
import pytest

import metrics_sp_ref as M
from conftest import get_backend
from oracle import metrics_ref
from wsl4mis_amd import _lib


@pytest.fixture(params=[pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)])
def mode(request):
    from wsl4mis_amd import runtime
    _lib._reset_for_tests()
    runtime._ws_cache.clear()
    if request.param == "emul":
        _lib.use_library_for_tests(get_backend("emul").lib)
    yield request.param
    _lib._reset_for_tests()
    runtime._ws_cache.clear()


# ---------------------------------------------------------------------------------------------- kernel through the C ABI
WG, TILE = 256, 1024                    # workgroup size and LDS tile of nearest_d2_sp_kernel (csrc/wsl_data.hip: kThreads, kSpTile)
SPACINGS = [(1e-3, 1.0, 1e3), (7.3, 0.9, 1.1), (10.0, 1.5625, 1.5625), (1.0, 1.0, 1.0)]
# (na, nb): 1, the workgroup size +-1 and the tile +-1 on both sides; the last nb needs three tiles with a ragged last one
COUNTS = [(1, 1), (2, 3), (WG - 1, WG + 1), (WG, TILE - 1), (WG + 1, TILE), (TILE - 1, TILE + 1), (TILE, WG - 1), (TILE + 1, WG),
          (300, 2 * TILE + 513), (1, TILE + 1), (WG + 1, 1)]


def run_kernel(be, a, b, sp):
    da, db = be.arr(a, np.int64), be.arr(b, np.int64)
    out = be.arr(np.full(a.shape[0], -1.0), np.float64)
    be.call("wsl_nearest_dist2_sp", be.ptr(da), a.shape[0], be.ptr(db), b.shape[0], sp[0], sp[1], sp[2], be.ptr(out), be.stream)
    be.sync()
    return be.np(out)


def test_kernel_is_bit_equal_to_the_specified_expression(be):
    rng = np.random.default_rng(41)
    for k, (na, nb) in enumerate(COUNTS):
        hi = 4096 if k % 2 == 0 else 24                          # coordinates up to 4095 | a small box: many exact ties and zeros
        a, b = rng.integers(0, hi, (na, 3)), rng.integers(0, hi, (nb, 3))
        for sp in (SPACINGS[k % 4], SPACINGS[(k + 1) % 4]):
            got = run_kernel(be, a, b, sp)
            assert np.array_equal(got, M.nearest_dist2_sp(a, b, *sp)), (na, nb, sp)


def test_kernel_point_set_cases(be):
    rng = np.random.default_rng(43)
    b = rng.integers(0, 4096, (TILE + 7, 3))
    b[5] = (4095, 4095, 4095)
    b[6] = (0, 0, 0)
    for sp in SPACINGS[:2]:
        a = b[rng.permutation(b.shape[0])[:WG + 3]]              # a is a subset of b: exact zeros
        assert np.array_equal(run_kernel(be, a, b, sp), np.zeros(a.shape[0]))
        a2 = rng.integers(0, 4096, (70, 3))
        a2[0], a2[1] = (0, 0, 0), (4095, 4095, 4095)
        bd = np.concatenate([b, b[:40], b[-3:]])                 # duplicated points change nothing
        ref = M.nearest_dist2_sp(a2, b, *sp)
        assert np.array_equal(run_kernel(be, a2, bd, sp), ref)
        assert np.array_equal(run_kernel(be, np.concatenate([a2, a2[:9]]), b, sp), np.concatenate([ref, ref[:9]]))
        # the farthest pair of the coordinate range
        far = run_kernel(be, np.array([[0, 0, 0]]), np.array([[4095, 4095, 4095]]), sp)
        assert np.array_equal(far, M.nearest_dist2_sp([[0, 0, 0]], [[4095, 4095, 4095]], *sp))
    # 2-D point sets: z = 0 everywhere, any valid sz -- the z term is an exact zero
    a, b2 = rng.integers(0, 300, (WG + 9, 3)), rng.integers(0, 300, (TILE + 100, 3))
    a[:, 0] = 0
    b2[:, 0] = 0
    g1, g2 = run_kernel(be, a, b2, (1.0, 0.9, 1.1)), run_kernel(be, a, b2, (123.456, 0.9, 1.1))
    dy, dx = (a[:, None, 1] - b2[None, :, 1]).astype(np.float64) * 0.9, (a[:, None, 2] - b2[None, :, 2]).astype(np.float64) * 1.1
    assert np.array_equal(g1, (dy * dy + dx * dx).min(axis=1)) and np.array_equal(g1, g2)


def test_kernel_rejects_bad_arguments_and_writes_nothing(be):
    a, b = be.arr(np.zeros((4, 3)), np.int64), be.arr(np.ones((5, 3)), np.int64)
    out = be.arr(np.full(4, -1.0), np.float64)
    ok = (1.0, 1.0, 1.0)
    bad = [(0, 5, ok), (-1, 5, ok), (4, 0, ok), (4, -2, ok)]
    for v in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for ax in range(3):
            bad.append((4, 5, tuple(v if i == ax else 1.0 for i in range(3))))
    for na, nb, sp in bad:
        with pytest.raises(_lib.WslError):
            be.call("wsl_nearest_dist2_sp", be.ptr(a), na, be.ptr(b), nb, sp[0], sp[1], sp[2], be.ptr(out), be.stream)
    for args in ((None, be.ptr(b), be.ptr(out)), (be.ptr(a), None, be.ptr(out)), (be.ptr(a), be.ptr(b), None)):
        with pytest.raises(_lib.WslError):
            be.call("wsl_nearest_dist2_sp", args[0], 4, args[1], 5, 1.0, 1.0, 1.0, args[2], be.stream)
    be.sync()
    assert np.array_equal(be.np(out), np.full(4, -1.0))
    be.call("wsl_nearest_dist2_sp", be.ptr(a), 4, be.ptr(b), 5, 2.0, 3.0, 4.0, be.ptr(out), be.stream)      # and the good call works
    be.sync()
    assert np.array_equal(be.np(out), np.full(4, 29.0))


# ---------------------------------------------------------------------------------------------- metrics against medpy's algorithm
SP3 = [(10.0, 1.5625, 1.5625), (7.3, 0.9, 1.1), 1.25]             # ACDC-like, all three different, a scalar
SP2 = [(1.5625, 1.5625), (0.9, 1.1), 1.25]


@functools.lru_cache(maxsize=None)
def mask_cases():
    """(pred, gt, spacings) pairs and, per spacing, the restatement's (pred -> gt distances, hd95, asd) -- computed once"""
    rng = np.random.default_rng(17)
    cases = []
    for shape in ((6, 40, 48), (9, 64, 56), (1, 33, 47), (4, 30, 30)):
        gt, pred = M.blobs(rng, shape, 3), M.blobs(rng, shape, 3)
        if shape[0] == 4:
            pred = np.ones(shape, bool)                           # object touching every array face
        assert gt.any() and pred.any(), shape
        cases.append((pred, gt, SP3))
    gt2, pred2 = M.blobs(rng, (1, 48, 40), 3)[0], M.blobs(rng, (1, 48, 40), 3)[0]
    assert gt2.any() and pred2.any()
    cases.append((pred2, gt2, SP2))
    out = []
    for pred, gt, sps in cases:
        out.append((pred, gt, [(sp, M.surface_distances(pred, gt, sp), M.hd95(pred, gt, sp), M.asd(pred, gt, sp)) for sp in sps]))
    return out


def test_surface_distances_hd95_asd_match_medpy_with_spacing(mode):
    from wsl4mis_amd import val_2D
    n = 0
    for pred, gt, refs in mask_cases():
        for sp, d_ref, h_ref, a_ref in refs:
            d = val_2D.surface_distances(pred, gt, sp)
            assert str(d.dtype) == "torch.float64" and d.device == val_2D.rt.device()
            d = d.cpu().numpy()
            assert d.shape == d_ref.shape
            rel = np.max(np.abs(d - d_ref) / np.where(d_ref > 0, d_ref, 1.0))
            h, a = val_2D.hd95_percase(pred, gt, sp), val_2D.asd_percase(pred, gt, sp)
            print(f"shape {pred.shape} spacing {sp}: {d.size} distances, max rel diff {rel:.3e}, "
                  f"{int(np.count_nonzero(d != d_ref))} not bit-equal; hd95 {h!r} vs {h_ref!r}; asd {a!r} vs {a_ref!r}")
            assert np.all(np.abs(d - d_ref) <= 1e-12 * d_ref), (pred.shape, sp, rel)
            assert abs(h - h_ref) <= 1e-12 * max(1.0, h_ref), (pred.shape, sp, h, h_ref)
            assert abs(a - a_ref) <= 1e-10 * a_ref, (pred.shape, sp, a, a_ref)
            n += d.size
    assert n > 5000


def test_unit_spacing_path_is_unchanged_and_agrees_with_spacing_one(mode):
    from wsl4mis_amd import val_2D
    for pred, gt, _ in mask_cases():
        h_ref = metrics_ref.hd95(pred, gt)
        h = val_2D.hd95_percase(pred, gt)
        assert abs(h - h_ref) <= 1e-12 * max(1.0, h_ref), (pred.shape, h, h_ref)
        assert val_2D.metric_percase(pred, gt) == (val_2D.dice_percase(pred, gt), h)
        d, d_ref = val_2D.surface_distances(pred, gt).cpu().numpy(), metrics_ref._surface_distances(pred, gt)
        assert d.shape == d_ref.shape and np.all(np.abs(d - d_ref) <= 1e-12 * d_ref)     # (exact integers under the root on both sides)
        assert val_2D.hd95_percase(pred, gt, np.float64(1.0)) == val_2D.hd95_percase(pred, gt, np.array(1.0))     # scalars of any kind
        h1 = val_2D.hd95_percase(pred, gt, (1.0,) * pred.ndim)
        assert abs(h1 - h) <= 1e-12 * max(1.0, h), (pred.shape, h1, h)
        a_ref = metrics_ref._surface_distances(pred, gt).mean()
        assert abs(val_2D.asd_percase(pred, gt) - a_ref) <= 1e-10 * a_ref


def test_metric_error_cases(mode):
    from wsl4mis_amd import val_2D
    pred, gt, _ = mask_cases()[0]
    for fn in (val_2D.surface_distances, val_2D.hd95_percase, val_2D.asd_percase):
        with pytest.raises(RuntimeError, match="length equal to input rank"):
            fn(pred, gt, (1.0, 2.0))
        with pytest.raises(RuntimeError, match="length equal to input rank"):
            fn(pred[0], gt[0], (1.0, 2.0, 3.0))
        for sp in (None, (10.0, 1.5, 1.5)):
            with pytest.raises(RuntimeError, match="The first supplied array does not contain any binary object"):
                fn(np.zeros_like(pred), gt, sp)
            with pytest.raises(RuntimeError, match="The second supplied array does not contain any binary object"):
                fn(pred, np.zeros_like(gt), sp)
    with pytest.raises(RuntimeError, match="length equal to input rank"):
        M.surface_distances(pred, gt, (1.0, 2.0))                 # the restatement raises the same way


# ---------------------------------------------------------------------------------------------- niilite (plain CPU)
def test_niilite_round_trip_and_header_layout(tmp_path):
    from wsl4mis_amd.dataloaders import niilite
    rng = np.random.default_rng(5)
    vol = rng.standard_normal((5, 12, 9)).astype(np.float32)
    sp = (1.5625, 1.25, 10.0)                                    # exact in float32
    for name in ("v.nii", "v.nii.gz"):
        p = str(tmp_path / name)
        niilite.write_volume(p, vol, spacing_xyz=sp)
        h = niilite.read_header(p)
        assert h["dim"] == [3, 9, 12, 5, 1, 1, 1, 1] and tuple(h["pixdim"][1:4]) == sp and niilite.spacing_xyz(p) == sp
        assert h["datatype"] == 16 and len(h["raw"]) == 348
        got = niilite.read_volume(p)
        assert got.dtype == np.float32 and np.array_equal(got, vol)
        blob = (gzip.open(p, "rb") if name.endswith(".gz") else open(p, "rb")).read()
        assert open(p, "rb").read(2) == (b"\x1f\x8b" if name.endswith(".gz") else b"\x5c\x01")
        assert len(blob) == 352 + vol.nbytes and blob[352:] == vol.tobytes()          # C-order bytes of the [z, y, x] array
        assert struct.unpack_from("<i", blob, 0)[0] == 348
        assert struct.unpack_from("<h", blob, 70)[0] == 16 and struct.unpack_from("<h", blob, 72)[0] == 32
        assert struct.unpack_from("<f", blob, 108)[0] == 352.0
        assert blob[344:348] == b"n+1\0" and blob[348:352] == b"\0\0\0\0"
        assert struct.unpack_from("<8h", blob, 40) == (3, 9, 12, 5, 1, 1, 1, 1)
    niilite.write_volume(str(tmp_path / "u.nii"), np.arange(24, dtype=np.uint8).reshape(2, 3, 4))          # converted to float32
    assert np.array_equal(niilite.read_volume(str(tmp_path / "u.nii")), np.arange(24, dtype=np.float32).reshape(2, 3, 4))
    assert niilite.spacing_xyz(str(tmp_path / "u.nii")) == (1.0, 1.0, 1.0)


def big_endian_file(path, data_zyx, pixdim, srow):
    """a big-endian int16 single-file NIfTI-1 built field by field from the public layout (nifti1.h)"""
    raw = bytearray(348)
    struct.pack_into(">i", raw, 0, 348)
    struct.pack_into(">8h", raw, 40, 3, *reversed(data_zyx.shape), 1, 1, 1, 1)
    struct.pack_into(">hh", raw, 70, 4, 16)
    struct.pack_into(">8f", raw, 76, *pixdim)
    struct.pack_into(">f", raw, 108, 352.0)
    struct.pack_into(">ff", raw, 112, 1.0, 0.0)
    raw[123] = 10
    struct.pack_into(">hh", raw, 252, 1, 2)
    struct.pack_into(">6f", raw, 256, 0.0, 0.5, 0.25, -10.0, 20.0, 30.0)
    struct.pack_into(">12f", raw, 280, *[v for r in srow for v in r])
    raw[344:348] = b"n+1\0"
    with gzip.open(path, "wb") as fh:
        fh.write(bytes(raw) + b"\0\0\0\0" + data_zyx.astype(">i2").tobytes())


def test_niilite_big_endian_like_and_errors(tmp_path):
    from wsl4mis_amd.dataloaders import niilite
    data = (np.arange(4 * 6 * 5).reshape(4, 6, 5) - 50).astype(np.int16)
    pixdim = (-1.0, 1.40625, 1.5, 10.0, 1.0, 0.0, 0.0, 0.0)
    srow = [[-1.40625, 0.0, 0.0, 90.0], [0.0, 1.5, 0.0, -80.0], [0.0, 0.0, 10.0, 5.5]]
    src = str(tmp_path / "be.nii.gz")
    big_endian_file(src, data, pixdim, srow)
    h = niilite.read_header(src)
    assert h["byteorder"] == ">" and h["dim"] == [3, 5, 6, 4, 1, 1, 1, 1] and h["datatype"] == 4 and h["bitpix"] == 16
    assert tuple(h["pixdim"]) == pixdim and niilite.spacing_xyz(src) == (1.40625, 1.5, 10.0)
    assert h["srow"] == srow and (h["qform_code"], h["sform_code"]) == (1, 2) and h["vox_offset"] == 352.0
    got = niilite.read_volume(src)
    assert got.dtype == np.int16 and got.dtype.isnative and np.array_equal(got, data)
    # like=: the geometry travels (the reference's CopyInformation), the data are ours, little-endian float32
    out = str(tmp_path / "pred.nii.gz")
    pred = np.random.default_rng(1).integers(0, 4, data.shape).astype(np.uint8)
    niilite.write_volume(out, pred, like=src)
    g = niilite.read_header(out)
    assert g["byteorder"] == "<" and g["datatype"] == 16 and g["dim"] == h["dim"]
    assert g["srow"] == srow and tuple(g["pixdim"]) == pixdim and (g["qform_code"], g["sform_code"]) == (1, 2)
    assert g["quatern"] == [0.0, 0.5, 0.25] and g["qoffset"] == [-10.0, 20.0, 30.0] and g["xyzt_units"] == 10
    assert np.array_equal(niilite.read_volume(out), pred.astype(np.float32))
    niilite.write_volume(str(tmp_path / "pred2.nii"), pred, like=h)                      # a header dict works too
    assert niilite.read_header(str(tmp_path / "pred2.nii"))["srow"] == srow
    with pytest.raises(niilite.NiiError, match="dim"):
        niilite.write_volume(out, pred[:, :, :4], like=src)
    # a 3-D source stored as 4-D with a trailing 1 (common) is the same grid: CopyInformation accepts it, so does like=
    raw4 = bytearray(h["raw"])
    struct.pack_into(">8h", raw4, 40, 4, 5, 6, 4, 1, 1, 1, 1)
    src4 = str(tmp_path / "be4.nii")
    open(src4, "wb").write(bytes(raw4) + b"\0\0\0\0" + data.astype(">i2").tobytes())
    assert niilite.read_volume(src4).shape == (1, 4, 6, 5)
    niilite.write_volume(str(tmp_path / "pred4.nii"), pred, like=src4)
    g4 = niilite.read_header(str(tmp_path / "pred4.nii"))
    assert g4["dim"] == [3, 5, 6, 4, 1, 1, 1, 1] and g4["srow"] == srow and tuple(g4["pixdim"]) == pixdim
    # truncated files: inside the header, inside the data, inside the gzip stream
    blob = gzip.open(src, "rb").read()
    for n, what in ((200, "header"), (352 + 17, "voxel data")):
        p = str(tmp_path / f"cut{n}.nii")
        open(p, "wb").write(blob[:n])
        with pytest.raises(niilite.NiiError, match="truncated"):
            niilite.read_volume(p)
    with pytest.raises(niilite.NiiError, match="truncated"):
        niilite.read_header(str(tmp_path / "cut200.nii"))
    cut = str(tmp_path / "cut.nii.gz")
    open(cut, "wb").write(open(src, "rb").read()[:60])
    with pytest.raises(niilite.NiiError, match="truncated"):
        niilite.read_volume(cut)
    bad = bytearray(blob)
    bad[344:348] = b"ni1\0"
    open(str(tmp_path / "pair.nii"), "wb").write(bytes(bad))
    with pytest.raises(niilite.NiiError, match="single-file"):
        niilite.read_header(str(tmp_path / "pair.nii"))
    open(str(tmp_path / "junk.nii"), "wb").write(b"\1" * 400)
    with pytest.raises(niilite.NiiError, match="not a NIfTI-1"):
        niilite.read_header(str(tmp_path / "junk.nii"))
