"""Minimal NIfTI-1 reader / writer for the offline test stage (ref: code/test_2D_fully.py:104-123).

The reference reads the voxel spacing of `<case>.nii.gz` with SimpleITK (`ReadImage(...).GetSpacing()`) and writes the
prediction, image and ground truth of every test volume as float32 NIfTI files that carry the source's geometry
(`GetImageFromArray` + `CopyInformation` + `WriteImage`).  nibabel, SimpleITK and medpy are not in the image, so this module
does exactly that subset with `struct` + `gzip`, in the spirit of `h5lite`:

    s = spacing_xyz(path)                                   # pixdim[1:4] = sitk's GetSpacing()
    write_volume(out, array_zyx, like=path)                 # float32, geometry of `path`
    write_volume(out, array_zyx, spacing_xyz=(1.5, 1.5, 10))
    array_zyx = read_volume(path)

Single-file NIfTI-1 (`n+1`), plain or gzip-compressed (recognised by its first two bytes, not by its name), either byte
order.  NIfTI-2, Analyze / `ni1` header-image pairs and scaled integer data raise `NiiError` instead of guessing.  Format
reference: the public nifti1.h (348-byte header; field offsets as in `_FIELDS` below)."""
import gzip
import struct

import numpy as np


class NiiError(Exception):
    pass


HDR = 348
# geometry the reference's CopyInformation carries over: (offset, struct format) of pixdim[8], xyzt_units, qform_code + sform_code,
# quatern_b/c/d + qoffset_x/y/z, srow_x/y/z
_GEOMETRY = ((76, "8f"), (123, "B"), (252, "2h"), (256, "6f"), (280, "12f"))
_DTYPES = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2", 768: "u4"}


def _open(path):
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def _read(fh, n, path, what):
    try:
        b = fh.read(n)
    except (EOFError, OSError, gzip.BadGzipFile) as e:
        raise NiiError(f"{path}: truncated or damaged while reading the {what} ({e})")
    if len(b) != n:
        raise NiiError(f"{path}: truncated: {len(b)} of {n} bytes of the {what}")
    return b


def _parse(raw, path):
    if struct.unpack("<i", raw[:4])[0] == HDR:
        e = "<"
    elif struct.unpack(">i", raw[:4])[0] == HDR:
        e = ">"
    else:
        raise NiiError(f"{path}: not a NIfTI-1 header (sizeof_hdr is neither 348 nor its byte swap; NIfTI-2 is not read)")
    magic = raw[344:348]
    if magic != b"n+1\0":
        raise NiiError(f"{path}: magic {magic!r}: only single-file NIfTI-1 ('n+1') is read (no Analyze / 'ni1' pairs)")
    u = lambda fmt, off: struct.unpack_from(e + fmt, raw, off)
    h = {"byteorder": e, "raw": bytes(raw), "magic": magic,
         "dim": list(u("8h", 40)), "datatype": u("h", 70)[0], "bitpix": u("h", 72)[0], "pixdim": list(u("8f", 76)),
         "vox_offset": u("f", 108)[0], "scl_slope": u("f", 112)[0], "scl_inter": u("f", 116)[0], "xyzt_units": u("B", 123)[0],
         "qform_code": u("h", 252)[0], "sform_code": u("h", 254)[0], "quatern": list(u("3f", 256)), "qoffset": list(u("3f", 268)),
         "srow": [list(u("4f", 280 + 16 * r)) for r in range(3)]}
    if not 1 <= h["dim"][0] <= 7:
        raise NiiError(f"{path}: dim[0] = {h['dim'][0]}")
    return h


def _sizes(dim):
    """dim[1 : 1 + dim[0]] without its trailing singleton axes"""
    s = list(dim[1:1 + dim[0]])
    while len(s) > 1 and s[-1] == 1:
        s.pop()
    return s


def read_header(path):
    """the header of a .nii / .nii.gz file as a dict: dim[8], pixdim[8], datatype, bitpix, vox_offset, scl_slope / scl_inter,
    qform_code / sform_code, quatern, qoffset, srow (3 x 4), byteorder ('<' or '>') and `raw`, the 348 header bytes"""
    with _open(path) as fh:
        return _parse(_read(fh, HDR, path, "header"), path)


def spacing_xyz(path):
    """pixdim[1:4]: what SimpleITK's Image.GetSpacing() returns for the file (x, y, z)"""
    return tuple(float(v) for v in read_header(path)["pixdim"][1:4])


def read_volume(path):
    """the voxel data in numpy's order: dim reversed ([z, y, x] for a 3-D file), in the file's data type"""
    with _open(path) as fh:
        h = _parse(_read(fh, HDR, path, "header"), path)
        if h["datatype"] not in _DTYPES:
            raise NiiError(f"{path}: datatype {h['datatype']} is not read")
        if h["scl_slope"] not in (0.0, 1.0) or (h["scl_slope"] == 1.0 and h["scl_inter"] != 0.0):
            raise NiiError(f"{path}: scaled data (scl_slope {h['scl_slope']}, scl_inter {h['scl_inter']}) is not read")
        shape = tuple(reversed(h["dim"][1:1 + h["dim"][0]]))
        if any(n <= 0 for n in shape):
            raise NiiError(f"{path}: dim {h['dim']}")
        off = int(h["vox_offset"])
        if off < HDR + 4:
            raise NiiError(f"{path}: vox_offset {h['vox_offset']}")
        _read(fh, off - HDR, path, "extension")
        dt = np.dtype(h["byteorder"] + _DTYPES[h["datatype"]])
        n = int(np.prod(shape))
        data = _read(fh, n * dt.itemsize, path, "voxel data")
    return np.frombuffer(data, dt, n).reshape(shape).astype(dt.newbyteorder("="))


def write_volume(path, array_zyx, like=None, spacing_xyz=None):
    """Write `array_zyx` as float32 single-file NIfTI-1 (gzip when `path` ends in .gz): dim = the reversed array shape, data =
    the array's C-order bytes (sitk.GetImageFromArray's convention).  like: a file (or a read_header dict) whose geometry
    -- pixdim, units, qform / sform codes, quaternion, offsets, srow -- is carried over, the reference's CopyInformation; it must
    have the same sizes (trailing singleton axes aside).  Otherwise a plain header with pixdim[1:4] = spacing_xyz (default
    1, 1, 1) and no qform / sform."""
    a = np.ascontiguousarray(array_zyx, dtype="<f4")
    if not 1 <= a.ndim <= 7:
        raise NiiError(f"cannot write a {a.ndim}-D array")
    dim = [a.ndim] + list(reversed(a.shape)) + [1] * (7 - a.ndim)
    raw = bytearray(HDR)
    struct.pack_into("<i", raw, 0, HDR)
    struct.pack_into("<8h", raw, 40, *dim)
    struct.pack_into("<hh", raw, 70, 16, 32)                     # datatype float32, bitpix
    struct.pack_into("<f", raw, 108, float(HDR + 4))             # vox_offset: header + the empty 4-byte extension flag
    struct.pack_into("<f", raw, 112, 1.0)                        # scl_slope (scl_inter 0): unscaled
    raw[344:348] = b"n+1\0"
    if like is not None:
        if spacing_xyz is not None:
            raise NiiError("give `like` or `spacing_xyz`, not both")
        h = like if isinstance(like, dict) else read_header(like)
        if _sizes(h["dim"]) != _sizes(dim):                      # (a 3-D volume stored with dim[0] = 4 and a trailing 1 is the same grid)
            raise NiiError(f"like= has dim {h['dim']}, the array needs {dim} (CopyInformation needs equal sizes)")
        for off, fmt in _GEOMETRY:
            struct.pack_into("<" + fmt, raw, off, *struct.unpack_from(h["byteorder"] + fmt, h["raw"], off))
    else:
        sp = [float(v) for v in (spacing_xyz if spacing_xyz is not None else (1.0,) * min(a.ndim, 3))]
        if len(sp) != min(a.ndim, 3) or not all(np.isfinite(v) and v > 0 for v in sp):
            raise NiiError(f"spacing_xyz {spacing_xyz!r} does not fit a {a.ndim}-D array")
        struct.pack_into("<8f", raw, 76, 1.0, *(sp + [1.0] * (7 - len(sp))))
        raw[123] = 2                                             # xyzt_units: millimetres
    blob = bytes(raw) + b"\0\0\0\0" + a.tobytes()
    if str(path).endswith(".gz"):
        with open(path, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:     # reproducible bytes
            gz.write(blob)
    else:
        with open(path, "wb") as fh:
            fh.write(blob)
