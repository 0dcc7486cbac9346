"""Hot-path helpers of the reference's utils/image_tools.py, restated without SimpleITK.

Only the five functions that define the sliding-window semantics are provided:
  image_partition_by_fixed_size  (image_tools.py:163-218)   pure index arithmetic, host side
  add_image_region / add_image_value (image_tools.py:435-469) -> device kernels, see core/seg_infer.py
  convert_image_to_tensor / convert_tensor_to_image (image_tools.py:274-326)
plus the geometry functions around the patch path, on the device:
  resample / resample_spacing                         (image_tools.py:329-377)  trilinear / NN (and cubic B-spline, not in
                                                      the reference), ITK inside test and padding
  pick_largest_connected_component / remove_small_connected_component (image_tools.py:380-432)  26-connectivity
  get_bounding_box                                    (image_tools.py:481-510)
Images are `Image3d` (numpy [z, y, x] + spacing / origin / direction); the `*_device` variants take and return device
tensors so that core/seg_infer.segmentation_volume keeps the whole chain on the GPU.
"""
import ctypes

import numpy as np
import torch

from segmentation3d import _engine as E
from segmentation3d.utils.image3d import Image3d, image_size_spacing


def _ceil_to(value, multiple):
    return value if value % multiple == 0 else multiple * (value // multiple + 1)


def image_partition_by_fixed_size(image, bbox_start_voxel, bbox_end_voxel, partition_size, partition_stride,
                                  max_stride):
    """Split the bounding box of an image into fixed-size, overlapping boxes (reference: image_tools.py:163-218).

    :param image: Image3d / sitk-like object (GetSize, GetSpacing) or a (size_xyz, spacing_xyz) pair
    :param bbox_start_voxel, bbox_end_voxel: partition region [start, end) in voxels (x, y, z); updated in place like
           the reference does (rounded up to a multiple of max_stride and clamped into the image)
    :param partition_size, partition_stride: physical size / stride of the boxes (mm)
    :return: (start_voxels, end_voxels), lists of [x, y, z]; order: x outermost, z innermost
    """
    size, spacing = image_size_spacing(image)
    extent, box, step, count = [0] * 3, [0] * 3, [0] * 3, [0] * 3
    for d in range(3):
        assert size[d] >= max_stride and size[d] % max_stride == 0
        # region: rounded up to the stride multiple, never larger than the image, shifted back inside if needed
        extent[d] = min(_ceil_to(min(size[d], bbox_end_voxel[d] - bbox_start_voxel[d]), max_stride), size[d])
        bbox_end_voxel[d] = bbox_start_voxel[d] + extent[d]
        if bbox_end_voxel[d] > size[d]:
            bbox_end_voxel[d] = size[d]
            bbox_start_voxel[d] = size[d] - extent[d]
        assert bbox_start_voxel[d] >= 0
        # box and step in voxels (round half up), box a stride multiple, both at most the region
        box[d] = min(extent[d], _ceil_to(int(partition_size[d] / spacing[d] + 0.5), max_stride))
        step[d] = min(extent[d], int(partition_stride[d] / spacing[d] + 0.5))
        count[d] = int(np.ceil((extent[d] - box[d]) / step[d]) + 1)
    start_voxels, end_voxels = [], []
    for ix in range(count[0]):
        for iy in range(count[1]):
            for iz in range(count[2]):
                lo = [bbox_start_voxel[d] + i * step[d] for d, i in enumerate((ix, iy, iz))]
                for d in range(3):  # the last box of a row is pulled back so that it ends at the region border
                    lo[d] = min(lo[d], bbox_end_voxel[d] - box[d])
                    assert lo[d] >= 0
                start_voxels.append([int(v) for v in lo])
                end_voxels.append([int(lo[d] + box[d]) for d in range(3)])
    return start_voxels, end_voxels


def convert_image_to_tensor(image):
    """Image3d (or list of them) -> float tensor [C, z, y, x] (reference: image_tools.py:274-294)"""
    if isinstance(image, Image3d):
        return torch.from_numpy(np.ascontiguousarray(image.array)).unsqueeze(0).float()
    if isinstance(image, (list, tuple)):
        return torch.cat([convert_image_to_tensor(im) for im in image], 0)
    raise ValueError('unknown input type')


def convert_tensor_to_image(tensor, dtype=None):
    """3-D tensor -> Image3d, 4-D tensor -> list of Image3d (reference: image_tools.py:297-326)"""
    assert isinstance(tensor, torch.Tensor), 'input must be a tensor'
    data = tensor.detach().cpu().numpy()
    if dtype is not None:
        data = data.astype(dtype)
    if tensor.dim() == 3:
        return Image3d(data)
    if tensor.dim() == 4:
        return [Image3d(data[i]) for i in range(data.shape[0])]
    raise ValueError('Only supports 3-dimsional or 4-dimensional image volume')


# ---------------------------------------------------------------------------------------------------------------------
# geometry on the device
# ---------------------------------------------------------------------------------------------------------------------
def _device():
    return torch.device('cuda', torch.cuda.current_device())


def index_affine(src_frame, dst_frame):
    """3 x 4 matrix M with  c_src = M @ (x, y, z, 1)  for an index (x, y, z) of the destination grid: destination
    index -> physical point -> continuous source index, as sitk.Resample does with an identity transform.
    frame = (spacing, origin, direction), direction row-major 3 x 3"""
    s_sp, s_or, s_dir = (np.asarray(v, dtype=np.float64) for v in src_frame)
    d_sp, d_or, d_dir = (np.asarray(v, dtype=np.float64) for v in dst_frame)
    Ds, Dd = s_dir.reshape(3, 3), d_dir.reshape(3, 3)
    to_src = np.diag(1.0 / s_sp) @ np.linalg.inv(Ds)
    M = np.zeros((3, 4))
    M[:, :3] = to_src @ Dd @ np.diag(d_sp)
    M[:, 3] = to_src @ (d_or - s_or)
    return M


def mirror_index_affine(M, out_size, mirror):
    """index map of the destination grid mirrored along the axes flagged in `mirror` = (x, y, z): destination index i of a
    mirrored axis of n voxels reads what index n - 1 - i read before.  The axis column of the 3 x 4 matrix is negated and
    (n - 1) times the column goes to the offset; a copy is returned."""
    M = np.array(M, dtype=np.float64)
    for a in range(3):
        if mirror[a]:
            M[:, 3] += (int(out_size[a]) - 1) * M[:, a]
            M[:, a] = -M[:, a]
    return M


def mirror_frame(frame, out_size, mirror):
    """(spacing, origin, direction) of the grid that mirror_index_affine samples: the origin moves to the last voxel of a
    mirrored axis and that axis' direction column changes sign"""
    spacing, origin, direction = (np.array(v, dtype=np.float64) for v in frame)
    D = direction.reshape(3, 3).copy()
    for a in range(3):
        if mirror[a]:
            origin = origin + D[:, a] * spacing[a] * (int(out_size[a]) - 1)
            D[:, a] = -D[:, a]
    return [float(v) for v in spacing], [float(v) for v in origin], [float(v) for v in D.reshape(-1)]


def rotation_matrix(angles):
    """R = Rz(gz) Ry(gy) Rx(gx) for angles = (gx, gy, gz) in radians, float64"""
    gx, gy, gz = (float(v) for v in angles)
    cx, sx, cy, sy, cz, sz = np.cos(gx), np.sin(gx), np.cos(gy), np.sin(gy), np.cos(gz), np.sin(gz)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rx


def rotate_index_affine(M, src_frame, dst_frame, out_size, angles):
    """index map of the destination grid rotated in physical space about its geometric centre
    c = origin + D diag(spacing) (n - 1) / 2: the sampled point p(i) of index i becomes p' = c + R (p(i) - c) with
    R = Rz(gz) Ry(gy) Rx(gx), angles = (gx, gy, gz) in radians.  M is index_affine(src_frame, dst_frame); a copy is
    returned, and with all angles zero it is M bit for bit.  Apply before mirror_index_affine."""
    M = np.array(M, dtype=np.float64)
    if not any(float(a) != 0.0 for a in angles):
        return M
    s_sp, s_or, s_dir = (np.asarray(v, dtype=np.float64) for v in src_frame)
    d_sp, d_or, d_dir = (np.asarray(v, dtype=np.float64) for v in dst_frame)
    to_src = np.diag(1.0 / s_sp) @ np.linalg.inv(s_dir.reshape(3, 3))
    A = d_dir.reshape(3, 3) @ np.diag(d_sp)                       # index -> physical offset from the origin
    n = np.array([int(v) for v in out_size], dtype=np.float64)
    c = d_or + A @ ((n - 1.0) / 2.0)
    R = rotation_matrix(angles)
    out = np.zeros((3, 4))
    out[:, :3] = to_src @ R @ A
    out[:, 3] = to_src @ (c + R @ (d_or - c) - s_or)
    return out


def bspline_control_dims(out_size, spacing, grid_mm):
    """(gx, gy, gz) control points of the cubic B-spline displacement field over a destination grid of `out_size` voxels
    at `spacing` mm with control spacing `grid_mm`: floor((n - 1) sp / h) + 4 per axis"""
    h = float(grid_mm)
    return tuple(int(np.floor((int(out_size[a]) - 1) * (float(spacing[a]) / h))) + 4 for a in range(3))


def _deform_call_args(src_frame, dst_frame, out_size, deform, mirror):
    """host arguments of the seg3d_resample_deform entries: L (3 x 3 `to_src` of index_affine), the control tensor, its
    dims, the per-axis spacing / grid factors and the mirror mask.  deform = (ctrl, grid_mm), ctrl a float32 device
    tensor [gz, gy, gx, 3] of displacements in mm (world x, y, z)."""
    ctrl, grid_mm = deform
    E.require_device(ctrl)
    if ctrl.dtype != torch.float32 or ctrl.dim() != 4 or ctrl.shape[3] != 3 or not ctrl.is_contiguous():
        raise ValueError('control tensor must be a contiguous float32 [gz, gy, gx, 3] tensor')
    h = float(grid_mm)
    if not h > 0.0:
        raise ValueError('control grid spacing must be positive, got {}'.format(grid_mm))
    d_sp = [float(v) for v in dst_frame[0]]
    want = bspline_control_dims(out_size, d_sp, h)
    gz, gy, gx = (int(v) for v in ctrl.shape[:3])
    if (gx, gy, gz) != want:
        raise ValueError('control tensor has (gx, gy, gz) = {}, the grid needs {}'.format((gx, gy, gz), want))
    s_sp, _, s_dir = (np.asarray(v, dtype=np.float64) for v in src_frame)
    L = np.ascontiguousarray(np.diag(1.0 / s_sp) @ np.linalg.inv(s_dir.reshape(3, 3)), dtype=np.float64)
    t = np.array([sp / h for sp in d_sp], dtype=np.float64)
    mask = sum(1 << a for a in range(3) if mirror is not None and mirror[a])
    return L, ctrl, (gx, gy, gz), t, mask


def _crop_index_map(src_frame, dst_frame, out_size, rotation, mirror):
    M = index_affine(src_frame, dst_frame)
    if rotation is not None:
        M = rotate_index_affine(M, src_frame, dst_frame, out_size, rotation)
    if mirror is not None and any(mirror):
        M = mirror_index_affine(M, out_size, mirror)
    return np.ascontiguousarray(M, dtype=np.float64)


def bspline_prefilter_device(volume, out=None):
    """samples -> cubic B-spline coefficients (seg3d_bspline_prefilter_mc, whole-sample mirror): volume a float32 device
    tensor [Z, Y, X] or [Z, Y, X, M], M <= 8; `out`: a contiguous tensor of the same shape, `volume` itself for in place.
    Returns the coefficients: what the 'BSPLINE' resampling entries take with prefiltered=True."""
    E.require_device(volume, out)
    if volume.dim() not in (3, 4) or volume.dtype != torch.float32:
        raise ValueError('volume must be a float32 [Z, Y, X] or [Z, Y, X, M] tensor')
    if out is None:
        volume = volume.contiguous()
        out = torch.empty_like(volume)
    elif (not volume.is_contiguous() or out.shape != volume.shape or not out.is_contiguous()
          or out.dtype != torch.float32):
        raise ValueError('volume and out must be contiguous float32 tensors of one shape')
    Z, Y, X = (int(v) for v in volume.shape[:3])
    M = int(volume.shape[3]) if volume.dim() == 4 else 1
    E.call('seg3d_bspline_prefilter_mc', E.ptr(volume), E.ptr(out), X, Y, Z, M, E.stream_ptr())
    return out


# element types a 'LINEAR' / 'NN' resampling source may have -> the dtype code of the typed entries (csrc/label_device.h);
# every value of the three integer types is exact in a float, which is what makes a compact source lossless
_SRC_DTYPE_CODES = {torch.int8: 0, torch.uint8: 1, torch.int16: 2, torch.float32: 4}


def resample_device(src, src_frame, out_size, dst_frame, interp_method, padding_value=0.0, mirror=None, rotation=None,
                    deform=None, prefiltered=False):
    """src: float32 (or, for 'LINEAR' / 'NN' / 'LABEL_LINEAR', int16 / uint8 / int8) device tensor [Z, Y, X]; returns the float32 device
    tensor [Zo, Yo, Xo] of the destination grid: the M = 1 case of resample_device_mc (a [Z, Y, X] volume is the same
    memory as [Z, Y, X, 1])."""
    E.require_device(src)
    if src.dim() != 3:
        raise ValueError('src must be a [Z, Y, X] tensor')
    return resample_device_mc(src.unsqueeze(3), src_frame, out_size, dst_frame, interp_method, padding_value,
                              mirror=mirror, rotation=rotation, deform=deform, prefiltered=prefiltered)[..., 0]


def resample_device_mc(src, src_frame, out_size, dst_frame, interp_method, padding_value=0.0, out=None, mirror=None,
                       rotation=None, deform=None, prefiltered=False):
    """M co-registered channels in one launch: src float32 device tensor [Z, Y, X, M] (channels-last) -> [Zo, Yo, Xo, M].
    `out`: a contiguous [Zo, Yo, Xo, M] destination, e.g. slot b of an NDHWC batch.  Channel m equals resample_device
    on src[..., m] bit for bit (seg3d_resample_affine_mc; with `deform` seg3d_resample_deform_mc).
    mirror = (x, y, z) flags: the destination grid is sampled mirrored along those axes (mirror_index_affine).
    rotation = (gx, gy, gz) radians: the grid is rotated about its centre (rotate_index_affine).  deform = (ctrl, grid_mm):
    the sampled points are displaced by a cubic B-spline field (ctrl float32 device [gz, gy, gx, 3] mm,
    bspline_control_dims points).  Without the last two this is the plain affine launch.
    interp_method 'BSPLINE': exact cubic B-spline interpolation (seg3d_resample_bspline_mc / _deform_mc).  With
    prefiltered=False src holds samples and is prefiltered into a temporary first (bspline_prefilter_device); with
    prefiltered=True src already holds the coefficients and the call is the one evaluation launch.  The other methods
    ignore the keyword.
    'LINEAR' and 'NN' also take a CONTIGUOUS int16, uint8 or int8 src, a volume kept as its file stores it
    (seg3d_resample_affine_typed_mc / seg3d_resample_deform_typed_mc): the result, always float32, equals the call on
    src.float() bit for bit.  'BSPLINE' with such a source and any other dtype raise ValueError.
    interp_method 'LABEL_LINEAR': for LABEL MAPS, M = 1 only (seg3d_resample_label / seg3d_resample_label_deform; defined
    in include/seg3d_hip.h and DESIGN.md section 7 row f22): every distinct value among a voxel's eight trilinear taps is
    interpolated as its 0 / 1 indicator and the value with the largest membership is written, ties to the smallest value --
    the first-maximum arg-max over per-label 'LINEAR' planes, in one launch and without the planes.  An arg-max, not a
    `>= 0.5` threshold: a voxel where no label reaches 0.5 still gets its strongest label.  Takes the same sources, mirror,
    rotation, deform and padding_value; M > 1 and prefiltered=True raise ValueError."""
    if interp_method not in ('LINEAR', 'NN', 'BSPLINE', 'LABEL_LINEAR'):
        raise ValueError('Unsupported interpolation type.')
    E.require_device(src)
    if src.dim() != 4 or src.dtype not in _SRC_DTYPE_CODES:
        raise ValueError('src must be a float32 (or int16 / uint8 / int8) [Z, Y, X, M] tensor')
    if interp_method == 'LABEL_LINEAR':
        if int(src.shape[3]) != 1:
            raise ValueError("'LABEL_LINEAR' interpolates one label map: M = {} channels".format(int(src.shape[3])))
        if prefiltered:
            raise ValueError("'LABEL_LINEAR' reads labels, not B-spline coefficients: prefiltered=True")
    typed = src.dtype != torch.float32
    if typed and interp_method == 'BSPLINE':
        raise ValueError("'BSPLINE' evaluates fp32 coefficients: a {} source takes 'LINEAR' or 'NN'".format(src.dtype))
    if typed and not src.is_contiguous():
        raise ValueError('a {} source must be contiguous'.format(src.dtype))
    src = src.contiguous()
    Zi, Yi, Xi, M = src.shape
    Xo, Yo, Zo = (int(v) for v in out_size)
    if out is None:
        out = torch.empty((Zo, Yo, Xo, M), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (Zo, Yo, Xo, M) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError('out must be a contiguous float32 [{}, {}, {}, {}] tensor'.format(Zo, Yo, Xo, M))
    M_ = _crop_index_map(src_frame, dst_frame, (Xo, Yo, Zo), rotation, mirror)
    if interp_method == 'BSPLINE':
        coef = src if prefiltered else bspline_prefilter_device(src)
        if deform is None:
            E.call('seg3d_resample_bspline_mc', E.ptr(coef), E.ptr(out), int(M), int(M), Xi, Yi, Zi, Xo, Yo, Zo,
                   M_.ctypes.data_as(ctypes.c_void_p), float(padding_value), E.stream_ptr())
            return out
        L, ctrl, g, t, mask = _deform_call_args(src_frame, dst_frame, (Xo, Yo, Zo), deform, mirror)
        E.call('seg3d_resample_bspline_deform_mc', E.ptr(coef), E.ptr(out), int(M), int(M), Xi, Yi, Zi, Xo, Yo, Zo,
               M_.ctypes.data_as(ctypes.c_void_p), float(padding_value), L.ctypes.data_as(ctypes.c_void_p), E.ptr(ctrl),
               g[0], g[1], g[2], t.ctypes.data_as(ctypes.c_void_p), mask, E.stream_ptr())
        return out
    if interp_method == 'LABEL_LINEAR':   # one entry for every source type: the dtype code is always passed
        if deform is None:
            E.call('seg3d_resample_label', E.ptr(src), _SRC_DTYPE_CODES[src.dtype], E.ptr(out), Xi, Yi, Zi, Xo, Yo, Zo,
                   M_.ctypes.data_as(ctypes.c_void_p), float(padding_value), E.stream_ptr())
            return out
        L, ctrl, g, t, mask = _deform_call_args(src_frame, dst_frame, (Xo, Yo, Zo), deform, mirror)
        E.call('seg3d_resample_label_deform', E.ptr(src), _SRC_DTYPE_CODES[src.dtype], E.ptr(out), Xi, Yi, Zi, Xo, Yo, Zo,
               M_.ctypes.data_as(ctypes.c_void_p), float(padding_value), L.ctypes.data_as(ctypes.c_void_p), E.ptr(ctrl),
               g[0], g[1], g[2], t.ctypes.data_as(ctypes.c_void_p), mask, E.stream_ptr())
        return out
    # a float source calls the float entries; any other goes through the typed ones with its dtype code
    suffix, source = ('_typed_mc', (E.ptr(src), _SRC_DTYPE_CODES[src.dtype])) if typed else ('_mc', (E.ptr(src),))
    if deform is None:
        E.call('seg3d_resample_affine' + suffix, *source, E.ptr(out), int(M), int(M), Xi, Yi, Zi, Xo, Yo, Zo,
               M_.ctypes.data_as(ctypes.c_void_p), int(interp_method == 'LINEAR'), float(padding_value), E.stream_ptr())
        return out
    L, ctrl, g, t, mask = _deform_call_args(src_frame, dst_frame, (Xo, Yo, Zo), deform, mirror)
    E.call('seg3d_resample_deform' + suffix, *source, E.ptr(out), int(M), int(M), Xi, Yi, Zi, Xo, Yo, Zo,
           M_.ctypes.data_as(ctypes.c_void_p), int(interp_method == 'LINEAR'), float(padding_value),
           L.ctypes.data_as(ctypes.c_void_p), E.ptr(ctrl), g[0], g[1], g[2], t.ctypes.data_as(ctypes.c_void_p), mask,
           E.stream_ptr())
    return out


def ensemble_accumulate_device(probs, src_frame, acc, dst_frame, weight, first, pad0=1.0, mask=None, regions_order=None):
    """one ensemble member onto the image grid (seg3d_ensemble_accumulate):
    probs float32 contiguous device [C, Zi, Yi, Xi] on the grid `src_frame`, acc float32 contiguous device [C, Zo, Yo, Xo]
    on the grid `dst_frame`.  Plane c of probs is resampled exactly as resample_device(probs[c], src_frame, (Xo, Yo, Zo),
    dst_frame, 'LINEAR', pad0 if c == 0 else 0.0) and acc[c] = weight * that when `first` (acc is not read), else
    acc[c] + weight * that (float32, rounded multiply then rounded add).  mask: None, or an int8 device [Zo, Yo, Xo] tensor
    that receives the label map of the updated acc in the same pass -- the first-maximum arg-max, or with regions_order
    (C labels in 1..127) the sequential overwrite rule p_r > 0.5.  Returns acc."""
    for name, t, dtype, dim in (('probs', probs, torch.float32, 4), ('acc', acc, torch.float32, 4),
                                ('mask', mask, torch.int8, 3)):
        if t is None and name == 'mask':
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != dim or not t.is_contiguous():
            raise ValueError('{} must be a contiguous {} device tensor with {} dimensions'.format(name, dtype, dim))
        if t.device != probs.device:
            raise ValueError('{} is on {} but probs on {}'.format(name, t.device, probs.device))
    E.require_device(probs, acc, mask)
    C, Zi, Yi, Xi = (int(v) for v in probs.shape)
    Zo, Yo, Xo = (int(v) for v in acc.shape[1:])
    if not 1 <= C <= 16:
        raise ValueError('{} planes: 1..16 are supported'.format(C))
    if int(acc.shape[0]) != C:
        raise ValueError('acc has {} planes, probs {}'.format(int(acc.shape[0]), C))
    if min(Zi, Yi, Xi, Zo, Yo, Xo) < 1:
        raise ValueError('empty grid: probs {}, acc {}'.format(tuple(probs.shape), tuple(acc.shape)))
    if mask is not None and tuple(mask.shape) != (Zo, Yo, Xo):
        raise ValueError('mask must be [{}, {}, {}], got {}'.format(Zo, Yo, Xo, tuple(mask.shape)))
    order = None
    if regions_order is not None:
        from segmentation3d.loss.region_loss import check_region_class_order
        order = (ctypes.c_int * C)(*check_region_class_order(regions_order, C))
    weight = float(weight)
    if not np.isfinite(weight):
        raise ValueError('weight must be finite, got {!r}'.format(weight))
    M_ = _crop_index_map(src_frame, dst_frame, (Xo, Yo, Zo), None, None)
    E.call('seg3d_ensemble_accumulate', E.ptr(probs), E.ptr(acc), E.ptr(mask), C, Xi, Yi, Zi, Xo, Yo, Zo,
           M_.ctypes.data_as(ctypes.c_void_p), weight, int(bool(first)), float(pad0), order, E.stream_ptr())
    return acc


def planar_to_channels_last(planes):
    """[M, Z, Y, X] float32 device tensor -> [Z, Y, X, M] (seg3d_ncdhw_to_ndhwc with N = 1, C = M)"""
    E.require_device(planes)
    planes = planes.contiguous()
    M, Z, Y, X = planes.shape
    out = torch.empty((Z, Y, X, M), dtype=torch.float32, device=planes.device)
    E.call('seg3d_ncdhw_to_ndhwc', E.ptr(planes), E.ptr(out), 1, int(M), Z * Y * X, E.stream_ptr())
    return out


def storage_dtype(array, kind):
    """numpy dtype a host array is kept resident as under dataset.resident_storage = 'compact' (pure host function).
    kind 'image': an array of an integer element type whose min and max lie in [-32768, 32767] -> int16; anything else --
    float files, a NIfTI with scl_slope / scl_inter (already floats), uint16 above 32767 -- -> float32.
    kind 'mask': integer values all in [0, 255] -> uint8; otherwise all in [-32768, 32767] -> int16; else float32.
    Every value of the chosen integer type is exact in a float, so the crops of the compact case are those of the
    float32 case bit for bit."""
    if kind not in ('image', 'mask'):
        raise ValueError("kind must be 'image' or 'mask', got {!r}".format(kind))
    array = np.asarray(array)
    if not np.issubdtype(array.dtype, np.integer):
        return np.dtype(np.float32)
    lo, hi = (int(array.min()), int(array.max())) if array.size else (0, 0)
    if kind == 'mask' and lo >= 0 and hi <= 255:
        return np.dtype(np.uint8)
    if lo >= -32768 and hi <= 32767:
        return np.dtype(np.int16)
    return np.dtype(np.float32)


def case_storage_dtype(images):
    """storage_dtype of a case's image volume: int16 only if EVERY modality qualifies, else the whole volume is float32"""
    compact = all(storage_dtype(im.array, 'image') == np.int16 for im in images)
    return np.dtype(np.int16 if compact else np.float32)


def images_to_host(images, dtype):
    """list of M co-registered Image3d -> the channels-last [Z, Y, X, M] host array of a non-float storage dtype, built
    once per case with np.stack(..., axis=-1)"""
    return np.ascontiguousarray(np.stack([np.asarray(im.array).astype(dtype, copy=False) for im in images], axis=-1))


def images_to_device(images, device, dtype=np.float32):
    """list of M co-registered Image3d -> resident [Z, Y, X, M] device tensor, float32 by default; a non-float `dtype`
    (a storage_dtype) is laid out channels-last on the host (images_to_host) and uploaded as it is"""
    if np.dtype(dtype) != np.float32:
        return torch.from_numpy(images_to_host(images, dtype)).to(device)
    planes = torch.from_numpy(np.stack([np.asarray(im.array, dtype=np.float32) for im in images], 0)).to(device)
    if len(images) == 1:                    # [1, Z, Y, X] is the same memory as [Z, Y, X, 1]
        return planes[0].unsqueeze(3)
    return planar_to_channels_last(planes)


def normalizer_params(normalizers, num_modality):
    """per-modality normalisers (objects with to_dict(), checkpoint dicts, or None = no normalisation) -> the
    Seg3dNormalizers struct passed by value to seg3d_patch_gather_normalize_mc"""
    if len(normalizers) != num_modality:
        raise ValueError('{} crop normalizers for {} modalities: one normalizer per modality'.format(
            len(normalizers), num_modality))
    params = E.Normalizers()
    for m in range(8):
        n = params.n[m]
        d = None if m >= num_modality or normalizers[m] is None else normalizers[m]
        if d is not None and hasattr(d, 'to_dict'):
            d = d.to_dict()
        if d is None:
            n.type, n.mean, n.stddev, n.clip, n.clip_lo, n.clip_hi = -1, 0.0, 1.0, 0, -1.0, 1.0
        elif d['type'] == 0:
            n.type, n.mean, n.stddev, n.clip, n.clip_lo, n.clip_hi = 0, float(d['mean']), float(d['stddev']), \
                int(bool(d['clip'])), -1.0, 1.0
        elif d['type'] == 1:
            sigma = float(d['clip_sigma'])
            n.type, n.mean, n.stddev, n.clip, n.clip_lo, n.clip_hi = 1, 0.0, 1.0, 1, -sigma, sigma
        elif d['type'] == 3:
            # the kernel clips the z-score, the rule clips the raw value: f(x) = fp32 (x - mean) / stddev is monotone
            # including its rounding, so clip(f(x), f(lo), f(hi)) == f(clip(x, lo, hi)) bit for bit when the bounds are
            # rounded as the kernel rounds them (fp32 subtract, correctly rounded fp32 divide, no contraction)
            mean, std = np.float32(d['mean']), np.float32(d['stddev'])
            if not std > 0:
                raise ValueError('stddev must be positive, got {!r}'.format(d['stddev']))
            lo, hi = d.get('lower'), d.get('upper')
            f_lo = float('-inf') if lo is None else float((np.float32(lo) - mean) / std)
            f_hi = float('inf') if hi is None else float((np.float32(hi) - mean) / std)
            n.type, n.mean, n.stddev, n.clip, n.clip_lo, n.clip_hi = 0, float(mean), float(std), \
                int(lo is not None or hi is not None), f_lo, f_hi
            if n.clip == 0:
                n.clip_lo, n.clip_hi = -1.0, 1.0
        elif d['type'] == 2:
            raise ValueError('a VolumeNormalizer (type 2) takes its numbers from a volume: resolve it first '
                             '(image_tools.resolve_normalizers)')
        else:
            raise ValueError('Unsupported normalization type.')
    return params


# ---------------------------------------------------------------------------------------------------------------------
# whole-volume statistics (csrc/volume_stats.hip) and the case-level normalisers built on them
# ---------------------------------------------------------------------------------------------------------------------
_STAT_MODES = {'all': 0, 'nonzero': 1, 'mask': 2}


class VolumeStatsAccumulator(object):
    """the split entries of seg3d_volume_stats_*: statistics of the union of several volumes' selected voxels (a data set).
    Every volume is passed once per pass, in any order, with the same M:
        acc = VolumeStatsAccumulator(M, mode, quantiles, clip, device)
        for level in acc.levels():
            for volume, sel in volumes: acc.add_hist(volume, sel, level)
            acc.resolve(level)
        for volume, sel in volumes: acc.add_moments(volume, sel)
        stats = acc.finish()
    Nothing is read back before finish(), which makes the one device-to-host transfer."""

    def __init__(self, num_modality, mode='nonzero', quantiles=(), clip=False, device=None, begin=True):
        if mode not in _STAT_MODES:
            raise ValueError("mode must be 'all', 'nonzero' or 'mask', got {!r}".format(mode))
        self.M, self.mode = int(num_modality), _STAT_MODES[mode]
        if not 1 <= self.M <= 8:
            raise ValueError('{} modalities, 1..8 are supported'.format(self.M))
        self.quantiles = [float(q) for q in quantiles]
        if len(self.quantiles) > 4 or any(not 0.0 <= q <= 1.0 for q in self.quantiles):
            raise ValueError('quantiles {!r}: at most four values in [0, 1]'.format(list(quantiles)))
        self.clip = bool(clip)
        if self.clip and (len(self.quantiles) < 2 or self.quantiles[0] > self.quantiles[1]):
            raise ValueError('the clamp needs two quantiles q0 <= q1')
        self.device = device if device is not None else _device()
        self._q = (ctypes.c_double * 4)(*(self.quantiles + [0.0] * (4 - len(self.quantiles))))
        self.state = torch.empty((E.query('seg3d_volume_stats_state_bytes', self.M) // 8,), dtype=torch.int64,
                                 device=self.device)
        E.require_device(self.state)
        if begin:   # (the one-volume entry zeroes the state itself)
            E.call('seg3d_volume_stats_begin', E.ptr(self.state), self.M, E.stream_ptr())

    def levels(self):
        return (0, 1, 2) if self.quantiles else (0,)

    def _check(self, volume, sel):
        E.require_device(volume, sel)
        if volume.dtype != torch.float32 or volume.dim() != 4 or not volume.is_contiguous() \
                or int(volume.shape[3]) != self.M:
            raise ValueError('volume must be a contiguous float32 [Z, Y, X, {}] tensor'.format(self.M))
        nv = int(volume.shape[0]) * int(volume.shape[1]) * int(volume.shape[2])
        if not 0 < nv < 2 ** 31:
            raise ValueError('{} voxels: 1 .. 2^31 - 1 per call'.format(nv))
        if self.mode == 2:
            if sel is None or sel.dtype != torch.uint8 or not sel.is_contiguous() \
                    or tuple(sel.shape) != tuple(volume.shape[:3]):
                raise ValueError("mode 'mask' needs a contiguous uint8 selection plane of the volume's [Z, Y, X]")
        return nv

    def add_hist(self, volume, sel, level):
        nv = self._check(volume, sel)
        E.call('seg3d_volume_stats_accumulate_hist', E.ptr(volume), E.ptr(sel) if self.mode == 2 else None, nv, self.M,
               self.mode, int(level), E.ptr(self.state), E.stream_ptr())

    def resolve(self, level):
        E.call('seg3d_volume_stats_resolve', E.ptr(self.state), self.M, len(self.quantiles), self._q, int(level),
               E.stream_ptr())

    def add_moments(self, volume, sel):
        nv = self._check(volume, sel)
        E.call('seg3d_volume_stats_accumulate_moments', E.ptr(volume), E.ptr(sel) if self.mode == 2 else None, nv, self.M,
               self.mode, int(self.clip), E.ptr(self.state), E.stream_ptr())

    def finish(self):
        out = torch.empty((self.M, 9), dtype=torch.float64, device=self.device)
        E.call('seg3d_volume_stats_finish', E.ptr(self.state), self.M, len(self.quantiles), int(self.clip), E.ptr(out),
               E.stream_ptr())
        return _stats_rows(out, len(self.quantiles))


def _stats_rows(out, Q):
    rows = out.cpu().numpy()
    return [{'n': int(r[0]), 'min': float(r[1]), 'max': float(r[2]), 'mean': float(r[3]), 'std': float(r[4]),
             'q': [float(v) for v in r[5:5 + Q]]} for r in rows]


def volume_stats_device(volume, mode='nonzero', sel=None, quantiles=(), clip=False):
    """exact statistics of a whole float32 channels-last device volume [Z, Y, X, M] (seg3d_volume_stats): per modality a
    dict(n, min, max, mean, std, q) over the voxels selected by mode 'all' | 'nonzero' (x != 0) | 'mask' (sel != 0, a uint8
    [Z, Y, X] device tensor).  q: the order statistics sorted(S)[floor(q_i (n - 1) + 0.5)] of up to four `quantiles` in
    [0, 1] -- the nearest rank, not numpy's linear interpolation.  mean / population std (floored at 1e-6) in float64, with
    clip=True of the values clamped to [q[0], q[1]].  n == 0: all 0 and std = 1e-6.  One device-to-host transfer."""
    if volume.dim() != 4:
        raise ValueError('volume must be a float32 [Z, Y, X, M] tensor')
    with torch.cuda.device(volume.device):
        acc = VolumeStatsAccumulator(int(volume.shape[3]), mode, quantiles, clip, volume.device, begin=False)
        nv = acc._check(volume, sel)
        out = torch.empty((acc.M, 9), dtype=torch.float64, device=volume.device)
        E.call('seg3d_volume_stats', E.ptr(volume), E.ptr(sel) if acc.mode == 2 else None, nv, acc.M, acc.mode,
               len(acc.quantiles), acc._q, int(acc.clip), E.ptr(acc.state), E.ptr(out), E.stream_ptr())
        return _stats_rows(out, len(acc.quantiles))


def _normalizer_dict(n):
    return n.to_dict() if n is not None and hasattr(n, 'to_dict') else n


def has_volume_normalizer(normalizers):
    """does the list hold a VolumeNormalizer (type 2), i.e. does it need a volume before it can be applied?"""
    return any(d is not None and d['type'] == 2 for d in (_normalizer_dict(n) for n in normalizers))


def resolve_normalizers(normalizers, volume):
    """normalisers of the modalities of `volume` (float32 channels-last device [Z, Y, X, M], holding SAMPLES -- before any
    B-spline prefilter) -> a list in which every VolumeNormalizer / type-2 dict is replaced by the type-3 dict of its
    numbers for this volume; the other entries are returned as they are, and without a type 2 nothing is launched.
    Modalities that share (foreground, clip_percentiles) share one statistics call; a modality whose non-zero selection is
    empty is resolved over all voxels."""
    from segmentation3d.utils.normalizer import resolved_normalizer
    dicts = [_normalizer_dict(n) for n in normalizers]
    if not any(d is not None and d['type'] == 2 for d in dicts):
        return list(normalizers)
    if volume.dim() != 4 or int(volume.shape[3]) != len(dicts):
        raise ValueError('{} normalizers for a volume of shape {}: one per modality of [Z, Y, X, M]'.format(
            len(dicts), tuple(volume.shape)))
    out, cache = list(normalizers), {}

    def stats(foreground, pct):
        key = (foreground, None if pct is None else tuple(pct))
        if key not in cache:
            q = [] if pct is None else [float(p) / 100.0 for p in pct]
            cache[key] = volume_stats_device(volume, foreground, quantiles=q, clip=bool(q))
        return cache[key]

    for m, d in enumerate(dicts):
        if d is None or d['type'] != 2:
            continue
        foreground, pct = d.get('foreground', 'nonzero'), d.get('clip_percentiles')
        st = stats(foreground, pct)[m]
        if st['n'] == 0 and foreground != 'all':
            st = stats('all', pct)[m]
        out[m] = resolved_normalizer(d, st).to_dict()
    return out


def _frame(image):
    return (image.GetSpacing(), image.GetOrigin(), image.GetDirection())


def resample(image, reference, interp_method, padding_value=0.0):
    """Resample `image` onto the grid of `reference` (reference: image_tools.py:329-345)"""
    assert isinstance(image, Image3d) and isinstance(reference, Image3d)
    src = torch.from_numpy(np.array(image.array, dtype=np.float32, order='C')).to(_device())
    out = resample_device(src, _frame(image), reference.GetSize(), _frame(reference), interp_method, padding_value)
    return Image3d(out.cpu().numpy(), *_frame(reference))


def resampled_size(in_size, in_spacing, out_spacing, max_stride):
    """output size of resample_spacing (image_tools.py:361-365): round half up, then up to a multiple of max_stride"""
    out = [int(in_size[d] * in_spacing[d] / out_spacing[d] + 0.5) for d in range(3)]
    return [max_stride * (v // max_stride + 1) if v % max_stride else v for v in out]


def resample_spacing(image, resampled_spacing, max_stride, interp_method):
    """Resample to a new spacing, same origin / direction, size a multiple of max_stride (image_tools.py:348-377);
    voxels beyond the input extent take ITK's default pixel value 0"""
    assert isinstance(image, Image3d)
    out_spacing = [float(v) for v in resampled_spacing]
    out_size = resampled_size(image.GetSize(), image.GetSpacing(), out_spacing, max_stride)
    dst_frame = (out_spacing, image.GetOrigin(), image.GetDirection())
    src = torch.from_numpy(np.array(image.array, dtype=np.float32, order='C')).to(_device())
    out = resample_device(src, _frame(image), out_size, dst_frame, interp_method, 0.0)
    return Image3d(out.cpu().numpy(), *dst_frame)


def connected_component_filter_device(mask, labels, mode, threshold=0):
    """mask: int8 device tensor [Z, Y, X]; per label keeps the largest 26-connected component (mode 'largest') or the
    components with at least `threshold` voxels (mode 'min_size'); composition as in the reference: the FIRST label's
    voxels become 1, every other label keeps its own value (image_tools.py:399-403, 429-431)"""
    assert isinstance(labels, list)
    E.require_device(mask)
    if mask.dtype != torch.int8:
        raise TypeError('mask must be int8')
    mask = mask.contiguous()
    Z, Y, X = mask.shape
    out = torch.zeros_like(mask)
    if not labels:
        return out
    ws = torch.empty(E.query('seg3d_ccl_workspace_ints', mask.numel()), dtype=torch.int32, device=mask.device)
    for k, label in enumerate(labels):
        E.call('seg3d_ccl26_select', E.ptr(mask), int(label), X, Y, Z, 0 if mode == 'largest' else 1, int(threshold),
               1 if k == 0 else int(label), int(k > 0), E.ptr(out), E.ptr(ws), E.stream_ptr())
    return out


def _mask_to_device(mask):
    assert isinstance(mask, Image3d)
    return torch.from_numpy(np.array(mask.array, dtype=np.int8, order='C')).to(_device())


def pick_largest_connected_component(mask, labels):
    """keep, for every label, only its largest 26-connected component (image_tools.py:380-405)"""
    out = connected_component_filter_device(_mask_to_device(mask), labels, 'largest')
    return Image3d(out.cpu().numpy().astype(mask.array.dtype), *_frame(mask))


def remove_small_connected_component(mask, labels, threshold):
    """drop, for every label, the 26-connected components smaller than `threshold` voxels (image_tools.py:408-432)"""
    out = connected_component_filter_device(_mask_to_device(mask), labels, 'min_size', threshold)
    return Image3d(out.cpu().numpy().astype(mask.array.dtype), *_frame(mask))


def get_bounding_box_device(mask, selected_labels):
    """mask: int8 device tensor [Z, Y, X] -> (start_voxel, end_voxel) in (x, y, z), end exclusive, or (None, None)"""
    E.require_device(mask)
    mask = mask.contiguous()
    Z, Y, X = mask.shape
    box = torch.tensor([2 ** 31 - 1] * 3 + [-1] * 3, dtype=torch.int32, device=mask.device)
    labels = [] if selected_labels is None else [int(v) for v in selected_labels]
    if selected_labels is not None and not labels:
        return None, None
    arr = (ctypes.c_int * max(1, len(labels)))(*labels) if labels else None
    E.call('seg3d_mask_bounding_box', E.ptr(mask), X, Y, Z, arr, len(labels), E.ptr(box), E.stream_ptr())
    b = box.cpu().tolist()
    if b[3] < 0:
        print('Fail to get the bounding box.')
        return None, None
    return [b[0], b[1], b[2]], [b[3] + 1, b[4] + 1, b[5] + 1]


def get_bounding_box(mask, selected_labels):
    """bounding box of the selected labels (None: every non-zero voxel), end exclusive (image_tools.py:481-510)"""
    return get_bounding_box_device(_mask_to_device(mask), selected_labels)


# ---------------------------------------------------------------------------------------------------------------------
# training crops on the device: crop_image (image_tools.py:103-141) + the crop normalisers
# ---------------------------------------------------------------------------------------------------------------------
def crop_origin(cropping_center, cropping_size, cropping_spacing):
    """world position of the crop's first voxel (image_tools.py:121-126): centre - size/2, moved in by half a voxel;
    like the reference this ignores the image direction"""
    out = []
    for idx in range(3):
        physical = int(cropping_size[idx]) * float(cropping_spacing[idx])
        out.append(float(cropping_center[idx]) - physical / 2.0 + float(cropping_spacing[idx]) / 2.0)
    return out


def crop_image_device(volume, frame, cropping_center, cropping_size, cropping_spacing, interp_method, mirror=None,
                      rotation=None, deform=None, prefiltered=False):
    """volume: float32 (or, for 'LINEAR' / 'NN' / 'LABEL_LINEAR', int16 / uint8 / int8) device tensor [Z, Y, X] with frame
    (spacing, origin, direction) -> float32 crop [z, y, x]: the M = 1 case of crop_image_device_mc.  'LABEL_LINEAR' is the
    mode for a label map (resample_device_mc)"""
    return crop_image_device_mc(volume.unsqueeze(3), frame, cropping_center, cropping_size, cropping_spacing, interp_method,
                                mirror=mirror, rotation=rotation, deform=deform, prefiltered=prefiltered)[..., 0]


def crop_image(image, cropping_center, cropping_size, cropping_spacing, interp_method):
    """Image3d in, Image3d out (reference: image_tools.py:103-141)"""
    assert isinstance(image, Image3d)
    src = torch.from_numpy(np.array(image.array, dtype=np.float32, order='C')).to(_device())
    out = crop_image_device(src, _frame(image), cropping_center, cropping_size, cropping_spacing, interp_method)
    spacing = [float(cropping_spacing[idx]) for idx in range(3)]
    return Image3d(out.cpu().numpy(), spacing, crop_origin(cropping_center, cropping_size, spacing), image.GetDirection())


def normalize_crop_device(crop, normalizer):
    """apply a FixedNormalizer / AdaptiveNormalizer (utils/normalizer.py) to a float32 device crop [z, y, x] with the
    patch kernel of the inference path (csrc/patch.hip: fp64 statistics, population std floored at 1e-6): the M = 1 case
    of normalize_crop_device_mc"""
    return normalize_crop_device_mc(crop.contiguous().unsqueeze(3), normalizer_params([normalizer], 1))[..., 0]


def crop_image_device_mc(volume, frame, cropping_center, cropping_size, cropping_spacing, interp_method, out=None,
                         mirror=None, rotation=None, deform=None, prefiltered=False):
    """volume: float32 device tensor [Z, Y, X, M] (channels-last) with frame (spacing, origin, direction) -> crop
    [z, y, x, M] of `cropping_size` voxels at `cropping_spacing`, centred at the world point `cropping_center`, zero
    outside, one launch for all modalities; mirror = (x, y, z) flags: the crop comes out mirrored along those axes (same
    launch, mirrored index map); rotation / deform: training augmentation inside the same launch, and prefiltered (the
    volume holds 'BSPLINE' coefficients): see resample_device_mc.  'LINEAR' and 'NN' also take a contiguous int16 / uint8 /
    int8 volume (a compact resident case); the crop is float32 and equals the crop of volume.float() bit for bit.
    'LABEL_LINEAR' (M = 1, a label map): the per-label trilinear vote, see resample_device_mc."""
    size = [int(cropping_size[idx]) for idx in range(3)]
    spacing = [float(cropping_spacing[idx]) for idx in range(3)]
    dst_frame = (spacing, crop_origin(cropping_center, size, spacing), frame[2])
    return resample_device_mc(volume, frame, size, dst_frame, interp_method, 0.0, out=out, mirror=mirror,
                              rotation=rotation, deform=deform, prefiltered=prefiltered)


def normalize_crop_device_mc(crop, params, out=None):
    """per-modality normalisation of a channels-last device crop [z, y, x, M] with the multi-modality patch kernel
    (P = 1, start 0); `params` from normalizer_params.  out may be `crop` itself (in place)."""
    E.require_device(crop)
    if not crop.is_contiguous():
        raise ValueError('crop must be contiguous [z, y, x, M]')
    bz, by, bx, M = crop.shape
    dev = crop.device
    if out is None:
        out = torch.empty_like(crop)
    starts = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    ws = torch.empty((E.query('seg3d_patch_stats_mc_doubles', bx, by, bz, 1, M),), dtype=torch.float64, device=dev)
    mean_std = torch.empty((M, 2), dtype=torch.float32, device=dev)
    E.call('seg3d_patch_gather_normalize_mc', E.ptr(crop), E.ptr(starts), E.ptr(out), E.ptr(ws), E.ptr(mean_std), bz, by,
           bx, bx, by, bz, 1, int(M), params, E.stream_ptr())
    return out


def _crop_modalities(crop):
    """M of a training crop handed to the intensity, blur and low-resolution passes: contiguous float32 [z, y, x] (M = 1)
    or channels-last [z, y, x, M], 1 <= M <= 8"""
    if crop.dtype != torch.float32 or crop.dim() not in (3, 4) or not crop.is_contiguous():
        raise ValueError('crop must be a contiguous float32 [z, y, x] or [z, y, x, M] tensor')
    M = 1 if crop.dim() == 3 else int(crop.shape[3])
    if not 1 <= M <= 8:
        raise ValueError('{} modalities, 1..8 are supported'.format(M))
    return M


INTENSITY_NEUTRAL = {'brightness': 1.0, 'contrast': 1.0, 'gamma': 1.0, 'invert': False, 'sigma': 0.0}


def intensity_params(params, num_modality, seed=0):
    """list of per-modality dicts (keys of INTENSITY_NEUTRAL, missing = neutral; None = all neutral) -> the
    Seg3dIntensityParams struct passed by value to seg3d_augment_intensity; seed: the 64-bit Philox key"""
    if len(params) != num_modality:
        raise ValueError('{} intensity parameter sets for {} modalities'.format(len(params), num_modality))
    out = E.IntensityParams()
    for m in range(8):
        d = dict(INTENSITY_NEUTRAL)
        if m < num_modality and params[m] is not None:
            unknown = set(params[m]) - set(d)
            if unknown:
                raise ValueError('unknown intensity parameter(s) {}'.format(sorted(unknown)))
            d.update(params[m])
        for key in ('brightness', 'contrast', 'gamma'):
            if not (np.isfinite(d[key]) and d[key] > 0.0):
                raise ValueError('{} must be positive, got {}'.format(key, d[key]))
        if not (np.isfinite(d['sigma']) and d['sigma'] >= 0.0):
            raise ValueError('sigma must be >= 0, got {}'.format(d['sigma']))
        p = out.m[m]
        p.brightness, p.contrast, p.gamma, p.invert, p.sigma = float(d['brightness']), float(d['contrast']), \
            float(d['gamma']), int(bool(d['invert'])), float(d['sigma'])
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError('seed must be in [0, 2^64), got {}'.format(seed))
    out.seed_lo, out.seed_hi = seed & 0xffffffff, seed >> 32
    return out


def augment_intensity_device(crop, params, seed=0, grid_blocks=0):
    """brightness, contrast, gamma and additive Gaussian noise on a normalised float32 device crop, IN PLACE
    (csrc/augment.hip, seg3d_augment_intensity): crop [z, y, x] (one modality) or channels-last [z, y, x, M], contiguous;
    params: one dict per modality with any of brightness, contrast, gamma (> 0), invert (bool), sigma (>= 0) -- missing
    keys are neutral and a neutral transform is skipped exactly -- or a ready E.IntensityParams.  seed: the noise's 64-bit
    Philox key; the noise of a voxel depends on (seed, voxel index, modality) alone.  Returns `crop`."""
    E.require_device(crop)
    M = _crop_modalities(crop)
    Z, Y, X = (int(v) for v in crop.shape[:3])
    prm = params if isinstance(params, E.IntensityParams) else intensity_params(params, M, seed)
    need_stats = any(prm.m[m].contrast != 1.0 or prm.m[m].gamma != 1.0 for m in range(M))
    ws = None
    if need_stats:
        ws = torch.empty((E.query('seg3d_augment_intensity_workspace_doubles', X, Y, Z, M),), dtype=torch.float64,
                         device=crop.device)
    E.call('seg3d_augment_intensity', E.ptr(crop), E.ptr(ws), X, Y, Z, M, prm, int(grid_blocks), E.stream_ptr())
    return crop


BLUR_MAX_SIGMA = 2.0     # radius ceil(3 sigma) <= 6: the halo the blur kernel stages in LDS


def gaussian_taps(sigma):
    """(R, taps) of the Gaussian blur: R = ceil(3 sigma) and the 2R + 1 taps w[-R..R] as float64,
    w[k] = exp(-k^2 / (2 sigma^2)) / sum_j exp(-j^2 / (2 sigma^2)); 0 < sigma <= 2 voxels"""
    sigma = float(sigma)
    if not (np.isfinite(sigma) and 0.0 < sigma <= BLUR_MAX_SIGMA):
        raise ValueError('blur sigma must be in (0, {}] voxels, got {}'.format(BLUR_MAX_SIGMA, sigma))
    R = int(np.ceil(3.0 * sigma))
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return R, w / w.sum()


def lowres_sizes(size, zoom):
    """low-grid sizes of the low-resolution simulation: n' = max(1, floor(n zoom + 0.5)) per axis of `size`, zoom in
    (0, 1]; zoom 1 is the identity"""
    zoom = float(zoom)
    if not (np.isfinite(zoom) and 0.0 < zoom <= 1.0):
        raise ValueError('low-resolution zoom must be in (0, 1], got {}'.format(zoom))
    return tuple(max(1, int(np.floor(int(n) * zoom + 0.5))) for n in size)


def blur_params(sigmas, num_modality):
    """per-modality sigma in voxels (0 or None = off) -> the Seg3dBlurParams struct passed by value to seg3d_augment_blur:
    radius and the taps w[|k|], k = 0..R, computed in double and rounded to float32"""
    if len(sigmas) != num_modality:
        raise ValueError('{} blur sigmas for {} modalities'.format(len(sigmas), num_modality))
    if not 1 <= num_modality <= 8:
        raise ValueError('{} modalities, 1..8 are supported'.format(num_modality))
    out = E.BlurParams()
    for m in range(num_modality):
        s = 0.0 if sigmas[m] is None else float(sigmas[m])
        if s == 0.0:
            continue
        R, w = gaussian_taps(s)
        out.radius[m] = R
        for k in range(R + 1):
            out.taps[m][k] = float(w[R + k])
    return out


def lowres_params(sizes, num_modality, crop_size=None):
    """per-modality low-grid sizes (nx', ny', nz') -> the Seg3dLowresParams struct passed by value to
    seg3d_augment_lowres; with crop_size = (nx, ny, nz), None stands for "off" and 1 <= n' <= n is checked"""
    if len(sizes) != num_modality:
        raise ValueError('{} low-grid sizes for {} modalities'.format(len(sizes), num_modality))
    if not 1 <= num_modality <= 8:
        raise ValueError('{} modalities, 1..8 are supported'.format(num_modality))
    out = E.LowresParams()
    for m in range(num_modality):
        sz = sizes[m]
        if sz is None:
            if crop_size is None:
                raise ValueError('low-grid size None (off) needs the crop size')
            sz = crop_size
        if len(sz) != 3 or any(int(v) != v or int(v) < 1 for v in sz):
            raise ValueError('low-grid size must be three positive integers, got {!r}'.format(sizes[m]))
        if crop_size is not None and any(int(v) > int(n) for v, n in zip(sz, crop_size)):
            raise ValueError('low-grid size {!r} exceeds the crop {!r}'.format(tuple(sz), tuple(crop_size)))
        out.nx[m], out.ny[m], out.nz[m] = (int(v) for v in sz)
    return out


def _filter_buffers(crop, out):
    E.require_device(crop, out)
    M = _crop_modalities(crop)
    if out is None:
        out = torch.empty_like(crop)
    else:
        if out.shape != crop.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError('out must be a contiguous float32 tensor of the crop\'s shape')
        nbytes = crop.numel() * 4
        if out.data_ptr() < crop.data_ptr() + nbytes and crop.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError('out overlaps crop: the filters run out of place')
    return M, out


def blur_device(crop, sigmas, out=None):
    """Gaussian blur of a normalised float32 device crop, OUT OF PLACE (csrc/augment_filter.hip, seg3d_augment_blur):
    crop [z, y, x] (one modality) or channels-last [z, y, x, M], contiguous; sigmas: one sigma in voxels per modality
    (0 or None = that modality is copied), or a ready E.BlurParams.  Separable, half-sample reflection at the border,
    radius ceil(3 sigma) <= 6.  Returns `out` (allocated when None; it must not overlap `crop`)."""
    M, out = _filter_buffers(crop, out)
    Z, Y, X = (int(v) for v in crop.shape[:3])
    prm = sigmas if isinstance(sigmas, E.BlurParams) else blur_params(sigmas, M)
    E.call('seg3d_augment_blur', E.ptr(crop), E.ptr(out), X, Y, Z, M, prm, E.stream_ptr())
    return out


def lowres_device(crop, zooms, out=None):
    """low-resolution simulation of a normalised float32 device crop, OUT OF PLACE (seg3d_augment_lowres): nearest
    down-sampling to the low grid of lowres_sizes(crop size, zoom), Keys cubic (a = -0.5) up-sampling back; the low grid
    is never stored.  zooms: one zoom in (0, 1] per modality (1 or None = that modality is copied), or a ready
    E.LowresParams.  Returns `out` (allocated when None; it must not overlap `crop`)."""
    M, out = _filter_buffers(crop, out)
    Z, Y, X = (int(v) for v in crop.shape[:3])
    if isinstance(zooms, E.LowresParams):
        prm = zooms
    else:
        if len(zooms) != M:
            raise ValueError('{} low-resolution zooms for {} modalities'.format(len(zooms), M))
        prm = lowres_params([None if z is None else lowres_sizes((X, Y, Z), z) for z in zooms], M, (X, Y, Z))
    E.call('seg3d_augment_lowres', E.ptr(crop), E.ptr(out), X, Y, Z, M, prm, E.stream_ptr())
    return out


def signed_distance_device(labels, class_ids, spacing, ignore_label=None):
    """signed Euclidean distance maps of a device label volume: `labels` [Z, Y, X] or a batch [N, Z, Y, X] of class ids
    (any dtype), `class_ids` 1..16 ids, `spacing` = (sx, sy, sz).  Returns float32 [K, Z, Y, X] or [N, K, Z, Y, X]: for
    each class the distance between voxel centres to the class (positive outside it) or to the rest (negative inside it),
    0 where the class or the rest is empty.  Negative labels and `ignore_label` are neither object nor background.  Every
    axis is at most 256 voxels (seg3d_signed_distance)."""
    from segmentation3d import _ops
    batched = labels.dim() == 4
    if labels.dim() not in (3, 4):
        raise ValueError('labels must be [Z, Y, X] or [N, Z, Y, X], got {}'.format(tuple(labels.shape)))
    phi = _ops.signed_distance(labels if batched else labels[None], class_ids, spacing, ignore_label)
    return phi if batched else phi[0]


def soft_skeleton_device(x, iters):
    """the soft skeleton of a float device volume `x` [Z, Y, X] (or any batch [..., Z, Y, X] of volumes) by `iters` = 1..16
    iterations of min / max pooling, as the clDice loss computes it: with E = min over a voxel and its 6 face neighbours,
    D = max over the 3x3x3 neighbourhood (nothing exists outside the volume) and O = D(E(.)):  x_0 = x,
    s_0 = relu(x_0 - O(x_0)), then x_j = E(x_{j-1}), d_j = relu(x_j - O(x_j)), s_j = s_{j-1} + relu(d_j - s_{j-1} d_j).
    Returns s_iters, float32, same shape; a 0 / 1 mask gives an exact 0 / 1 skeleton.  Every axis is at most 256 voxels
    (seg3d_soft_skeleton)."""
    from segmentation3d import _ops
    return _ops.soft_skeleton(x, iters)


def get_image_frame(image):
    """spacing, origin, direction packed into 15 float32 (image_tools.py:26-41)"""
    return np.array(list(image.GetSpacing()) + list(image.GetOrigin()) + list(image.GetDirection()), dtype=np.float32)


def set_image_frame(image, frame):
    """inverse of get_image_frame (image_tools.py:44-61)"""
    frame = np.asarray(frame)
    image.spacing = tuple(float(v) for v in frame[:3])
    image.origin = tuple(float(v) for v in frame[3:6])
    image.direction = tuple(float(v) for v in frame[6:15])


def select_random_voxels_in_multi_class_mask(mask, num_selected, selected_label):
    """`num_selected` random voxels (x, y, z) carrying `selected_label` (image_tools.py:246-271; numpy global RNG)"""
    mask_npy = mask.array if isinstance(mask, Image3d) else np.asarray(mask)
    valid_voxels = np.argwhere(mask_npy == selected_label)
    selected_voxels = []
    while len(valid_voxels) > 0 and len(selected_voxels) < num_selected:
        selected_voxels.append(valid_voxels[np.random.randint(0, len(valid_voxels))][::-1])
    return selected_voxels
