"""Frame metrics of the reference's QA stage (src/qa/*), evaluated on the device.

The reference scores the frames its Tester wrote with one script per metric (``compute_frame_*`` / ``compute_depth_*`` of
``src/qa/<NN>_<Metric>/src/<Metric>02_NeRF_LLFF.py``; the ``01_RealEstate`` siblings compute the same quantities), through
skimage, pandas and scipy on the host.  Here the frame never leaves the GPU: the HIP library reduces the uint8 image pair /
the fp32 depth pair to a handful of sums (exact int64 for the image errors, fp64 for everything else, fixed-order reductions --
csrc/metrics.hip) and the functions below evaluate the reference's expressions on those sums.  Sorting (for the median and the
ranks) and mask compaction are torch calls on the device, or -- ``sorter='library'`` -- the HIP library's own stable radix sort and
order-preserving compaction (csrc/sort.hip).

SSIM is pinned to a restatement of skimage's ``structural_similarity(gt, eval, multichannel=True, gaussian_weights=True,
sigma=1.5, use_sample_covariance=False)`` on ``scipy.ndimage.gaussian_filter`` (tests/qa_reference.py), not to skimage itself.
The reference's scripts round scaled fp32 depths to fp32 before subtracting; here the scale is applied in fp64 (a difference
of ~1e-7, below their 4-decimal rounding).

LPIPS (04, 14) is ``lpips.LPIPS(net='alex')`` on the device (csrc/lpips.hip: the five AlexNet convolutions as implicit GEMMs on
the fp32 matrix cores, fixed-order fp64 layer sums).  The build carries no network weights: ``LpipsWeights`` takes them from the
caller's checkpoint files (torchvision's AlexNet + the package's ``alex.pth``, or a saved ``lpips.LPIPS`` state dict), read with
``torch.load(weights_only=True)`` -- neither package has to be installed.  The metric is pinned to tests/lpips_reference.py, a
restatement of the package's published definition.  ``net='vgg'`` is the same metric on VGG-16's thirteen convolutions (what much
of the literature tabulates), through the same kernels and pinned to tests/lpips_vgg_reference.py; one ``LpipsWeights`` holds one
backbone.

The masks of the masked metrics are the stage's own first step (``src/qa/00_Common/src/mask_generators``): ``visibility_mask``
splats the training views' depths into the test view and tests them against its depth, on the device (csrc/visibility_mask.hip).
The Warper behind them is a utility of its own too: ``forward_warp`` (colour frame, mask, depth and flow), ``bilinear_splatting``
along any flow and ``bilinear_interpolation``, the backward warp (csrc/warp.hip), pinned to tests/warp_reference.py.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import numpy
import torch

from . import ops

Tensor = torch.Tensor
IMAGE_METRICS = ('RMSE', 'PSNR', 'SSIM')
DEPTH_METRICS = ('DepthRMSE', 'DepthMAE', 'DepthSROCC')
SSIM_CROP = (ops.SSIM_WINDOW - 1) // 2     # skimage crops the map by (win_size - 1) // 2 before taking the mean
SORTERS = ('torch', 'library')


def _sorter(sorter) -> bool:
    """True for the library's sort and compaction, False for torch's; anything else is refused."""
    if sorter not in SORTERS:
        raise RuntimeError(f"sorter: expected 'torch' or 'library', got {sorter!r}")
    return sorter == 'library'


def _ratio(numerator, denominator):
    """numpy's float64 division: x / 0 = inf, 0 / 0 = nan, silently."""
    with numpy.errstate(divide='ignore', invalid='ignore'):
        return numpy.float64(numerator) / numpy.float64(denominator)


def _psnr(mse):
    with numpy.errstate(divide='ignore', invalid='ignore'):
        return 10 * numpy.log10(255 ** 2 / numpy.float64(mse))


def image_metrics(eval_image: Tensor, gt_image: Tensor, mask: Optional[Tensor] = None) -> Dict[str, float]:
    """RMSE, PSNR and SSIM of a uint8 (h,w,3) frame against its ground truth, both on the GPU; with a bool (h,w) ``mask`` also
    MaskedRMSE, MaskedPSNR, MaskedSSIM (an all-false mask gives nan).  Identical images give PSNR = inf."""
    gt, image, mask, h, w = ops._image_pair(gt_image, eval_image, mask)
    if min(h, w) < ops.SSIM_WINDOW:
        raise RuntimeError(f'gt_image: the {ops.SSIM_WINDOW}-tap SSIM window exceeds the image extent {h} x {w}: every side must '
                           f'be at least {ops.SSIM_WINDOW}')
    errors = ops.image_error_sums(gt, image, mask)
    ssim = ops.ssim_sums(gt, image)
    if mask is not None:
        ssim = torch.cat([ssim, ops.ssim_sums(gt, image, mask)])
    errors, ssim = errors.cpu().numpy(), ssim.cpu().numpy()     # 3 + (2 or 4) scalars cross to the host
    mse = _ratio(int(errors[0]), h * w * 3)
    out = {'RMSE': float(numpy.sqrt(mse)), 'PSNR': float(_psnr(mse)),
           'SSIM': float(_ratio(ssim[0], 3 * (h - 2 * SSIM_CROP) * (w - 2 * SSIM_CROP)))}
    if mask is not None:
        kept = 3 * int(errors[2])
        mse = _ratio(int(errors[1]), kept)
        out.update({'MaskedRMSE': float(numpy.sqrt(mse)), 'MaskedPSNR': float(_psnr(mse)), 'MaskedSSIM': float(_ratio(ssim[3], kept))})
    return out


def ssim_map(eval_image: Tensor, gt_image: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """The whole SSIM map S, float64 (h,w,3) on the device, border included (of (gt, where(mask, eval, gt)) with a mask)."""
    return ops.ssim_sums(gt_image, eval_image, mask, return_map=True)[1]


def _srocc(x: Tensor, y: Tensor, library: bool = False) -> Optional[Tensor]:
    """Rank-correlation sums of two flat fp32 device tensors (None when they are empty)."""
    if x.numel() == 0:
        return None
    if library:
        return ops.rank_correlation_sums(x, y, ops.sort_values(x), ops.sort_values(y))
    return ops.rank_correlation_sums(x, y, torch.sort(x).values, torch.sort(y).values)


def _correlation(sums) -> float:
    """numpy.corrcoef's normalisation (scipy.stats.spearmanr): cov / std_x / std_y, clipped to [-1, 1]; nan for a constant side."""
    if sums is None:
        return float('nan')
    with numpy.errstate(divide='ignore', invalid='ignore'):
        r = numpy.float64(sums[0]) / numpy.sqrt(numpy.float64(sums[1])) / numpy.sqrt(numpy.float64(sums[2]))
    return float(numpy.clip(r, -1.0, 1.0))


def depth_metrics(eval_depth: Tensor, gt_depth: Tensor, eval_scale: float = 1.0, gt_scale: float = 1.0,
                  mask: Optional[Tensor] = None, sorter: str = 'torch') -> Dict[str, float]:
    """DepthRMSE, DepthMAE (normalised by the median of the scaled ground truth) and DepthSROCC of an fp32 (h,w) depth map, both
    on the GPU; with a bool (h,w) ``mask`` also the Masked* forms (an all-false mask gives nan).  ``eval_scale`` / ``gt_scale``:
    the reference's per-side factors (get_depth_scale), applied before anything else.  ``sorter``: 'torch' sorts and selects the
    masked pixels with torch ops, 'library' with the HIP library's (``ops.sort_values``, ``ops.compact_pair``); the metrics are the
    same values either way."""
    library = _sorter(sorter)
    gt = ops._typed(gt_depth, 'gt_depth', (torch.float32,))
    if gt.dim() != 2 or gt.numel() < 1:
        raise RuntimeError(f'gt_depth: expected a non-empty shape (h, w), got {tuple(gt.shape)}')
    depth = ops._typed(eval_depth, 'eval_depth', (torch.float32,), tuple(gt.shape))
    if mask is not None:
        mask = ops._typed(mask, 'mask', (torch.bool, torch.uint8), tuple(gt.shape))
    gt_flat, eval_flat = gt.reshape(-1), depth.reshape(-1)
    sort = ops.sort_values if library else (lambda values: torch.sort(values).values)
    sorted_gt = sort(gt_flat)
    pieces = [ops.depth_error_sums(gt, depth, gt_scale, eval_scale, None, sorted_gt),
              ops.rank_correlation_sums(gt_flat, eval_flat, sorted_gt, sort(eval_flat))]
    masked_ranks = None
    if mask is not None:
        pieces.append(ops.depth_error_sums(gt, depth, gt_scale, eval_scale, mask))
        if library:
            masked_ranks = _srocc(*ops.compact_pair(gt_flat, eval_flat, mask.reshape(-1)), library=True)
        else:
            keep = mask.reshape(-1).bool()
            masked_ranks = _srocc(gt_flat[keep], eval_flat[keep])
        if masked_ranks is not None:
            pieces.append(masked_ranks)
    sums = torch.cat(pieces).cpu().numpy()                      # at most 14 scalars cross to the host
    n, median = gt.numel(), sums[3]
    out = {'DepthRMSE': float(numpy.sqrt(_ratio(sums[1], n))), 'DepthMAE': float(_ratio(_ratio(sums[0], n), median)),
           'DepthSROCC': _correlation(sums[4:7])}
    if mask is not None:
        kept = sums[9]
        out.update({'MaskedDepthRMSE': float(numpy.sqrt(_ratio(sums[8], kept))),
                    'MaskedDepthMAE': float(_ratio(_ratio(sums[7], kept), median)),
                    'MaskedDepthSROCC': _correlation(None if masked_ranks is None else sums[11:14])})
    return out


# ---------------------------------------------------------------------------------------------------------------
# the masks of the masked metrics (the reference's src/qa/00_Common/src/mask_generators)
def _matrices(value, name: str, shape) -> numpy.ndarray:
    """A camera matrix argument (numpy or tensor, any float type) as float64 on the host, shape checked."""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    array = numpy.asarray(value)
    if array.dtype.kind != 'f':
        raise RuntimeError(f'{name}: expected a floating-point matrix, got {array.dtype}')
    if array.shape != tuple(shape):
        raise RuntimeError(f'{name}: expected shape {tuple(shape)}, got {array.shape}')
    return array.astype(numpy.float64)


def visibility_cameras(extrinsics_train, extrinsic_test, intrinsics_train, intrinsic_test=None) -> numpy.ndarray:
    """The (T,30) float64 table ``ops.visibility_mask_project`` takes, inverted and composed on the host as the reference's
    ``compute_transformed_points`` does: per view inv(K_train) | rows 0..2 of E_test inv(E_train) | K_test (the training view's own
    intrinsic without ``intrinsic_test``).  Extrinsics are 4x4 world-to-camera, intrinsics 3x3."""
    views = len(extrinsics_train)
    e_train = _matrices(extrinsics_train, 'extrinsics_train', (views, 4, 4))
    e_test = _matrices(extrinsic_test, 'extrinsic_test', (4, 4))
    k_train = _matrices(intrinsics_train, 'intrinsics_train', (e_train.shape[0], 3, 3))
    k_test = None if intrinsic_test is None else _matrices(intrinsic_test, 'intrinsic_test', (3, 3))
    table = numpy.empty((e_train.shape[0], ops.VISIBILITY_CAMERA), dtype=numpy.float64)
    for v in range(e_train.shape[0]):
        table[v, 0:9] = numpy.linalg.inv(k_train[v]).reshape(-1)
        table[v, 9:21] = numpy.matmul(e_test, numpy.linalg.inv(e_train[v]))[:3].reshape(-1)
        table[v, 21:30] = (k_train[v] if k_test is None else k_test).reshape(-1)
    return table


def visibility_mask(depth_train: Tensor, depth_test: Tensor, extrinsics_train, extrinsic_test, intrinsics_train, intrinsic_test=None,
                    depth_error_threshold: float = 0.05, min_views: int = 2, return_views: bool = False, sorter: str = 'torch'):
    """The mask of the reference's masked metrics, computed on the device: a test pixel is visible from a training view when that
    view's depth, splatted into the test view (``Warper.forward_warp``: bilinear proximity x depth weight 1 / exp(50 L / max L)),
    lands on it and agrees with ``depth_test`` to ``depth_error_threshold`` x the view's largest depth (``MaskComputer.compute_mask``);
    the mask holds where at least ``min_views`` training views see the pixel (the scripts' ``numpy.sum(masks, axis=0) > 1``).

    ``depth_train`` float32 (T,h,w) and ``depth_test`` float32 (h,w) on the GPU, z-depths in the extrinsics' units (divide by the
    scene's translation scale first, as the reference's script does); extrinsics (T,4,4) / (4,4) world-to-camera and intrinsics
    (T,3,3) / (3,3), numpy or tensor -- without ``intrinsic_test`` every training view's own intrinsic is used.  Train and test views
    share one resolution.  Returns the bool (h,w) mask on the device; ``return_views``: (mask, per-view masks bool (T,h,w), warped
    depths float64 (T,h,w), weight sums float64 (T,h,w)).  Arithmetic is fp64 and free of atomics: the same input gives the same bits.
    As in the reference a point behind the test camera still splats (with the largest depth weight) and no image is warped; a source
    whose projection is not finite, and a view whose depths give max L = 0, add nothing (undefined in the reference).
    ``sorter``: the stable sort of the splat keys -- 'torch' (``torch.sort(stable=True)``) or 'library' (``ops.sort_keys_with_order``
    over just the bits the keys of this frame use); the stable order is unique, so the outputs are the same bits either way."""
    library = _sorter(sorter)
    depth_train = ops._typed(depth_train, 'depth_train', (torch.float32,))
    if depth_train.dim() != 3 or depth_train.numel() < 1:
        raise RuntimeError(f'depth_train: expected a non-empty shape (views, h, w), got {tuple(depth_train.shape)}')
    views, h, w = (int(s) for s in depth_train.shape)
    depth_test = ops._typed(depth_test, 'depth_test', (torch.float32,), (h, w))
    if isinstance(min_views, bool) or int(min_views) != min_views or not 1 <= int(min_views) <= views:
        raise RuntimeError(f'min_views: expected 1..{views} (the number of training views), got {min_views}')
    if not float(depth_error_threshold) >= 0.0:
        raise RuntimeError(f'depth_error_threshold: expected a non-negative number, got {depth_error_threshold}')
    cameras = visibility_cameras(_matrices(extrinsics_train, 'extrinsics_train', (views, 4, 4)), extrinsic_test,
                                 _matrices(intrinsics_train, 'intrinsics_train', (views, 3, 3)), intrinsic_test)
    points, keys, stats = ops.visibility_mask_project(depth_train, torch.from_numpy(cameras).to(depth_train.device))
    if library:     # (every key is below views * keys per view: project's layout, ops._visibility_extent)
        key_bits = max(1, (views * ops._visibility_extent(views, h, w, 'depth_train') - 1).bit_length())
        sorted_keys, order = ops.sort_keys_with_order(keys.reshape(-1), key_bits)
    else:
        sorted_keys, order = torch.sort(keys.reshape(-1), stable=True)     # every list in ascending source order
    starts = ops.visibility_mask_list_starts(sorted_keys, views, h, w)
    gathered = ops.visibility_mask_gather(points, order, starts, stats, depth_test, depth_error_threshold, return_views)
    mask_views = gathered[0] if return_views else gathered
    mask = ops.visibility_mask_combine(mask_views, int(min_views))
    return (mask, mask_views.bool(), gathered[1], gathered[2]) if return_views else mask


# ---------------------------------------------------------------------------------------------------------------
# the reference's Warper as a utility of its own (src/qa/00_Common/src/mask_generators/Warper.py): csrc/warp.hip
def _splat_index(keys: Tensor, h: int, w: int, library: bool):
    """(order, starts) of one frame's splat keys: the stable sort (torch's or the library's) and the list starts."""
    if library:
        key_bits = max(1, (ops._visibility_extent(1, h, w, 'keys') - 1).bit_length())
        sorted_keys, order = ops.sort_keys_with_order(keys.reshape(-1), key_bits)
    else:
        sorted_keys, order = torch.sort(keys.reshape(-1), stable=True)     # every list in ascending source order
    return order, ops.visibility_mask_list_starts(sorted_keys, 1, h, w)


def forward_warp(frame1: Tensor, depth1: Tensor, extrinsic1, extrinsic2, intrinsic1, intrinsic2=None, mask1: Optional[Tensor] = None,
                 sorter: str = 'torch'):
    """``Warper.forward_warp`` on the device: view 1's frame and depth splatted into view 2 (bilinear proximity x depth weight
    1 / exp(50 L / max L), L = log(1 + clip(Z, 0, 1000)) of the transformed depth Z).

    ``frame1`` uint8 (h,w,3) and ``depth1`` float32 (h,w) on the GPU, ``mask1`` bool (h,w) on the GPU or None (pixels where it is false
    are ignored); extrinsics (4,4) world-to-camera and intrinsics (3,3), numpy or tensor (``intrinsic2`` None: ``intrinsic1``).
    Returns, on the device, ``(warped_frame2 uint8 (h,w,3), mask2 bool (h,w), warped_depth2 float64 (h,w), flow12 float64 (h,w,2))``:
    the colour clipped to [0, 255] and rounded half to even, True where something landed, the splatted Z (0 elsewhere), and the
    flow (q0 / q2 - x, q1 / q2 - y) of every pixel of view 1.  The two splats share one projection, one sort and one list-start
    pass; ``warped_depth2`` and ``mask2`` are, bit for bit, what ``visibility_mask`` computes for the same view (without a ``mask1``).
    Arithmetic is fp64 and free of atomics: the same input gives the same bits.  As in the reference a point behind camera 2 still
    splats, with the largest weight, and max L is taken over every pixel, masked ones included.  Not pinned by the reference
    (undefined there) and given no contribution here: a source whose projection is not finite or leaves int32, and a view whose
    depths give max L = 0.  ``sorter``: as for ``visibility_mask``; the outputs are the same bits either way."""
    library = _sorter(sorter)
    frame1, h, w, c = ops._warp_frame(frame1, 'frame1', True)
    if c != 3:
        raise RuntimeError(f'frame1: expected shape (h, w, 3), got {tuple(frame1.shape)}')
    depth1 = ops._typed(depth1, 'depth1', (torch.float32,), (h, w))
    mask1 = ops._warp_mask(mask1, 'mask1', h, w)
    ops._warp_together(frame1.device, depth1=depth1, mask1=mask1)
    cameras = visibility_cameras(_matrices(extrinsic1, 'extrinsic1', (4, 4))[None], _matrices(extrinsic2, 'extrinsic2', (4, 4)),
                                 _matrices(intrinsic1, 'intrinsic1', (3, 3))[None],
                                 None if intrinsic2 is None else _matrices(intrinsic2, 'intrinsic2', (3, 3)))
    points, keys, stats, flow12 = ops.warp_project(depth1, torch.from_numpy(cameras[0]).to(depth1.device), mask1)
    order, starts = _splat_index(keys, h, w, library)
    warped_frame2, mask2 = ops.warp_splat_gather(points, order, starts, stats, frame1, is_image=True)
    warped_depth2, _ = ops.warp_splat_gather(points, order, starts, stats, points[0, 2].unsqueeze(-1))     # Z splats itself
    return warped_frame2, mask2, warped_depth2[:, :, 0], flow12


def bilinear_splatting(frame1: Tensor, depth1: Tensor, flow12: Tensor, mask1: Optional[Tensor] = None,
                       flow12_mask: Optional[Tensor] = None, is_image: bool = False, sorter: str = 'torch'):
    """``Warper.bilinear_splatting`` on the device: ``frame1`` (h,w,c), c in 1..4, splatted along ``flow12`` float64 (h,w,2) with the
    depth weights of ``depth1`` float32 or float64 (h,w) -- every source adds its value to the (up to) four cells around
    (x + flow_x, y + flow_y).  ``mask1`` / ``flow12_mask`` bool (h,w) or None: a source where either is false adds nothing, but still
    counts in max L, as in the reference.  ``is_image``: ``frame1`` is uint8 and so is the result (clipped to [0, 255], rounded half
    to even); without it ``frame1`` is float32 or float64 and the result float64.  Returns ``(warped (h,w,c), mask2 bool (h,w))`` on
    the device: sum v weight / sum weight where something landed, else 0.  fp64, no atomics, the same bits on every call; the
    positions are numpy's bit for bit.  A float32 ``depth1`` is widened first (handed one, the reference computes its depth weights in
    float32; ``forward_warp``'s own depth is float64).  Not pinned by the reference (undefined there) and given no contribution here: a source
    whose position or depth is not finite or leaves int32, and a ``depth1`` whose max L is 0.  ``sorter``: as for
    ``visibility_mask``."""
    library = _sorter(sorter)
    frame1, h, w, _ = ops._warp_frame(frame1, 'frame1', bool(is_image))
    depth1 = ops._typed(depth1, 'depth1', (torch.float32, torch.float64), (h, w))
    flow12 = ops._typed(flow12, 'flow12', (torch.float64,), (h, w, 2))
    mask1 = ops._warp_mask(mask1, 'mask1', h, w)
    flow12_mask = ops._warp_mask(flow12_mask, 'flow12_mask', h, w)
    ops._warp_together(frame1.device, depth1=depth1, flow12=flow12, mask1=mask1, flow12_mask=flow12_mask)
    points, keys, stats = ops.warp_positions_from_flow(flow12, depth1, mask1, flow12_mask)
    order, starts = _splat_index(keys, h, w, library)
    return ops.warp_splat_gather(points, order, starts, stats, frame1, is_image=bool(is_image))


def bilinear_interpolation(frame2: Tensor, flow12: Tensor, mask2: Optional[Tensor] = None, flow12_mask: Optional[Tensor] = None,
                           is_image: bool = False):
    """``Warper.bilinear_interpolation`` on the device, the backward warp: pixel (x, y) of the result reads ``frame2`` (h,w,c), c in
    1..4, at (x + flow_x, y + flow_y) (``flow12`` float64 (h,w,2)) through four bilinear taps of the frame padded by one cell of
    zeros; ``mask2`` bool (h,w) or None marks the known pixels of ``frame2``, ``flow12_mask`` the valid flows.  dtypes and
    ``is_image`` as for ``bilinear_splatting``.  Returns ``(warped (h,w,c), mask1 bool (h,w))`` on the device: nr / dr where the
    weight dr of the known taps is positive, else 0.  Every pixel is independent and the operations keep the reference's order, so
    the float64 result is numpy's bit for bit.  Not pinned by the reference (undefined there): a pixel whose position is not finite
    or leaves int32 reads nothing (0, mask False); with ``is_image`` a NaN value is stored as 0."""
    return ops.warp_interpolate(frame2, flow12, mask2, flow12_mask, bool(is_image))


# ---------------------------------------------------------------------------------------------------------------
# LPIPS (the reference's src/qa/04_LPIPS, 14_MaskedLPIPS: lpips.LPIPS(net='alex') on the 8-bit frames)
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)      # the package's ScalingLayer buffers
_LPIPS_CONV_KEYS = {'lpips': ('net.slice1.0', 'net.slice2.3', 'net.slice3.6', 'net.slice4.8', 'net.slice5.10'),
                    'torchvision': ('features.0', 'features.3', 'features.6', 'features.8', 'features.10')}
# VGG-16: torchvision's `features` indices of the thirteen convolutions; the package's slices keep those indices
_VGG_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_VGG_SLICES = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
_LPIPS_VGG_CONV_KEYS = {'lpips': tuple(f'net.slice{s}.{i}' for s, i in zip(_VGG_SLICES, _VGG_FEATURES)),
                        'torchvision': tuple(f'features.{i}' for i in _VGG_FEATURES)}


def lpips_tensors(state_dict, lin_state_dict=None, net: str = 'alex') -> Dict[str, object]:
    """The tensors of LPIPS-alex (5 + 5 + 5) or LPIPS-vgg (13 + 13 + 5) and the scaling layer's buffers out of checkpoint
    dictionaries, identified by name: {'conv_weights': [5 | 13], 'conv_biases': [5 | 13], 'lin_weights': [5] as (c_out,),
    'shift': (3,), 'scale': (3,)}, float32 on the host.  ``net`` chooses the network; it is never guessed from the file.

    ``state_dict``: a saved ``lpips.LPIPS(net='alex').state_dict()`` (``net.slice{1..5}.{0,3,6,8,10}.*``, ``lin{k}.model.1.weight``,
    ``scaling_layer.*``) or torchvision's AlexNet (``features.{0,3,6,8,10}.*``; classifier keys are ignored).  ``lin_state_dict``: the
    package's ``alex.pth`` (``lin{k}.model.1.weight`` only), needed with torchvision's file and overriding otherwise.  A missing or
    mis-shaped tensor raises with its key; ``scaling_layer.shift`` / ``.scale``, where present, replace the package's constants.

    ``net='vgg'``: a saved ``lpips.LPIPS(net='vgg').state_dict()`` -- its convolutions are ``net.slice1.{0,2}``, ``net.slice2.{5,7}``,
    ``net.slice3.{10,12,14}``, ``net.slice4.{17,19,21}``, ``net.slice5.{24,26,28}`` (the slices keep torchvision's indices), plus
    ``lin{0..4}.model.1.weight`` and ``scaling_layer.*`` -- or torchvision's ``vgg16`` (``features.N.weight`` / ``.bias`` for N in
    0 2 5 7 10 12 14 17 19 21 24 26 28; ``classifier.*`` is ignored) with the package's ``vgg.pth`` as ``lin_state_dict``.  This
    key layout is written from the packages' published definitions; neither package was at hand to load a real file.  A file
    of the other network fails on its first tensor, by name or by shape."""
    convs, tap_convs = ops._lpips_net(net)[3:5]
    for name, value in (('state_dict', state_dict), ('lin_state_dict', lin_state_dict)):
        if not (value is None and name == 'lin_state_dict') and not hasattr(value, 'keys'):
            raise RuntimeError(f'{name}: expected a dictionary of tensors (a state dict), got {type(value).__name__}')
    conv_keys = _LPIPS_CONV_KEYS if net == 'alex' else _LPIPS_VGG_CONV_KEYS
    layout = next((name for name, keys in conv_keys.items() if any(k.startswith(keys[0] + '.') for k in state_dict.keys())), None)
    if layout is None:
        raise RuntimeError(f"state_dict: neither a saved lpips.LPIPS(net='{net}') state dict (no key 'net.slice1.0.weight') nor "
                           f"torchvision's {'AlexNet' if net == 'alex' else 'vgg16'} (no key 'features.0.weight')")

    def take(source, key, shape):
        if key not in source:
            raise RuntimeError(f'{key}: missing from the checkpoint')
        value = source[key]
        if not isinstance(value, torch.Tensor) or tuple(value.shape) != tuple(shape):
            got = tuple(value.shape) if isinstance(value, torch.Tensor) else type(value).__name__
            raise RuntimeError(f'{key}: expected a tensor of shape {tuple(shape)}, got {got}')
        return value.detach().to('cpu', torch.float32).contiguous()

    out: Dict[str, object] = {'conv_weights': [], 'conv_biases': [], 'lin_weights': []}
    for l, (c_out, c_in, k) in enumerate(convs):
        prefix = conv_keys[layout][l]
        out['conv_weights'].append(take(state_dict, prefix + '.weight', (c_out, c_in, k, k)))
        out['conv_biases'].append(take(state_dict, prefix + '.bias', (c_out,)))
        if l not in tap_convs:
            continue
        t = tap_convs.index(l)
        lin_key = f'lin{t}.model.1.weight'
        lin_source = lin_state_dict if lin_state_dict is not None else state_dict
        if lin_key not in lin_source and f'lins.{t}.model.1.weight' in lin_source:
            lin_key = f'lins.{t}.model.1.weight'
        out['lin_weights'].append(take(lin_source, lin_key, (1, c_out, 1, 1)).reshape(c_out))
    for name, default in (('shift', LPIPS_SHIFT), ('scale', LPIPS_SCALE)):
        key = f'scaling_layer.{name}'
        if key in state_dict:
            value = state_dict[key]
            if not isinstance(value, torch.Tensor) or value.numel() != 3:
                got = tuple(value.shape) if isinstance(value, torch.Tensor) else type(value).__name__
                raise RuntimeError(f'{key}: expected a tensor of 3 values, got {got}')
            out[name] = value.detach().to('cpu', torch.float32).reshape(3)
        else:
            out[name] = torch.tensor(default, dtype=torch.float32)
    return out


class LpipsWeights:
    """The weights of LPIPS-alex or LPIPS-vgg, packed once for the device kernels (``ops.lpips_pack``); pass it to ``lpips_metrics``
    / ``harness.evaluate_frames(lpips_weights=...)``.  ``tensors``: what ``lpips_tensors`` returned for the same ``net``, which
    ``.net`` keeps."""

    def __init__(self, tensors: Dict[str, object], device='cuda', net: str = 'alex'):
        ops._lpips_net(net)
        self.net = net
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        move = lambda group: [t.to(self.device) for t in group]
        self.packed = ops.lpips_pack(move(tensors['conv_weights']), move(tensors['conv_biases']), move(tensors['lin_weights']),
                                     tensors['shift'], tensors['scale'], net=net)

    @classmethod
    def from_state_dict(cls, state_dict, lin_state_dict=None, device='cuda', net: str = 'alex') -> 'LpipsWeights':
        return cls(lpips_tensors(state_dict, lin_state_dict, net), device, net)

    @classmethod
    def load(cls, path, lin_path=None, device='cuda', net: str = 'alex') -> 'LpipsWeights':
        """``path``: torchvision's AlexNet checkpoint (then ``lin_path`` is the package's ``alex.pth``) or a saved
        ``lpips.LPIPS(net='alex').state_dict()``; with ``net='vgg'`` torchvision's ``vgg16-397923af.pth`` (then ``lin_path`` is the
        package's ``vgg.pth``) or a saved ``lpips.LPIPS(net='vgg').state_dict()``.  Plain ``torch.save``d dictionaries of tensors,
        read with ``weights_only=True``."""
        state = torch.load(path, map_location='cpu', weights_only=True)
        lin_state = None if lin_path is None else torch.load(lin_path, map_location='cpu', weights_only=True)
        return cls.from_state_dict(state, lin_state, device, net)


def lpips_metrics(eval_image: Tensor, gt_image: Tensor, weights: LpipsWeights, mask: Optional[Tensor] = None) -> Dict[str, float]:
    """LPIPS (version 0.1, on the backbone of ``weights.net``: AlexNet or VGG-16) of a uint8 (h,w,3) frame against its ground truth,
    both on the GPU; with a bool (h,w) ``mask`` also MaskedLPIPS, the score of (gt, where(mask, eval, gt)) -- exactly 0 for an
    all-false mask, as in the reference."""
    gt, image, mask, h, w = ops._image_pair(gt_image, eval_image, mask)
    net = weights.net if isinstance(weights, LpipsWeights) else 'alex'
    _, name, min_extent = ops._lpips_net(net)[:3]
    if min(h, w) < min_extent:
        raise RuntimeError(f'gt_image: {name} needs {min_extent} pixels on every side, the image extent is {h} x {w}')
    if not isinstance(weights, LpipsWeights):
        raise RuntimeError(f'weights: expected qa.LpipsWeights, got {type(weights).__name__}')
    sums = ops.lpips_sums(gt, image, weights.packed, net=net)
    if mask is not None:
        sums = torch.cat([sums, ops.lpips_sums(gt, image, weights.packed, mask, net=net)])
    sums = sums.cpu().numpy()                                   # 5 or 10 scalars cross to the host
    pixels = [th * tw for th, tw, _ in ops.lpips_tap_shapes(h, w, net)]
    score = lambda layer_sums: float(sum(numpy.float64(s) / n for s, n in zip(layer_sums, pixels)))
    out = {'LPIPS': score(sums[:5])}
    if mask is not None:
        out['MaskedLPIPS'] = score(sums[5:])
    return out


# ---------------------------------------------------------------------------------------------------------------
# the reference's bookkeeping (compute_avg_* of every src/qa script): merged_data.round(4) per frame, numpy.mean of the
# rounded values, numpy.round(., 4) of the mean
def round4(value: float) -> float:
    """numpy.round(value, 4) -- what pandas' DataFrame.round applies: rint(value * 1e4) / 1e4, halves to even."""
    return float(numpy.round(numpy.float64(value), 4))


def summarise(rows: Iterable[Dict[str, float]]) -> Dict[str, object]:
    """``rows``: per-frame {'frame_num': ., metric: value, ...} -> {'frames': the rows with every metric rounded to 4 decimals,
    'average': {metric: round4(mean of the rounded values)}} over the frames that carry the metric."""
    frames: List[Dict[str, float]] = []
    for row in rows:
        frames.append({k: (v if k == 'frame_num' else round4(v)) for k, v in row.items()})
    names: List[str] = []
    for row in frames:
        names += [k for k in row if k != 'frame_num' and k not in names]
    average = {name: round4(numpy.mean([row[name] for row in frames if name in row])) for name in names}
    return {'frames': frames, 'average': average}
