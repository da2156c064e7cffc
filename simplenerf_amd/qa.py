"""Frame metrics of the reference's QA stage (src/qa/*), evaluated on the device.

The reference scores the frames its Tester wrote with one script per metric (``compute_frame_*`` / ``compute_depth_*`` of
``src/qa/<NN>_<Metric>/src/<Metric>02_NeRF_LLFF.py``; the ``01_RealEstate`` siblings compute the same quantities), through
skimage, pandas and scipy on the host.  Here the frame never leaves the GPU: the HIP library reduces the uint8 image pair /
the fp32 depth pair to a handful of sums (exact int64 for the image errors, fp64 for everything else, fixed-order reductions --
csrc/metrics.hip) and the functions below evaluate the reference's expressions on those sums.  Sorting (for the median and the
ranks) and mask compaction are torch calls on the device.

SSIM is pinned to a restatement of skimage's ``structural_similarity(gt, eval, multichannel=True, gaussian_weights=True,
sigma=1.5, use_sample_covariance=False)`` on ``scipy.ndimage.gaussian_filter`` (tests/qa_reference.py), not to skimage itself.
The reference's scripts round scaled fp32 depths to fp32 before subtracting; here the scale is applied in fp64 (a difference
of ~1e-7, below their 4-decimal rounding).  LPIPS (04, 14) needs network weights and is not provided.
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


def _srocc(x: Tensor, y: Tensor) -> Optional[Tensor]:
    """Rank-correlation sums of two flat fp32 device tensors (None when they are empty)."""
    if x.numel() == 0:
        return None
    return ops.rank_correlation_sums(x, y, torch.sort(x).values, torch.sort(y).values)


def _correlation(sums) -> float:
    """numpy.corrcoef's normalisation (scipy.stats.spearmanr): cov / std_x / std_y, clipped to [-1, 1]; nan for a constant side."""
    if sums is None:
        return float('nan')
    with numpy.errstate(divide='ignore', invalid='ignore'):
        r = numpy.float64(sums[0]) / numpy.sqrt(numpy.float64(sums[1])) / numpy.sqrt(numpy.float64(sums[2]))
    return float(numpy.clip(r, -1.0, 1.0))


def depth_metrics(eval_depth: Tensor, gt_depth: Tensor, eval_scale: float = 1.0, gt_scale: float = 1.0,
                  mask: Optional[Tensor] = None) -> Dict[str, float]:
    """DepthRMSE, DepthMAE (normalised by the median of the scaled ground truth) and DepthSROCC of an fp32 (h,w) depth map, both
    on the GPU; with a bool (h,w) ``mask`` also the Masked* forms (an all-false mask gives nan).  ``eval_scale`` / ``gt_scale``:
    the reference's per-side factors (get_depth_scale), applied before anything else."""
    gt = ops._typed(gt_depth, 'gt_depth', (torch.float32,))
    if gt.dim() != 2 or gt.numel() < 1:
        raise RuntimeError(f'gt_depth: expected a non-empty shape (h, w), got {tuple(gt.shape)}')
    depth = ops._typed(eval_depth, 'eval_depth', (torch.float32,), tuple(gt.shape))
    if mask is not None:
        mask = ops._typed(mask, 'mask', (torch.bool, torch.uint8), tuple(gt.shape))
    gt_flat, eval_flat = gt.reshape(-1), depth.reshape(-1)
    sorted_gt = torch.sort(gt_flat).values
    pieces = [ops.depth_error_sums(gt, depth, gt_scale, eval_scale, None, sorted_gt),
              ops.rank_correlation_sums(gt_flat, eval_flat, sorted_gt, torch.sort(eval_flat).values)]
    masked_ranks = None
    if mask is not None:
        keep = mask.reshape(-1).bool()
        pieces.append(ops.depth_error_sums(gt, depth, gt_scale, eval_scale, mask))
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
