"""Host restatement of the reference's frame metrics (src/qa/<NN>_<Metric>/src/<Metric>02_NeRF_LLFF.py, compute_frame_* /
compute_depth_*): numpy for the one-line formulas, scipy.ndimage.gaussian_filter in float64 for what skimage's
``structural_similarity(gt, eval, multichannel=True, gaussian_weights=True, sigma=1.5, use_sample_covariance=False)`` computes
on uint8 input (data_range 255, truncate 3.5 -> 11 taps, mode 'reflect', crop of 5 before the mean), scipy.stats.spearmanr
for SROCC.  skimage is not a dependency: SSIM is pinned to THIS restatement, which tests/test_qa_host.py in turn holds to the
closed form for constant images.  The depth functions take the depths as float64 with the scales already applied."""
import numpy
from scipy.ndimage import gaussian_filter
from scipy.stats import spearmanr

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
PAD = 5


def ssim_map(gt, image):
    """S per channel, float64 (h,w,3), border included."""
    if min(gt.shape[:2]) < 11:
        raise ValueError('win_size exceeds image extent')
    out = numpy.empty(gt.shape, dtype=numpy.float64)
    blur = lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5, mode='reflect')
    for c in range(gt.shape[2]):
        x, y = gt[..., c].astype(numpy.float64), image[..., c].astype(numpy.float64)
        ux, uy = blur(x), blur(y)
        uxx, uyy, uxy = blur(x * x), blur(y * y), blur(x * y)
        vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
        a1, a2, b1, b2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
        out[..., c] = (a1 * a2) / (b1 * b2)
    return out


def image_metrics(image, gt, mask=None):
    error = gt.astype('float') - image.astype('float')
    with numpy.errstate(divide='ignore', invalid='ignore'):
        mse = numpy.mean(numpy.square(error))
        out = {'RMSE': numpy.sqrt(numpy.mean(numpy.square(error))), 'PSNR': 10 * numpy.log10(255 ** 2 / mse)}
        s = ssim_map(gt, image)
        out['SSIM'] = numpy.mean([s[PAD:-PAD, PAD:-PAD, c].mean(dtype=numpy.float64) for c in range(3)])
        if mask is not None:
            mask_3d = numpy.stack([mask] * 3, axis=2)
            mse = numpy.sum(numpy.square(mask_3d * error)) / numpy.sum(mask_3d)
            out['MaskedRMSE'] = numpy.sqrt(numpy.sum(numpy.square(mask_3d * error)) / numpy.sum(mask_3d))
            out['MaskedPSNR'] = 10 * numpy.log10(255 ** 2 / mse)
            masked_image = mask_3d * image + (~mask_3d) * gt
            out['MaskedSSIM'] = numpy.sum(mask_3d * ssim_map(gt, masked_image)) / numpy.sum(mask_3d)
    return {k: float(v) for k, v in out.items()}


def error_sums(image, gt, mask=None):
    """The exact integers behind RMSE / PSNR: (sum of squared differences, the same on the mask, masked pixel count)."""
    sq = numpy.square(gt.astype(numpy.int64) - image.astype(numpy.int64)).sum(axis=2)
    if mask is None:
        return int(sq.sum()), 0, 0
    return int(sq.sum()), int(sq[mask].sum()), int(mask.sum())


def depth_metrics(depth, gt, eval_scale=1.0, gt_scale=1.0, mask=None):
    """``depth``, ``gt``: float32 (h,w); cast to float64 before the scales are applied."""
    gt = gt.astype(numpy.float64) * gt_scale
    depth = depth.astype(numpy.float64) * eval_scale
    with numpy.errstate(divide='ignore', invalid='ignore'):
        error = gt - depth
        scaled_error = gt / numpy.median(gt) - depth / numpy.median(gt)
        out = {'DepthRMSE': numpy.sqrt(numpy.mean(numpy.square(error))), 'DepthMAE': numpy.mean(numpy.abs(scaled_error)),
               'DepthSROCC': spearmanr(gt.ravel(), depth.ravel()).correlation}
        if mask is not None:
            out['MaskedDepthRMSE'] = numpy.sqrt(numpy.sum(numpy.square(mask * error)) / numpy.sum(mask))
            out['MaskedDepthMAE'] = numpy.sum(numpy.abs(mask * scaled_error)) / numpy.sum(mask)
            out['MaskedDepthSROCC'] = spearmanr(gt[mask], depth[mask]).correlation if mask.any() else numpy.nan
    return {k: float(v) for k, v in out.items()}


# tolerances of the comparison with the device (both sides fp64): SSIM 1e-9 absolute (the variance's cancellation amplifies
# rounding by <= 2 * 65025 / 58.5 ~ 2e3, x ~22 additions x 1.1e-16 ~ 1e-11 per pixel), depth sums 1e-12 relative, SROCC 1e-10
def assert_close(got: dict, want: dict, names=None):
    import math
    assert set(got) == set(want), set(got) ^ set(want)
    for name in (names or want):
        g, w = got[name], want[name]
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) and math.isnan(w)) or g == w, (name, g, w)
        elif name in ('RMSE', 'PSNR', 'MaskedRMSE', 'MaskedPSNR'):
            assert g == w, (name, g, w)
        elif name in ('SSIM', 'MaskedSSIM'):
            assert abs(g - w) <= 1e-9, (name, g, w)
        elif name.endswith('SROCC'):
            assert abs(g - w) <= 1e-10, (name, g, w)
        else:
            assert abs(g - w) <= 1e-12 * abs(w), (name, g, w)
