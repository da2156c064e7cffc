"""LPIPS on the VGG-16 backbone restated with torch CPU ops: what simplenerf_amd.qa.lpips_metrics is pinned to for ``net='vgg'``.

``lpips.LPIPS(net='vgg')`` -- version 0.1, lin layers on, eval mode (the dropout of the lin layers is inert), spatial=False --
called as ``model(im2tensor(gt), im2tensor(eval))`` with normalize=False.  The network:
  * scaling layer: (x - shift) / scale with the package's constants, as for AlexNet;
  * torchvision's ``vgg16().features``: convolutions at indices 0 2 | 5 7 | 10 12 14 | 17 19 21 | 24 26 28, all 3 x 3, stride 1,
    pad 1, each followed by a ReLU; channels 3->64 64->64 | 64->128 128->128 | 128->256 256->256 256->256 | 256->512 512->512
    512->512 | 512->512 512->512 512->512; ``MaxPool2d(2, 2)`` (floor mode, no padding) at indices 4, 9, 16, 23 (the one at 30 is
    not used);
  * five taps after the ReLUs of convolutions 2, 7, 14, 21, 28 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3): 64, 128, 256, 512,
    512 channels;
  * per tap n = f / (sqrt(sum_c f^2) + 1e-10), v = sum_c lin_c (n_gt - n_eval)^2, the layer score is the spatial mean of v and
    LPIPS the sum of the five layer scores; masked form: eval' = where(mask, eval, gt) on the bytes.
The smallest image is 16 x 16 (16 -> 8 -> 4 -> 2 -> 1).  Written from the published definitions; neither ``lpips`` nor
``torchvision`` is imported, and it has not been run against the packages.  ``dtype`` float64 is the oracle, float32 the precision
class of the package (which computes in float32).
"""
import functools

import numpy
import torch
import torch.nn.functional as F

from tests.lpips_reference import SCALE, SHIFT, im2tensor, random_images  # noqa: F401  (shared with the AlexNet restatement)

# (c_out, c_in, max-pool 2x2 s2 before the convolution, the tap its ReLU feeds or None) in the order of torchvision's `features`
CONVS = ((64, 3, False, None), (64, 64, False, 0), (128, 64, True, None), (128, 128, False, 1), (256, 128, True, None),
         (256, 256, False, None), (256, 256, False, 2), (512, 256, True, None), (512, 512, False, None), (512, 512, False, 3),
         (512, 512, True, None), (512, 512, False, None), (512, 512, False, 4))
FEATURE_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
TAP_CHANNELS = (64, 128, 256, 512, 512)
# image (h, w): the minimum, every pool down to 1 | odd extents: a floor-mode pool drops a row and a column at several levels, row
# and column tails | regular | several 128-row tiles in conv1 - conv4, a partial single tile in conv5
SHAPES = ((16, 16), (37, 53), (64, 80), (96, 131))
SEED = 20240611


def random_weights(seed=SEED):
    """conv uniform +-sqrt(6 / fan_in), bias uniform +-0.1, lin uniform [0, 1); float32, the layout qa.lpips_tensors returns."""
    rng = numpy.random.default_rng(seed)
    out = {'conv_weights': [], 'conv_biases': [], 'lin_weights': [], 'shift': torch.tensor(SHIFT, dtype=torch.float32),
           'scale': torch.tensor(SCALE, dtype=torch.float32)}
    for c_out, c_in, _, _ in CONVS:
        bound = numpy.sqrt(6.0 / (c_in * 9))
        out['conv_weights'].append(torch.from_numpy(rng.uniform(-bound, bound, (c_out, c_in, 3, 3)).astype(numpy.float32)))
        out['conv_biases'].append(torch.from_numpy(rng.uniform(-0.1, 0.1, (c_out,)).astype(numpy.float32)))
    for channels in TAP_CHANNELS:
        out['lin_weights'].append(torch.from_numpy(rng.uniform(0.0, 1.0, (channels,)).astype(numpy.float32)))
    return out


def taps(x, weights, dtype):
    """The five tapped post-ReLU activations of VGG-16's features for x (n,3,h,w), scaling layer included."""
    shift = weights['shift'].to(dtype).reshape(1, 3, 1, 1)
    scale = weights['scale'].to(dtype).reshape(1, 3, 1, 1)
    x = (x.to(dtype) - shift) / scale
    out = []
    for l, (_, _, pool, tap) in enumerate(CONVS):
        if pool:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        x = F.relu(F.conv2d(x, weights['conv_weights'][l].to(dtype), weights['conv_biases'][l].to(dtype), stride=1, padding=1))
        if tap is not None:
            assert tap == len(out)
            out.append(x)
    return out


def lpips(gt, image, weights, dtype=torch.float64, mask=None):
    """-> {'score', 'sums' [5]: per tap the sum over its pixels, 'layers' [5]: the layer scores (their means),
    'taps' [5]: (2, c, h_l, w_l), gt first}.  ``mask``: the masked form, eval = where(mask, eval, gt) on the uint8 pixels."""
    gt, image = numpy.asarray(gt), numpy.asarray(image)
    if min(gt.shape[:2]) < 16:
        raise ValueError(f'VGG-16 needs 16 pixels on every side, the image extent is {gt.shape[0]} x {gt.shape[1]}')
    if mask is not None:
        image = numpy.where(numpy.asarray(mask).astype(bool)[:, :, None], image, gt)
    features = taps(torch.cat([im2tensor(gt), im2tensor(image)]), weights, dtype)
    sums, layers = [], []
    for l, f in enumerate(features):
        norm = torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True))
        n = f / (norm + 1e-10)
        d = (n[0:1] - n[1:2]) ** 2
        v = F.conv2d(d, weights['lin_weights'][l].to(dtype).reshape(1, -1, 1, 1))       # the lin layer: 1x1, no bias, one output
        sums.append(float(v.sum()))
        layers.append(float(v.mean(dim=(2, 3)).reshape(())))
    score = layers[0]
    for value in layers[1:]:
        score = score + value
    return {'score': float(score), 'sums': sums, 'layers': layers, 'taps': features}


@functools.lru_cache(maxsize=None)
def host_weights():
    return random_weights()


@functools.lru_cache(maxsize=None)
def case(shape):
    """The seeded pair and mask of a shape with the float64 restatement's results, plain and masked: computed once per session and
    shared by the tests; nobody writes to it."""
    gt, image, mask = random_images(*shape)
    return {'gt': gt, 'image': image, 'mask': mask, 'plain': lpips(gt, image, host_weights()),
            'masked': lpips(gt, image, host_weights(), mask=mask)}


@functools.lru_cache(maxsize=None)
def precision_class(shapes=SHAPES):
    """How far the float32 restatement lies from the float64 one over ``shapes``: {'feature': max over taps of
    max|x32 - x64| / max|x64|, 'sum': max over layers of |s32 - s64| / |s64|, 'score': max |score32 - score64|}."""
    feature = total = score = 0.0
    for shape in shapes:
        c = case(shape)
        lo, hi = lpips(c['gt'], c['image'], host_weights(), torch.float32), c['plain']
        for a, b in zip(lo['taps'], hi['taps']):
            feature = max(feature, float((a.double() - b).abs().max() / b.abs().max()))
        for a, b in zip(lo['sums'], hi['sums']):
            total = max(total, abs(a - b) / abs(b))
        score = max(score, abs(lo['score'] - hi['score']))
    return {'feature': feature, 'sum': total, 'score': score}
