"""Plain numpy restatement of the reference's Warper (src/qa/00_Common/src/mask_generators/Warper.py): ``forward_warp``,
``bilinear_splatting`` and ``bilinear_interpolation``, in the role tests/mask_reference.py has for the masks: the CPU tests hold it
to the fixtures the reference itself produced (tests/golden/warp_*.npz), and it serves the GPU tests for cases without a fixture.
Everything is float64 on inputs widened first.

Kept as the reference has it: floor and ceil are taken before the position is clipped; an integer coordinate adds all four corner
weights (each 1) to one cell; a point behind the second camera (Z < 0) splats with the largest depth weight; a masked source adds
nothing yet counts in max L; the backward warp adds its four taps in the order nw, sw, ne, se.  Different on purpose: a float32
``depth1`` is widened first, where the reference's ``bilinear_splatting`` would compute its depth weights in float32 (the fixtures hand
the reference the widened depth; ``forward_warp``'s own transformed depth is float64 on both sides).  Not pinned by the reference (its
astype('int') and 0 / 0 are undefined there) and given no contribution here: a source or a backward-warped pixel whose position is not
finite or leaves int32, a source whose depth is not finite, and every source of a depth whose largest log-depth is 0."""
import os

import numpy

from tests import mask_reference

INT_LIMIT = mask_reference.INT_LIMIT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VIEW = 1        # the view whose flow the fixtures' float splat and backward warps use (tools/make_golden_warp.py)


def _grid(h, w):
    ys, xs = numpy.mgrid[0:h, 0:w].astype(numpy.float64)
    return xs, ys


def positions(flow12):
    """-> padded positions X, Y (h,w) float64 of a (h,w,2) flow: (flow + grid) + 1, in that order."""
    flow12 = numpy.asarray(flow12, dtype=numpy.float64)
    xs, ys = _grid(*flow12.shape[:2])
    return (flow12[..., 0] + xs) + 1.0, (flow12[..., 1] + ys) + 1.0


def _pinned(*coordinates):
    with numpy.errstate(invalid='ignore'):
        out = numpy.ones(coordinates[0].shape, dtype=bool)
        for v in coordinates:
            out &= numpy.isfinite(v) & (numpy.abs(v) < INT_LIMIT)
    return out


def _image(values):
    return numpy.round(numpy.clip(numpy.where(numpy.isnan(values), 0.0, values), 0.0, 255.0)).astype(numpy.uint8)


def _corners(x, y, h, w):
    """Clipped corner cells and proximity weights of pinned positions, in the order nw, sw, ne, se: [(row, col, prox)]."""
    fx, cx = numpy.clip(numpy.floor(x), 0, w + 1), numpy.clip(numpy.ceil(x), 0, w + 1)
    fy, cy = numpy.clip(numpy.floor(y), 0, h + 1), numpy.clip(numpy.ceil(y), 0, h + 1)
    x, y = numpy.clip(x, 0, w + 1), numpy.clip(y, 0, h + 1)
    return ((fy, fx, (1 - (y - fy)) * (1 - (x - fx))), (cy, fx, (1 - (cy - y)) * (1 - (x - fx))),
            (fy, cx, (1 - (y - fy)) * (1 - (cx - x))), (cy, cx, (1 - (cy - y)) * (1 - (cx - x))))


def bilinear_splatting(frame1, depth1, flow12, mask1=None, flow12_mask=None, is_image=False, return_weights=False):
    """-> (warped (h,w,c) float64 -- uint8 with ``is_image`` --, mask2 bool (h,w)); ``return_weights``: also the weight sums (h,w)."""
    frame = numpy.asarray(frame1).astype(numpy.float64)
    h, w, c = frame.shape
    z = numpy.asarray(depth1).astype(numpy.float64)
    x, y = positions(flow12)
    keep = _pinned(x, y) & numpy.isfinite(z)
    for mask in (mask1, flow12_mask):
        if mask is not None:
            keep &= numpy.asarray(mask).astype(bool)
    with numpy.errstate(invalid='ignore'):
        log_depth = numpy.log(1.0 + numpy.clip(z, 0.0, 1000.0))
    top = numpy.max(numpy.where(numpy.isnan(log_depth), 0.0, log_depth))          # over every pixel, masked ones included
    sums = numpy.zeros(((h + 2) * (w + 2), c))
    ws = numpy.zeros((h + 2) * (w + 2))
    if top > 0.0 and keep.any():
        x, y, values, log_depth = x[keep], y[keep], frame[keep], log_depth[keep]      # row-major: ascending source order
        divisor = numpy.exp(log_depth / top * 50.0)
        for row, col, prox in _corners(x, y, h, w):
            cell = (row * (w + 2) + col).astype(numpy.int64)
            weight = prox / divisor
            for ch in range(c):
                sums[:, ch] += numpy.bincount(cell, values[:, ch] * weight, minlength=ws.size)
            ws += numpy.bincount(cell, weight, minlength=ws.size)
    sums, ws = sums.reshape(h + 2, w + 2, c)[1:-1, 1:-1], ws.reshape(h + 2, w + 2)[1:-1, 1:-1]
    mask2 = ws > 0
    with numpy.errstate(divide='ignore', invalid='ignore'):
        warped = numpy.where(mask2[..., None], sums / ws[..., None], 0.0)
    if is_image:
        warped = _image(warped)
    return (warped, mask2, ws) if return_weights else (warped, mask2)


def flow_of(depth1, extrinsic1, extrinsic2, intrinsic1, intrinsic2=None):
    """-> (flow12 (h,w,2), transformed depth Z (h,w)) of ``Warper.forward_warp``: q / q2 minus the pixel grid, and q2 -- the projection
    of ``mask_reference.project`` (whose positions are ``positions(flow12)``), operation for operation."""
    depth = numpy.asarray(depth1).astype(numpy.float64)
    h, w = depth.shape
    k1 = numpy.asarray(intrinsic1, dtype=numpy.float64)
    k2 = k1 if intrinsic2 is None else numpy.asarray(intrinsic2, dtype=numpy.float64)
    transform = numpy.asarray(extrinsic2, dtype=numpy.float64) @ numpy.linalg.inv(numpy.asarray(extrinsic1, dtype=numpy.float64))
    xs, ys = _grid(h, w)
    rays = numpy.einsum('ij,hwj->hwi', numpy.linalg.inv(k1), numpy.stack([xs, ys, numpy.ones_like(xs)], -1))
    moved = numpy.einsum('ij,hwj->hwi', transform[:3, :3], rays * depth[..., None]) + transform[:3, 3]
    q = numpy.einsum('ij,hwj->hwi', k2, moved)
    with numpy.errstate(divide='ignore', invalid='ignore'):
        flow12 = numpy.stack([q[..., 0] / q[..., 2] - xs, q[..., 1] / q[..., 2] - ys], -1)
    return flow12, q[..., 2]


def forward_warp(frame1, depth1, extrinsic1, extrinsic2, intrinsic1, intrinsic2=None, mask1=None):
    """-> (warped_frame2 uint8 (h,w,3), mask2 bool (h,w), warped_depth2 float64 (h,w), flow12 float64 (h,w,2))."""
    flow12, z = flow_of(depth1, extrinsic1, extrinsic2, intrinsic1, intrinsic2)
    warped_frame2, mask2 = bilinear_splatting(frame1, z, flow12, mask1, None, is_image=True)
    warped_depth2 = bilinear_splatting(z[..., None], z, flow12, mask1, None)[0][..., 0]
    return warped_frame2, mask2, warped_depth2, flow12


def bilinear_interpolation(frame2, flow12, mask2=None, flow12_mask=None, is_image=False):
    """-> (warped (h,w,c) float64 -- uint8 with ``is_image`` --, mask1 bool (h,w)).  Each product and sum is the reference's, in its
    order: (prox x flow12_mask) x frame2 x mask2 per tap, the taps added nw, sw, ne, se."""
    frame = numpy.asarray(frame2)
    h, w, c = frame.shape
    known = numpy.ones((h, w), dtype=bool) if mask2 is None else numpy.asarray(mask2).astype(bool)
    valid = numpy.ones((h, w), dtype=bool) if flow12_mask is None else numpy.asarray(flow12_mask).astype(bool)
    x, y = positions(flow12)
    pinned = _pinned(x, y)
    x, y = numpy.where(pinned, x, 0.0), numpy.where(pinned, y, 0.0)
    padded = numpy.pad(frame, ((1, 1), (1, 1), (0, 0))).astype(numpy.float64)
    padded_known = numpy.pad(known, ((1, 1), (1, 1))).astype(numpy.float64)
    nr, dr = None, None
    with numpy.errstate(invalid='ignore'):
        for row, col, prox in _corners(x, y, h, w):
            row, col = row.astype(numpy.int64), col.astype(numpy.int64)
            weight = (prox * valid)[..., None]
            tap_known = padded_known[row, col][..., None]
            term, weight_known = weight * padded[row, col] * tap_known, weight * tap_known
            nr, dr = (term, weight_known) if nr is None else (nr + term, dr + weight_known)
        dr = numpy.where(pinned[..., None], dr, 0.0)
        with numpy.errstate(divide='ignore'):
            warped = numpy.where(dr > 0, nr / dr, 0.0)
    mask1 = dr[..., 0] > 0
    if is_image:
        warped = _image(warped)
    return warped, mask1


# ---------------------------------------------------------------------------------------------------------------
# the gates of the fixtures and of the device
TIE_BAND = 1e-9


def near_tie(unrounded):
    """Values whose rounding to uint8 a 1e-9 change could move: within TIE_BAND of k + 0.5."""
    clipped = numpy.clip(unrounded, 0.0, 255.0)
    return numpy.abs(numpy.abs(clipped - numpy.floor(clipped)) - 0.5) <= TIE_BAND


def relative(got, want, where=None):
    """Largest |got - want| / |want| over ``where`` (everywhere by default); 0 where both are 0."""
    got, want = numpy.asarray(got, dtype=numpy.float64), numpy.asarray(want, dtype=numpy.float64)
    error = numpy.abs(got - want) / numpy.maximum(numpy.abs(want), 1e-300)
    error = numpy.where(got == want, 0.0, error)
    if where is not None:
        error = numpy.where(where, error, 0.0)
    return float(error.max()) if error.size else 0.0


def flow_deviation(got, want):
    """Largest |got - want| / max(1, |want + grid|) of a (h,w,2) flow: the issue's gate is 1e-12 of it."""
    xs, ys = _grid(*want.shape[:2])
    scale = numpy.maximum(1.0, numpy.abs(want + numpy.stack([xs, ys], -1)))
    return float((numpy.abs(got - want) / scale).max())


def colour_difference(got, want, unrounded):
    """(values differing outside the tie band, largest difference inside it) of two uint8 frames."""
    band = near_tie(unrounded)
    difference = numpy.abs(got.astype(numpy.int64) - want.astype(numpy.int64))
    return int((difference[~band] != 0).sum()), int(difference[band].max()) if band.any() else 0


# ---------------------------------------------------------------------------------------------------------------
# inputs the CPU and the GPU tests share
def fixture(case, shape):
    with numpy.load(os.path.join(GOLDEN, f'warp_{case}_{shape[0]}x{shape[1]}.npz')) as data:
        return {k: data[k] for k in data.files}


def small_case(c, h=19, w=23):
    """The case without a fixture of the GPU tests: a flow with a block of exactly integer positions, a band off every side of the
    frame and a few non-finite entries; masks with holes.  -> dict of numpy inputs."""
    rng = numpy.random.RandomState(100 * c + h)
    flow = rng.uniform(-2.5, 2.5, (h, w, 2))
    flow[4:9, 5:11] = numpy.round(flow[4:9, 5:11])               # integer positions: four weights of 1 on one cell
    flow[4:9, 5:11, 0] = 2.0                                     # ... several of them on the same cell's neighbours
    flow[:, 0, 0] -= 6.0                                         # off the left side
    flow[:, -1, 0] += 6.0                                        # off the right
    flow[0, :, 1] -= 6.0                                         # off the top
    flow[-1, :, 1] += 6.0                                        # off the bottom
    flow[2, 3, 0], flow[10 % h, 12 % w, 1], flow[11 % h, 2, 0], flow[12 % h, 20 % w, 1] = numpy.nan, numpy.inf, -numpy.inf, 1e300
    return {'flow12': flow, 'frame': rng.uniform(-3.0, 9.0, (h, w, c)), 'image': rng.randint(0, 256, (h, w, c)).astype(numpy.uint8),
            'depth1': rng.uniform(0.5, 9.0, (h, w)).astype(numpy.float32), 'mask1': rng.random_sample((h, w)) > 0.15,
            'flow12_mask': rng.random_sample((h, w)) > 0.15}
