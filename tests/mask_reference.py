"""Plain numpy restatement of the reference's visibility masks (src/qa/00_Common/src/mask_generators: Warper.forward_warp,
MaskComputer.compute_mask, and the masked scripts' "visible in more than one training view"), in the role tests/qa_reference.py has
for the metrics: the CPU tests hold it to the fixtures the reference itself produced (tests/golden/visibility_mask_*.npz), and it
serves the GPU tests for cases without a fixture.  Everything is float64; depths come in as float32 and are widened first.

Kept as the reference has it: a point behind the test camera (Z < 0) splats with the largest depth weight; floor and ceil are taken
before the position is clipped; an integer coordinate adds all four corner weights (each 1) to one cell.  Not pinned by the reference
(its astype('int') and 0 / 0 are undefined there) and given no contribution here: a source whose position or depth is not finite or
leaves int32, and every source of a view whose largest log-depth is 0."""
import numpy

INT_LIMIT = 2147483000.0


def project(depth_train, extrinsic_train, extrinsic_test, intrinsic_train, intrinsic_test=None):
    """-> padded positions X, Y and transformed depth Z of every pixel of the (h,w) training depth, each (h,w) float64."""
    depth = numpy.asarray(depth_train).astype(numpy.float64)
    h, w = depth.shape
    k_train = numpy.asarray(intrinsic_train, dtype=numpy.float64)
    k_test = k_train if intrinsic_test is None else numpy.asarray(intrinsic_test, dtype=numpy.float64)
    transform = numpy.asarray(extrinsic_test, dtype=numpy.float64) @ numpy.linalg.inv(numpy.asarray(extrinsic_train, dtype=numpy.float64))
    ys, xs = numpy.mgrid[0:h, 0:w].astype(numpy.float64)
    rays = numpy.einsum('ij,hwj->hwi', numpy.linalg.inv(k_train), numpy.stack([xs, ys, numpy.ones_like(xs)], -1))
    points = rays * depth[..., None]
    moved = numpy.einsum('ij,hwj->hwi', transform[:3, :3], points) + transform[:3, 3]
    q = numpy.einsum('ij,hwj->hwi', k_test, moved)
    with numpy.errstate(divide='ignore', invalid='ignore'):
        # the reference turns the position into a flow (minus the pixel grid) and back before it adds the one-pixel pad
        x = ((q[..., 0] / q[..., 2] - xs) + xs) + 1.0
        y = ((q[..., 1] / q[..., 2] - ys) + ys) + 1.0
    return x, y, q[..., 2]


def splat(x, y, z):
    """-> (sum of Z weight, sum of weight), both (h,w) float64: the padded accumulators cropped by one cell per side."""
    h, w = z.shape
    with numpy.errstate(invalid='ignore'):
        pinned = numpy.isfinite(x) & numpy.isfinite(y) & numpy.isfinite(z) & (numpy.abs(x) < INT_LIMIT) & (numpy.abs(y) < INT_LIMIT)
        log_depth = numpy.log(1.0 + numpy.clip(z, 0.0, 1000.0))
    top = numpy.nanmax(numpy.where(numpy.isnan(log_depth), 0.0, log_depth))
    zw = numpy.zeros((h + 2) * (w + 2))
    ws = numpy.zeros((h + 2) * (w + 2))
    if top > 0.0 and pinned.any():
        x, y, z, log_depth = x[pinned], y[pinned], z[pinned], log_depth[pinned]      # row-major: ascending source order
        divisor = numpy.exp(log_depth / top * 50.0)
        fx, cx = numpy.clip(numpy.floor(x), 0, w + 1), numpy.clip(numpy.ceil(x), 0, w + 1)
        fy, cy = numpy.clip(numpy.floor(y), 0, h + 1), numpy.clip(numpy.ceil(y), 0, h + 1)
        x, y = numpy.clip(x, 0, w + 1), numpy.clip(y, 0, h + 1)
        for row, col, prox in ((fy, fx, (1 - (y - fy)) * (1 - (x - fx))), (cy, fx, (1 - (cy - y)) * (1 - (x - fx))),
                               (fy, cx, (1 - (y - fy)) * (1 - (cx - x))), (cy, cx, (1 - (cy - y)) * (1 - (cx - x)))):
            cell = (row * (w + 2) + col).astype(numpy.int64)
            weight = prox / divisor
            zw += numpy.bincount(cell, z * weight, minlength=zw.size)
            ws += numpy.bincount(cell, weight, minlength=ws.size)
    crop = lambda a: a.reshape(h + 2, w + 2)[1:-1, 1:-1]
    return crop(zw), crop(ws)


def warp(depth_train, extrinsic_train, extrinsic_test, intrinsic_train, intrinsic_test=None):
    """-> warping_mask bool (h,w), warped_depth float64 (h,w) (0 outside the mask), weight_sum float64 (h,w)."""
    zw, ws = splat(*project(depth_train, extrinsic_train, extrinsic_test, intrinsic_train, intrinsic_test))
    warping_mask = ws > 0
    with numpy.errstate(divide='ignore', invalid='ignore'):
        warped_depth = numpy.where(warping_mask, zw / ws, 0.0)
    return warping_mask, warped_depth, ws


def visibility_mask(depth_train, depth_test, extrinsics_train, extrinsic_test, intrinsics_train, intrinsic_test=None,
                    depth_error_threshold=0.05, min_views=2):
    """``depth_train`` (T,h,w) float32, ``depth_test`` (h,w) float32 -> {'mask' bool (h,w), 'mask_views' bool (T,h,w),
    'warping_mask' bool (T,h,w), 'warped_depth', 'weight_sum' float64 (T,h,w)}."""
    depth_test = numpy.asarray(depth_test).astype(numpy.float64)
    out = {'mask_views': [], 'warping_mask': [], 'warped_depth': [], 'weight_sum': []}
    for v in range(len(depth_train)):
        warping_mask, warped_depth, ws = warp(depth_train[v], extrinsics_train[v], extrinsic_test, intrinsics_train[v], intrinsic_test)
        # (fmax: a NaN depth is ignored by both maxima, as on the device; the reference's max would make the threshold NaN)
        threshold = float(depth_error_threshold) * float(numpy.fmax.reduce(numpy.asarray(depth_train[v], dtype=numpy.float64).reshape(-1)))
        out['mask_views'].append(warping_mask & (numpy.abs(warped_depth - depth_test) < threshold))
        out['warping_mask'].append(warping_mask)
        out['warped_depth'].append(warped_depth)
        out['weight_sum'].append(ws)
    out = {k: numpy.stack(v) for k, v in out.items()}
    out['mask'] = out['mask_views'].sum(0) >= int(min_views)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the gates of the fixtures and of the device (the issue's table): warped_depth to 1e-12 relative (1e-8 where a training view
# equals the test view: a coordinate that rounds across an integer moves a ~1e-13 weight to the neighbouring cell), warping_mask
# equal everywhere, the masks equal on every pixel that is not fragile
def fragile(warped_depth, depth_test, threshold):
    """Pixels whose depth error lies within 1e-9 x threshold of the threshold (``threshold``: per view, broadcastable)."""
    threshold = numpy.asarray(threshold, dtype=numpy.float64).reshape(-1, 1, 1)
    return numpy.abs(numpy.abs(warped_depth - numpy.asarray(depth_test, dtype=numpy.float64)) - threshold) <= 1e-9 * threshold


def compare(got, want, depth_test, thresholds, depth_tolerance, min_views=2):
    """``got`` / ``want``: dicts as ``visibility_mask`` returns ('weight_sum' optional).  -> the figures; asserts the gates."""
    assert numpy.array_equal(got['warping_mask'], want['warping_mask']), \
        f"warping_mask differs on {int((got['warping_mask'] != want['warping_mask']).sum())} pixels"
    scale = numpy.maximum(numpy.abs(want['warped_depth']), 1e-300)
    worst = float(numpy.max(numpy.where(want['warping_mask'], numpy.abs(got['warped_depth'] - want['warped_depth']) / scale, 0.0)))
    assert numpy.array_equal(got['warped_depth'][~want['warping_mask']], want['warped_depth'][~want['warping_mask']])   # zeros
    unsure = fragile(want['warped_depth'], depth_test, thresholds) & want['warping_mask']
    view_difference = int(((got['mask_views'] != want['mask_views']) & ~unsure).sum())
    # a combined pixel is unsure when some unsure view could move the count across min_views
    sure = (want['mask_views'] & ~unsure).sum(0)
    firm = (sure >= min_views) | (sure + unsure.sum(0) < min_views)
    mask_difference = int(((got['mask'] != want['mask']) & firm).sum())
    figures = {'warped_depth_relative': worst, 'mask_views_differing': view_difference, 'mask_differing': mask_difference,
               'fragile': int(unsure.sum())}
    assert worst <= depth_tolerance, figures
    assert view_difference == 0 and mask_difference == 0, figures
    return figures


# ---------------------------------------------------------------------------------------------------------------
# the analytic scene of the fixtures (tools/make_golden_masks.py) and of the cases without one: a slanted back plane
# z = 4 + 0.3 x + 0.2 y and a sphere (centre (0.15, -0.1, 2), radius 0.5) in front of it, so that views really occlude each other;
# cameras x right, y down, z forward, pinhole f = 0.9 w, z-depths ray-cast per view and stored as float32
SHAPES = ((24, 32), (37, 53), (64, 80))
CASES = ('generic', 'same_pose', 'behind')
PLANE = numpy.array([-0.3, -0.2, 1.0, 4.0])                  # n . p = 4
SPHERE = numpy.array([0.15, -0.1, 2.0, 0.5])


def _extrinsic(angles, position):
    """World-to-camera [R t; 0 1] of a camera at ``position`` rotated by ``angles`` (radians about x, y, z)."""
    (cx, sx), (cy, sy), (cz, sz) = ((numpy.cos(a), numpy.sin(a)) for a in angles)
    rx = numpy.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = numpy.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = numpy.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    pose = numpy.eye(4)
    pose[:3, :3] = rz @ ry @ rx
    pose[:3, 3] = position
    return numpy.linalg.inv(pose)


def ray_cast(extrinsic, intrinsic, h, w):
    """z-depth (h,w) float64 of the nearest surface along every pixel's ray (the plane is hit by every ray of these cameras)."""
    pose = numpy.linalg.inv(extrinsic)
    ys, xs = numpy.mgrid[0:h, 0:w].astype(numpy.float64)
    dirs = numpy.stack([xs, ys, numpy.ones_like(xs)], -1) @ numpy.linalg.inv(intrinsic).T @ pose[:3, :3].T     # camera z = 1
    origin = pose[:3, 3]
    depth = (PLANE[3] - PLANE[:3] @ origin) / (dirs @ PLANE[:3])
    rel = origin - SPHERE[:3]
    a, b, c = (dirs * dirs).sum(-1), 2 * dirs @ rel, rel @ rel - SPHERE[3] ** 2
    disc = b * b - 4 * a * c
    with numpy.errstate(invalid='ignore'):
        near = (-b - numpy.sqrt(disc)) / (2 * a)
    hit = (disc > 0) & (near > 0)
    return numpy.where(hit & (near < depth), near, depth)


def occlusion_scene(h, w, case='generic', seed=0):
    """-> {'depth_train' (3,h,w) float32, 'depth_test' (h,w) float32, 'extrinsics_train' (3,4,4), 'extrinsic_test' (4,4),
    'intrinsics_train' (3,3,3), 'intrinsic_test' (3,3)} (matrices float64).  'generic': three training views a few tenths of a unit
    and a few hundredths of a radian from the test view; 'same_pose': the first training view IS the test view (every coordinate an
    integer up to rounding); 'behind': the test camera moved forward past the sphere, whose points get Z < 0."""
    rng = numpy.random.RandomState(1000 * h + w + seed)
    k = numpy.array([[0.9 * w, 0, w / 2], [0, 0.9 * w, h / 2], [0, 0, 1]], dtype=numpy.float64)
    test = _extrinsic((0.0, 0.0, 0.0), (0.0, 0.0, 2.8 if case == 'behind' else 0.0))
    train = [_extrinsic(0.03 * rng.standard_normal(3), numpy.array([0.3, 0.2, 0.05]) * rng.standard_normal(3)) for _ in range(3)]
    if case == 'same_pose':
        train[0] = test.copy()
    return {'depth_train': numpy.stack([ray_cast(e, k, h, w) for e in train]).astype(numpy.float32),
            'depth_test': ray_cast(test, k, h, w).astype(numpy.float32), 'extrinsics_train': numpy.stack(train),
            'extrinsic_test': test, 'intrinsics_train': numpy.stack([k, k, k]), 'intrinsic_test': k.copy()}
