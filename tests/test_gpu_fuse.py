"""The point-cloud export on a real MI355X: ``geometry.fuse_depth_maps`` and ``geometry.voxel_thin`` against the numpy restatement of
tests/fuse_reference.py (tests/test_fuse_host.py pins that one, and shows that no decision of the analytic scene is marginal, so the
kept set is compared exactly).  Positions are equal or adjacent float32 values: both sides round fp64 results that differ by a few
units of 2^-53 at the most, so the tolerance is one float32 ulp of the coordinate -- derived, not measured.  The thinning sums in a
prescribed order and is compared bit for bit."""
import numpy
import pytest
import torch

from simplenerf_amd import geometry, harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import fuse_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def on_device(array):
    return torch.from_numpy(numpy.array(array)).to(DEV)          # (a copy: the shared scene is read-only)


def fuse(depth, image, extrinsics, intrinsics, tau=0.02, min_views=1, mask=None):
    """-> (points, colours, views) numpy arrays of one geometry.fuse_depth_maps call; dtypes and shapes checked."""
    points, colours, views = geometry.fuse_depth_maps(on_device(depth), on_device(image), extrinsics, intrinsics, tau, min_views,
                                                      None if mask is None else on_device(mask))
    n = points.shape[0]
    assert points.dtype == torch.float32 and tuple(points.shape) == (n, 3) and points.is_cuda
    assert colours.dtype == torch.uint8 and tuple(colours.shape) == (n, 3)
    assert views.dtype == torch.uint8 and tuple(views.shape) == (n,)
    return points.cpu().numpy(), colours.cpu().numpy(), views.cpu().numpy()


def assert_adjacent(got, want):
    """Equal or neighbouring float32 values, element by element."""
    assert got.shape == want.shape and got.dtype == want.dtype == numpy.float32
    ok = (got == want) | (numpy.nextafter(got, want) == want)
    assert ok.all(), (got[~ok][:4], want[~ok][:4])


def assert_equals_restatement(depth, image, extrinsics, intrinsics, tau, min_views, mask=None):
    """The device against the restatement, leaving out nothing: the caller's case has no marginal decision (checked here)."""
    margins = {}
    want_points, want_colours, want_views, sources = ref.fuse_depth_maps(depth, image, extrinsics, intrinsics, tau, min_views, mask, margins)
    assert all(m['threshold'] >= 1e-9 and m['tie'] >= 1e-9 for m in margins.values())
    points, colours, views = fuse(depth, image, extrinsics, intrinsics, tau, min_views, mask)
    assert len(points) == len(want_points)
    assert numpy.array_equal(colours, want_colours) and numpy.array_equal(views, want_views)     # the kept set, its order, the counts
    assert_adjacent(points, want_points)
    return points, colours, views, sources


# ------------------------------------------------------------------------------------------------------------------ the scene
@pytest.mark.parametrize('tau', [0.02, 0.05])
@pytest.mark.parametrize('min_views', [1, 2])
def test_scene_equals_the_restatement(tau, min_views):
    s = ref.scene()
    want_points, want_colours, want_views = ref.scene_expected(tau, min_views)[:3]
    points, colours, views = fuse(s['depth'], s['image'], s['extrinsics'], s['intrinsics'], tau, min_views)
    assert len(points) == {1: 577, 2: 372}[min_views]
    assert numpy.array_equal(colours, want_colours) and numpy.array_equal(views, want_views)
    assert_adjacent(points, want_points)


def test_two_calls_and_permuted_other_views_give_the_same_bits():
    s = ref.scene()
    first = fuse(s['depth'], s['image'], s['extrinsics'], s['intrinsics'])
    again = fuse(s['depth'], s['image'], s['extrinsics'], s['intrinsics'])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    swapped = [0, 2, 1]
    other = fuse(s['depth'][swapped], s['image'][swapped], s['extrinsics'][swapped], s['intrinsics'][swapped])
    sources = ref.scene_expected(0.02, 1)[3]
    of_view0 = int((sources[:, 0] == 0).sum())
    assert of_view0 == 178
    for a, b in zip(first, other):
        assert a[:of_view0].tobytes() == b[:of_view0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ smallest shapes
def test_one_view_keeps_every_valid_pixel_and_refuses_min_views_1():
    s = ref.scene()
    depth = s['depth'][:1].copy()
    depth[0, 0, 0], depth[0, 5, 9], depth[0, 12, 16] = 0.0, numpy.nan, -1.0
    points, colours, views, sources = assert_equals_restatement(depth, s['image'][:1], s['extrinsics'][:1], s['intrinsics'][:1], 0.02, 0)
    assert len(points) == 13 * 17 - 3 and not views.any()
    with pytest.raises(RuntimeError, match='min_views'):
        fuse(depth, s['image'][:1], s['extrinsics'][:1], s['intrinsics'][:1], 0.02, 1)


def test_one_by_one_frames():
    """Two cameras one unit apart whose single pixels look along z: the point of view 0 at depth 4 projects to x = -5 in view 1 with
    f = 20 (outside), so nothing agrees; with f = 0.4 it rounds to pixel 0 and the depths agree."""
    depth = numpy.full((2, 1, 1), 4.0, dtype=numpy.float32)
    image = numpy.array([[[[1, 2, 3]]], [[[4, 5, 6]]]], dtype=numpy.uint8)
    poses = [ref.camera_to_world((0.0, 0.0, 0.0), 0.0), ref.camera_to_world((1.0, 0.0, 0.0), 0.0)]
    extrinsics = numpy.stack([numpy.linalg.inv(p) for p in poses])
    for f, kept in ((20.0, 0), (0.4, 2)):
        intrinsics = numpy.stack([ref.intrinsic_of(1, 1, f)] * 2)
        points, colours, views, _ = assert_equals_restatement(depth, image, extrinsics, intrinsics, 0.02, 1)
        assert len(points) == kept
    points = fuse(depth, image, extrinsics, intrinsics, 0.02, 0)[0]
    assert points.tolist() == [[0.0, 0.0, 4.0], [1.0, 0.0, 4.0]]


@pytest.mark.parametrize('shape', [(13, 17), (5, 65)])
def test_widths_that_are_no_multiple_of_the_wave(shape):
    h, w = shape
    s = ref.scene(h, w, 20.0 * w / 17)
    assert_equals_restatement(s['depth'], s['image'], s['extrinsics'], s['intrinsics'], 0.02, 1)


def test_compaction_across_scan_blocks():
    """3 x 70 x 130 = 27 300 pixels are 14 tiles of 2048: the kept set and its order against a vectorised numpy evaluation of the rule
    (the looped restatement takes a minute at this size; the vectorised one is held to it on the small scene first)."""
    small = ref.scene()
    keep_small, points_small, views_small = ref.fuse_depth_maps_vectorised(small, 0.02, 1)
    want = ref.scene_expected(0.02, 1)
    assert int(keep_small.sum()) == 577 and numpy.array_equal(views_small, want[2])
    assert_adjacent(points_small, want[0])
    s = ref.scene(70, 130, 147.0)
    depth = s['depth'].copy()
    depth[:, ::7, ::5] = 0.0                                          # holes: kept pixels are not whole rows
    scene = dict(s, depth=depth)
    keep, want_points, want_views = ref.fuse_depth_maps_vectorised(scene, 0.02, 1)
    points, colours, views = fuse(depth, s['image'], s['extrinsics'], s['intrinsics'], 0.02, 1)
    assert 2048 * 4 < len(points) == int(keep.sum()) < 27300
    assert numpy.array_equal(colours, s['image'][keep]) and numpy.array_equal(views, want_views)
    assert_adjacent(points, want_points)


def test_all_pixels_invalid_gives_an_empty_cloud(tmp_path):
    s = ref.scene()
    depth = numpy.zeros_like(s['depth'])
    points, colours, views = fuse(depth, s['image'], s['extrinsics'], s['intrinsics'], 0.02, 0)
    assert points.shape == (0, 3) and colours.shape == (0, 3) and views.shape == (0,)
    geometry.save_ply(tmp_path / 'empty.ply', points, colours)
    assert (tmp_path / 'empty.ply').read_bytes().endswith(b'element vertex 0\nproperty float x\nproperty float y\nproperty float z\n'
                                                          b'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
    empty = fuse(numpy.zeros((3, 0, 17), numpy.float32), numpy.zeros((3, 0, 17, 3), numpy.uint8), s['extrinsics'], s['intrinsics'])
    assert [len(a) for a in empty] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ decision cases
def test_invalid_depths_are_neither_kept_nor_counted():
    """0, a negative depth, NaN and +inf: not sources, and a point that lands on one finds no agreement there."""
    s = ref.scene()
    depth = s['depth'].copy()
    depth[0, 2, 3], depth[0, 6, 8], depth[1, 6, 8], depth[1, 3, 3], depth[2, 9, 12] = 0.0, -5.0, numpy.nan, numpy.inf, -numpy.inf
    depth[1, 5:8, 6:10] = numpy.nan                                    # a block of witnesses of views 0 and 2
    points, colours, views, sources = assert_equals_restatement(depth, s['image'], s['extrinsics'], s['intrinsics'], 0.02, 1)
    kept = {tuple(source) for source in sources.tolist()}
    assert not kept & {(0, 2, 3), (0, 6, 8), (1, 6, 8), (1, 3, 3), (2, 9, 12), (1, 6, 7)}
    baseline = ref.scene_expected(0.02, 1)
    assert len(points) < len(baseline[0]) - 12                          # the block also took agreement away from other views
    assert numpy.isfinite(points).all()


def test_a_view_turned_round_never_agrees():
    """View 2 turned by 180 degrees about y: every point of views 0 and 1 is behind it (c_z <= 0) and its own points are behind them."""
    s = ref.scene()
    extrinsics = s['extrinsics'].copy()
    extrinsics[2] = numpy.linalg.inv(ref.camera_to_world((1.0, 0.2, 0.0), numpy.pi))
    points, colours, views, sources = assert_equals_restatement(s['depth'], s['image'], extrinsics, s['intrinsics'], 0.02, 1)
    assert set(sources[:, 0].tolist()) == {0, 1} and views.max() == 1
    assert len(fuse(s['depth'], s['image'], extrinsics, s['intrinsics'], 0.02, 2)[0]) == 0


def test_a_projection_outside_the_frame_and_a_degenerate_one():
    """View 1 moved 50 units sideways: every projection between it and the others leaves the frame.  A view whose intrinsic is all
    zeros projects to 0 / 0: it never agrees and nothing faults."""
    s = ref.scene()
    extrinsics = s['extrinsics'].copy()
    extrinsics[1] = numpy.linalg.inv(ref.camera_to_world((50.0, 0.1, 0.0), 0.0))
    points, colours, views, sources = assert_equals_restatement(s['depth'], s['image'], extrinsics, s['intrinsics'], 0.02, 1)
    assert set(sources[:, 0].tolist()) == {0, 2}
    table = geometry.fuse_cameras(s['extrinsics'], s['intrinsics'])
    table[1, 33:42] = 0.0
    got = [t.cpu().numpy() for t in ops.fuse_depth_maps(on_device(s['depth']), on_device(s['image']), on_device(table), 0.02, 1)]
    # nobody agrees with view 1, so the records of views 0 and 2 are those of the two-view fuse without it (view 1's own in between)
    pair = [0, 2]
    two = assert_equals_restatement(s['depth'][pair], s['image'][pair], s['extrinsics'][pair], s['intrinsics'][pair], 0.02, 1)
    of_view0 = int((two[3][:, 0] == 0).sum())
    of_view2 = len(two[0]) - of_view0
    assert of_view0 > 0 and of_view2 > 0 and len(got[0]) >= len(two[0])
    for three, both in zip(got, two[:3]):
        assert three[:of_view0].tobytes() == both[:of_view0].tobytes() and three[len(three) - of_view2:].tobytes() == both[of_view0:].tobytes()


def test_different_intrinsics_per_view():
    s = ref.scene()
    intrinsics = s['intrinsics'].copy()
    intrinsics[1] = ref.intrinsic_of(13, 17, 16.0)
    intrinsics[2, 0, 2] += 0.75
    poses = [numpy.linalg.inv(m) for m in s['extrinsics']]
    depth = numpy.stack([ref.plane_depths(poses[i], intrinsics[i], 13, 17) for i in range(3)]).astype(numpy.float32)
    points = assert_equals_restatement(depth, s['image'], s['extrinsics'], intrinsics, 0.02, 1)[0]
    assert len(points) > 300
    assert numpy.minimum(numpy.abs(points[:, 2] - 5.0), numpy.abs(points[:, 2] - 10.0)).max() < 2e-6


def test_the_mask():
    s = ref.scene()
    mask = numpy.ones(s['depth'].shape, dtype=numpy.uint8)
    mask[0, :, :5] = 0
    mask[1, 4:9, 4:12] = 0
    mask[2, 0, 0] = 0
    masked = assert_equals_restatement(s['depth'], s['image'], s['extrinsics'], s['intrinsics'], 0.02, 1, mask)
    assert 0 < len(masked[0]) < 577
    kept = {tuple(source) for source in masked[3].tolist()}
    assert not any(mask[v, y, x] == 0 for v, y, x in kept)
    as_bool = geometry.fuse_depth_maps(on_device(s['depth']), on_device(s['image']), s['extrinsics'], s['intrinsics'], 0.02, 1,
                                       on_device(mask.astype(bool)))
    assert as_bool[0].cpu().numpy().tobytes() == masked[0].tobytes()
    # a depth range is a mask
    window = (s['depth'] >= 4.0) & (s['depth'] <= 6.0)
    near = assert_equals_restatement(s['depth'], s['image'], s['extrinsics'], s['intrinsics'], 0.02, 1, window.astype(numpy.uint8))
    assert len(near[0]) > 50 and numpy.abs(near[0][:, 2] - 5.0).max() < 1e-6


def test_refusals():
    s = ref.scene()
    depth, image = on_device(s['depth']), on_device(s['image'])
    with pytest.raises(RuntimeError, match='min_views'):
        geometry.fuse_depth_maps(depth, image, s['extrinsics'], s['intrinsics'], 0.02, 3)
    with pytest.raises(RuntimeError, match='depth_error_threshold'):
        geometry.fuse_depth_maps(depth, image, s['extrinsics'], s['intrinsics'], -0.1)
    with pytest.raises(RuntimeError, match='depth_error_threshold'):
        geometry.fuse_depth_maps(depth, image, s['extrinsics'], s['intrinsics'], float('nan'))
    with pytest.raises(RuntimeError, match='image'):
        geometry.fuse_depth_maps(depth, image[:, :, :, :2], s['extrinsics'], s['intrinsics'])
    with pytest.raises(RuntimeError, match='depth'):
        geometry.fuse_depth_maps(depth.double(), image, s['extrinsics'], s['intrinsics'])
    with pytest.raises(RuntimeError, match='extrinsics'):
        geometry.fuse_depth_maps(depth, image, s['extrinsics'][:2], s['intrinsics'])
    with pytest.raises(RuntimeError, match='mask'):
        geometry.fuse_depth_maps(depth, image, s['extrinsics'], s['intrinsics'], mask=torch.ones((3, 13, 16), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.fuse_depth_maps(depth.cpu(), image, s['extrinsics'], s['intrinsics'])


# ------------------------------------------------------------------------------------------------------------------ the thinning
def thin(points, colours, voxel_size):
    out = geometry.voxel_thin(on_device(points), on_device(colours), voxel_size)
    m = out[0].shape[0]
    assert out[0].dtype == torch.float32 and tuple(out[0].shape) == (m, 3)
    assert out[1].dtype == torch.uint8 and tuple(out[1].shape) == (m, 3)
    assert out[2].dtype == torch.int32 and tuple(out[2].shape) == (m,)
    return tuple(t.cpu().numpy() for t in out)


def assert_thin_equals_restatement(points, colours, voxel_size):
    got = thin(points, colours, voxel_size)
    want = ref.voxel_thin(points, colours, voxel_size)
    assert got[0].tobytes() == want[0].tobytes()                        # positions bit for bit, in the restatement's order
    assert numpy.array_equal(got[1], want[1]) and numpy.array_equal(got[2], want[2])
    return got


def random_cloud(n, seed, extent=4.0):
    rng = numpy.random.default_rng(seed)
    return (rng.uniform(-extent, extent, (n, 3)).astype(numpy.float32), rng.integers(0, 256, (n, 3), dtype=numpy.uint8))


def test_thin_one_point():
    points, colours = numpy.array([[1.5, -2.25, 3.0]], numpy.float32), numpy.array([[9, 8, 255]], numpy.uint8)
    got = assert_thin_equals_restatement(points, colours, 0.1)
    assert got[0].tolist() == points.tolist() and got[1].tolist() == colours.tolist() and got[2].tolist() == [1]


def test_thin_all_points_in_one_voxel_and_a_run_longer_than_64():
    points, colours = random_cloud(300, 5)
    got = assert_thin_equals_restatement(points, colours, 100.0)
    assert got[2].tolist() == [300]
    # runs of ~40 and more than 64 side by side, across a tile boundary of 2048
    points, colours = random_cloud(5000, 6)
    got = assert_thin_equals_restatement(points, colours, 2.0)
    assert got[2].max() > 64 and got[2].sum() == 5000 and len(got[2]) == 64


def test_thin_every_point_in_its_own_voxel():
    grid = numpy.stack(numpy.meshgrid(numpy.arange(7), numpy.arange(5), numpy.arange(3), indexing='ij'), axis=-1).reshape(-1, 3)
    rng = numpy.random.default_rng(8)
    points = (grid[rng.permutation(len(grid))] * 0.5 + 0.125).astype(numpy.float32)
    colours = rng.integers(0, 256, (len(points), 3), dtype=numpy.uint8)
    got = assert_thin_equals_restatement(points, colours, 0.5)
    assert got[2].tolist() == [1] * 105
    order = numpy.lexsort((points[:, 0], points[:, 1], points[:, 2]))     # ascending key: z, then y, then x
    assert got[0].tobytes() == points[order].tobytes() and numpy.array_equal(got[1], colours[order])


def test_thin_the_fused_scene_and_an_empty_cloud():
    points, colours = ref.scene_expected(0.02, 1)[:2]
    got = assert_thin_equals_restatement(points, colours, ref.NATIVE_VOXEL)
    assert len(got[0]) == 147
    again = thin(points, colours, ref.NATIVE_VOXEL)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    empty = thin(numpy.zeros((0, 3), numpy.float32), numpy.zeros((0, 3), numpy.uint8), 1.0)
    assert [len(a) for a in empty] == [0, 0, 0]


def test_thin_refusals():
    points, colours = random_cloud(10, 9)
    bad = points.copy()
    bad[3, 1] = numpy.inf
    with pytest.raises(RuntimeError, match='not finite.*voxel_size'):
        thin(bad, colours, 1.0)
    bad[3, 1] = numpy.nan
    with pytest.raises(RuntimeError, match='not finite'):
        thin(bad, colours, 1.0)
    with pytest.raises(RuntimeError, match=r'voxel_size.*extents \d+ x \d+ x \d+'):
        thin(points, colours, 1e-3)                                       # ~8000^3 voxels
    for size in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='voxel_size'):
            thin(points, colours, size)
    with pytest.raises(RuntimeError, match='colours'):
        geometry.voxel_thin(on_device(points), on_device(colours[:5]), 1.0)
    lib_refusal = pytest.raises(RuntimeError, match='snerf_voxel_thin')
    with lib_refusal:                                                      # the library's own check of a caller's extents
        ops.voxel_thin(on_device(points), on_device(colours), 1.0, lo=(0.0, 0.0, 0.0), extents=(65536, 65536, 1))


# ------------------------------------------------------------------------------------------------------------------ the harness
def test_camera_matrices_agree_with_the_ray_generator():
    """inv(E)[:3] . [t . inv(K) . (x, y, 1); 1] against rays_o + t rays_d of harness.frame_batch, every pixel of an 11 x 7 camera, two
    values of t, to 16 float32 ulps of the largest coordinate (the rays are fp32; a wrong axis or pixel convention is off by about
    t / f, four orders of magnitude more)."""
    camera = synth.camera('fern', 1, resolution=(11, 7))
    extrinsic, intrinsic = geometry.camera_matrices(camera)
    batch = harness.frame_batch(camera, False, DEV)
    origins, directions = batch['rays_o'].cpu().numpy().astype(numpy.float64), batch['rays_d'].cpu().numpy().astype(numpy.float64)
    assert origins.shape == (77, 3)
    inverse, k_inverse = numpy.linalg.inv(extrinsic), numpy.linalg.inv(intrinsic)
    for t in (1.0, 7.5):
        for y in range(11):
            for x in range(7):
                point = ref.point_of(inverse, k_inverse, x, y, t)
                ray = origins[y * 7 + x] + t * directions[y * 7 + x]
                bound = 16 * numpy.spacing(numpy.float32(max(numpy.abs(point).max(), numpy.abs(ray).max())))
                assert numpy.abs(point - ray).max() <= bound, (t, y, x, point, ray)


def test_export_point_cloud(tmp_path):
    cfg = synth.make_configs('config1')
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 11, 150.0, 4.0).items()})
    model = model.to(DEV).eval()
    cameras = [synth.camera('fern', pose, resolution=(12, 15)) for pose in (0, 1, 2)]
    device = torch.device(DEV)
    out = harness.export_point_cloud(model, cfg, cameras, tmp_path / 'cloud.ply', device, depth_error_threshold=0.5, min_views=0)
    frames = [harness.predict_frame(model, cfg, camera, device) for camera in cameras]
    images, depths = numpy.stack([f['image'] for f in frames]), numpy.stack([f['depth'] for f in frames])
    assert numpy.array_equal(out['images_device'].cpu().numpy(), images)
    assert out['depths_device'].cpu().numpy().tobytes() == depths.tobytes()
    matrices = [geometry.camera_matrices(camera) for camera in cameras]
    want = geometry.fuse_depth_maps(on_device(depths), on_device(images), [m[0] for m in matrices], [m[1] for m in matrices], 0.5, 0)
    assert out['fused_points'] == want[0].shape[0] == int(((depths > 0) & numpy.isfinite(depths)).sum()) > 0
    for name, tensor in zip(('points', 'colours', 'counts'), want):
        assert out[name].cpu().numpy().tobytes() == tensor.cpu().numpy().tobytes(), name
    assert (tmp_path / 'cloud.ply').read_bytes() == geometry.ply_bytes(want[0], want[1])
    # a depth range masks, the thinning follows the fuse, an existing file is left alone
    low, high = float(numpy.float32(numpy.percentile(depths, 20))), float(numpy.float32(numpy.percentile(depths, 80)))
    ranged = harness.export_point_cloud(model, cfg, cameras, tmp_path / 'thin.ply', device, 0.5, 0, voxel_size=0.25, depth_range=(low, high))
    window = (depths >= low) & (depths <= high)
    fused = geometry.fuse_depth_maps(on_device(depths), on_device(images), [m[0] for m in matrices], [m[1] for m in matrices], 0.5, 0,
                                     on_device(window))
    assert ranged['fused_points'] == fused[0].shape[0] == int(window.sum())
    thinned = geometry.voxel_thin(fused[0], fused[1], 0.25)
    assert ranged['counts'].dtype == torch.int32 and int(ranged['counts'].sum()) == ranged['fused_points']
    for name, tensor in zip(('points', 'colours', 'counts'), thinned):
        assert ranged[name].cpu().numpy().tobytes() == tensor.cpu().numpy().tobytes(), name
    assert (tmp_path / 'thin.ply').read_bytes() == geometry.ply_bytes(thinned[0], thinned[1])
    harness.export_point_cloud(model, cfg, cameras[:2], tmp_path / 'cloud.ply', device, 0.5, 0)
    assert (tmp_path / 'cloud.ply').read_bytes() == geometry.ply_bytes(want[0], want[1])
