"""The mesh export on a real MI355X: ``geometry.tsdf_volume``, ``geometry.extract_mesh`` and ``geometry.colour_points`` against the
restatement of tests/mesh_reference.py (tests/test_mesh_host.py pins that one, and shows that no decision of the analytic scene is
marginal, so the volume is compared node for node).  Distances and positions are asked bit for bit: both sides evaluate the same
fp64 expressions in the same order, without contraction, with correctly rounded divisions.  What differs is printed; a difference of
more than one float32 ulp, or of sign, fails.  Counts, indices, orders, weights, colours and view counts are equal exactly."""
import ctypes

import numpy
import pytest
import torch

from simplenerf_amd import _lib, geometry, harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import mesh_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 1e-9


def on_device(array):
    return torch.from_numpy(numpy.array(array)).to(DEV)          # (a copy: the shared fixtures are read-only)


def assert_bits_or_one_ulp(got, want, what):
    """Bit for bit; what is not is printed, and may be one float32 ulp off, never of another sign."""
    assert got.shape == want.shape and got.dtype == want.dtype == numpy.float32, what
    differ = got.view(numpy.uint32) != want.view(numpy.uint32)
    if differ.any():
        print(f'{what}: {int(differ.sum())} of {differ.size} values differ, by up to {numpy.abs(got[differ] - want[differ]).max():.3e}')
    adjacent = (got == want) | (numpy.nextafter(got, want) == want)
    assert adjacent.all(), (what, got[~adjacent][:4], want[~adjacent][:4])
    assert numpy.array_equal(got < 0, want < 0), what


# ------------------------------------------------------------------------------------------------------------------ integrate
def integrate(depth, extrinsics, intrinsics, lo, voxel_size, extents, truncation, mask=None):
    tsdf, weight = geometry.tsdf_volume(on_device(depth), extrinsics, intrinsics, lo, voxel_size, extents, truncation,
                                        None if mask is None else on_device(mask))
    nx, ny, nz = extents
    assert tsdf.dtype == torch.float32 and tuple(tsdf.shape) == (nz, ny, nx) and tsdf.is_cuda
    assert weight.dtype == torch.uint8 and tuple(weight.shape) == (nz, ny, nx)
    return tsdf.cpu().numpy(), weight.cpu().numpy()


def assert_volume_equals_restatement(depth, extrinsics, intrinsics, lo, voxel_size, extents, truncation, mask=None, leave_out=0):
    """The device against the restatement; a node may be left out only when one of its decisions lies within 1e-9 of a tie or of -mu,
    at most ``leave_out`` of them."""
    margins = {}
    want_tsdf, want_weight = ref.tsdf_integrate(depth, extrinsics, intrinsics, lo, voxel_size, extents, truncation, mask, margins)
    marginal = (margins['tie'] < MARGIN) | (margins['behind'] < MARGIN)
    assert int(marginal.sum()) <= leave_out
    tsdf, weight = integrate(depth, extrinsics, intrinsics, lo, voxel_size, extents, truncation, mask)
    assert numpy.array_equal(weight[~marginal], want_weight[~marginal])
    assert_bits_or_one_ulp(tsdf[~marginal], want_tsdf[~marginal], 'tsdf')
    return tsdf, weight


SMALL_EXTENTS, SMALL_VOXEL = (13, 12, 11), 0.25            # a coarser grid over the sphere for the variants: 1716 nodes, two tiles


def test_scene_volume_equals_the_restatement():
    s = ref.scene()
    want_tsdf, want_weight, margins = ref.scene_volume()
    assert not ((margins['tie'] < MARGIN) | (margins['behind'] < MARGIN)).any()          # nothing is left out on this scene
    tsdf, weight = integrate(s['depth'], s['extrinsics'], s['intrinsics'], ref.GRID_LO, ref.GRID_VOXEL, ref.GRID_EXTENTS, ref.GRID_MU)
    assert numpy.array_equal(weight, want_weight)
    assert_bits_or_one_ulp(tsdf, want_tsdf, 'tsdf')
    again = integrate(s['depth'], s['extrinsics'], s['intrinsics'], ref.GRID_LO, ref.GRID_VOXEL, ref.GRID_EXTENTS, ref.GRID_MU)
    assert again[0].tobytes() == tsdf.tobytes() and again[1].tobytes() == weight.tobytes()


def test_volume_with_a_mask_and_with_invalid_depths():
    s = ref.scene()
    mask = numpy.ones(s['depth'].shape, dtype=numpy.uint8)
    mask[0, :, :20] = 0
    mask[3, 10:30, 10:30] = 0
    masked = assert_volume_equals_restatement(s['depth'], s['extrinsics'], s['intrinsics'], ref.GRID_LO, SMALL_VOXEL, SMALL_EXTENTS, 0.5, mask)
    plain = assert_volume_equals_restatement(s['depth'], s['extrinsics'], s['intrinsics'], ref.GRID_LO, SMALL_VOXEL, SMALL_EXTENTS, 0.5)
    assert masked[1].sum() < plain[1].sum()
    as_bool = geometry.tsdf_volume(on_device(s['depth']), s['extrinsics'], s['intrinsics'], ref.GRID_LO, SMALL_VOXEL, SMALL_EXTENTS, 0.5,
                                   on_device(mask.astype(bool)))
    assert as_bool[0].cpu().numpy().tobytes() == masked[0].tobytes()
    depth = s['depth'].copy()
    rng = numpy.random.default_rng(3)
    for value in (0.0, -2.0, numpy.nan, numpy.inf, -numpy.inf):
        depth[rng.uniform(size=depth.shape) < 0.04] = value
    sown = assert_volume_equals_restatement(depth, s['extrinsics'], s['intrinsics'], ref.GRID_LO, SMALL_VOXEL, SMALL_EXTENTS, 0.5)
    assert sown[1].sum() < plain[1].sum() and numpy.isfinite(sown[0]).all()


def test_volume_with_a_camera_inside_the_grid_and_without_views():
    s = ref.scene()
    inside = ref.look_at((0.3, 0.2, 0.1))
    extrinsics = numpy.concatenate([s['extrinsics'], inside[None]])
    intrinsics = numpy.concatenate([s['intrinsics'], s['intrinsics'][:1]])
    depth = numpy.concatenate([s['depth'], numpy.full((1, 48, 48), 0.6, numpy.float32)])
    nx, ny, nz = SMALL_EXTENTS
    nodes = numpy.stack(numpy.meshgrid(*[ref.GRID_LO[a] + SMALL_VOXEL * numpy.arange(n) for a, n in enumerate(SMALL_EXTENTS)], indexing='ij'), -1)
    c_z = nodes.reshape(-1, 3) @ inside[2, :3] + inside[2, 3]
    assert 100 < int((c_z <= 0).sum()) < nx * ny * nz - 100                              # nodes behind it and nodes in front of it
    seven = assert_volume_equals_restatement(depth, extrinsics, intrinsics, ref.GRID_LO, SMALL_VOXEL, SMALL_EXTENTS, 0.5)
    six = assert_volume_equals_restatement(s['depth'], s['extrinsics'], s['intrinsics'], ref.GRID_LO, SMALL_VOXEL, SMALL_EXTENTS, 0.5)
    assert seven[1].max() <= 7 and (seven[1] >= six[1]).all() and (seven[1] > six[1]).any()
    tsdf, weight = ops.tsdf_integrate(torch.empty((0, 48, 48), dtype=torch.float32, device=DEV),
                                      torch.empty((0, ops.FUSE_CAMERA), dtype=torch.float64, device=DEV), ref.GRID_LO, SMALL_VOXEL,
                                      SMALL_EXTENTS, 0.5)
    assert tuple(tsdf.shape) == (nz, ny, nx) and not weight.any() and (tsdf == 1.0).all()


# ------------------------------------------------------------------------------------------------------------------ extract
def extract(tsdf, weight, lo, voxel_size, min_weight=1):
    vertices, triangles = geometry.extract_mesh(on_device(tsdf), on_device(weight), lo, voxel_size, min_weight)
    assert vertices.dtype == torch.float32 and tuple(vertices.shape) == (vertices.shape[0], 3) and vertices.is_cuda
    assert triangles.dtype == torch.int32 and tuple(triangles.shape) == (triangles.shape[0], 3)
    return vertices.cpu().numpy(), triangles.cpu().numpy()


def assert_mesh_equals_restatement(tsdf, weight, lo, voxel_size, min_weight, want):
    vertices, triangles = extract(tsdf, weight, lo, voxel_size, min_weight)
    assert (len(vertices), len(triangles)) == (len(want[0]), len(want[1]))
    assert numpy.array_equal(triangles, want[1])                                         # every index, in the restatement's order
    assert_bits_or_one_ulp(vertices, want[0], 'vertices')
    return vertices, triangles


@pytest.mark.parametrize('case', ['scene', 'holed scene', 'min_weight 2', 'slab'])
def test_scene_mesh_equals_the_restatement(case):
    truncation, min_weight, extents, lo = {'scene': (ref.GRID_MU, 1, ref.GRID_EXTENTS, ref.GRID_LO),
                                           'holed scene': (0.25, 1, ref.GRID_EXTENTS, ref.GRID_LO),
                                           'min_weight 2': (ref.GRID_MU, 2, ref.GRID_EXTENTS, ref.GRID_LO),
                                           'slab': (ref.GRID_MU, 1, ref.SLAB_EXTENTS, ref.SLAB_LO)}[case]
    tsdf, weight, _ = ref.scene_volume(truncation, extents, lo)
    want = ref.scene_mesh(truncation, min_weight, extents, lo)
    assert tsdf.size > 5 * 2048                                                          # several compaction tiles of 2048 nodes
    vertices, triangles = assert_mesh_equals_restatement(tsdf, weight, lo, ref.GRID_VOXEL, min_weight, want)
    if case == 'scene':
        assert (len(vertices), len(triangles)) == (3736, 7468)
        again = extract(tsdf, weight, lo, ref.GRID_VOXEL, min_weight)
        assert again[0].tobytes() == vertices.tobytes() and again[1].tobytes() == triangles.tobytes()
    if case == 'slab':
        cube = ref.scene_mesh()[0]
        order = lambda v: v[numpy.lexsort((v[:, 0], v[:, 1], v[:, 2]))]
        assert numpy.abs(order(vertices).astype(numpy.float64) - order(cube)).max() <= 2.0 ** -22     # the cube's set of positions


@pytest.mark.parametrize('holes', [False, True])
def test_random_field_mesh_equals_the_restatement(holes):
    tsdf, weight = ref.random_field(holes)
    want = ref.extract_mesh(tsdf, weight, (0.5, -0.25, 2.0), 0.75)
    assert holes or len(want[3]) == 96                                                  # every (tetrahedron, case) pair occurs
    assert_mesh_equals_restatement(tsdf, weight, (0.5, -0.25, 2.0), 0.75, 1, want)


def test_plane_through_grid_nodes():
    tsdf, weight = ref.plane_field()
    want = ref.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    vertices, triangles = assert_mesh_equals_restatement(tsdf, weight, (0.0, 0.0, 0.0), 1.0, 1, want)
    assert len(vertices) == 63 and len(triangles) == 96 and (vertices[:, 0] == 3.0).all()
    assert ref.surface_statistics(vertices, triangles)['zero_area'] == 72


def test_volumes_without_a_surface_give_an_empty_mesh():
    tsdf, weight = ref.random_field()
    for volume in ((numpy.abs(tsdf), weight), (tsdf, numpy.zeros_like(weight)), (tsdf[:1], weight[:1]), (tsdf[:, :1], weight[:, :1]),
                   (tsdf[:, :, :1], weight[:, :, :1]), (tsdf[:1, :1, :1], weight[:1, :1, :1])):
        vertices, triangles = extract(numpy.ascontiguousarray(volume[0]), numpy.ascontiguousarray(volume[1]), (0.0, 0.0, 0.0), 1.0)
        assert vertices.shape == (0, 3) and triangles.shape == (0, 3)
    vertices, triangles = extract(tsdf, weight, (0.0, 0.0, 0.0), 1.0, min_weight=2)
    assert vertices.shape == (0, 3) and triangles.shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------ colour
def colour(points, scene, tolerance, mask=None, views=slice(None)):
    colours, agreeing = geometry.colour_points(on_device(points), on_device(scene['depth'][views]), on_device(scene['image'][views]),
                                               scene['extrinsics'][views], scene['intrinsics'][views], tolerance,
                                               None if mask is None else on_device(mask[views]))
    assert colours.dtype == torch.uint8 and tuple(colours.shape) == (len(points), 3) and colours.is_cuda
    assert agreeing.dtype == torch.uint8 and tuple(agreeing.shape) == (len(points),)
    return colours.cpu().numpy(), agreeing.cpu().numpy()


def test_vertex_colours_equal_the_restatement():
    want_colours, want_views, margins = ref.scene_colours()
    assert min(margins) >= MARGIN
    colours, views = colour(ref.scene_mesh()[0], ref.scene(), ref.COLOUR_TOLERANCE)
    assert numpy.array_equal(colours, want_colours) and numpy.array_equal(views, want_views)
    assert int((views == 0).sum()) == 40


def test_colours_of_points_no_view_sees():
    """Points on the sphere, far outside every frame, behind the cameras, NaN and infinite; with six views, with one and with a mask."""
    s = ref.scene()
    rng = numpy.random.default_rng(5)
    on_sphere = rng.normal(size=(40, 3))
    on_sphere /= numpy.linalg.norm(on_sphere, axis=1, keepdims=True)
    points = numpy.concatenate([on_sphere, [[9.0, 0.5, 0.2], [-30.0, 1.0, 1.0], [100.0, 100.0, 100.0], [0.0, 0.0, 50.0], [numpy.nan, 0.0, 0.0],
                                            [0.0, numpy.inf, 0.0], [0.0, 0.0, -numpy.inf], [1e30, -1e30, 1e30], [4.0, 0.3, 0.2]]]).astype(numpy.float32)
    mask = numpy.ones(s['depth'].shape, dtype=numpy.uint8)
    mask[:, 20:28, :] = 0
    for views, used_mask in ((slice(None), None), (slice(0, 1), None), (slice(None), mask)):
        margins = []
        want = ref.colour_points(points, s['depth'][views], s['image'][views], s['extrinsics'][views], s['intrinsics'][views], 0.05,
                                 None if used_mask is None else used_mask[views], margins)
        assert min(margins) >= MARGIN
        got = colour(points, s, 0.05, used_mask, views)
        assert numpy.array_equal(got[0], want[0]) and numpy.array_equal(got[1], want[1])
        assert not got[1][40:].any() and not got[0][40:].any() and got[1][:40].any()
    behind_view_0 = numpy.array([[9.0, 0.5, 0.2], [4.0, 0.3, 0.2]], numpy.float32)        # behind the camera at (4, 0.3, 0.2), and in it
    assert not colour(behind_view_0, s, 10.0, None, slice(0, 1))[1].any()
    empty = colour(numpy.zeros((0, 3), numpy.float32), s, 0.05)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_the_devices_own_volume_gives_a_closed_oriented_surface():
    s = ref.scene()
    depth, image = on_device(s['depth']), on_device(s['image'])
    tsdf, weight = geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], ref.GRID_LO, ref.GRID_VOXEL, ref.GRID_EXTENTS, ref.GRID_MU)
    vertices, triangles = geometry.extract_mesh(tsdf, weight, ref.GRID_LO, ref.GRID_VOXEL)
    colours, views = geometry.colour_points(vertices, depth, image, s['extrinsics'], s['intrinsics'], ref.COLOUR_TOLERANCE)
    stats = ref.assert_closed_oriented_surface(vertices.cpu().numpy(), triangles.cpu().numpy())
    assert (stats['vertices'], stats['edges'], stats['faces']) == (3736, 11202, 7468)
    radii = numpy.linalg.norm(vertices.cpu().numpy().astype(numpy.float64), axis=1)
    assert 0.87 <= radii.min() and radii.max() <= 1.11
    assert int((views == 0).sum()) == 40 and colours[views > 0].any()


def parse_ply_mesh(data):
    header, body = data.split(b'end_header\n', 1)
    lines = header.decode('ascii').split('\n')
    assert lines[:2] == ['ply', 'format binary_little_endian 1.0'] and lines[-3:-1] == [lines[-3], 'property list uchar int vertex_indices']
    nv, nf = int(lines[2].split()[-1]), int(lines[-3].split()[-1])
    assert lines[2] == f'element vertex {nv}' and lines[-3] == f'element face {nf}' and len(body) == nv * 15 + nf * 13
    vertices = numpy.frombuffer(body[:nv * 15], dtype=geometry.PLY_VERTEX)
    faces = numpy.frombuffer(body[nv * 15:], dtype=geometry.PLY_FACE)
    return vertices, faces


def test_export_mesh(tmp_path):
    cfg = synth.make_configs('config1')
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 11, 150.0, 4.0).items()})
    model = model.to(DEV).eval()
    cameras = [synth.camera('fern', pose, resolution=(12, 15)) for pose in (0, 1, 2)]
    device = torch.device(DEV)
    frames = [harness.predict_frame(model, cfg, camera, device) for camera in cameras]
    images, depths = numpy.stack([f['image'] for f in frames]), numpy.stack([f['depth'] for f in frames])
    matrices = [geometry.camera_matrices(camera) for camera in cameras]
    cloud = geometry.fuse_depth_maps(on_device(depths), on_device(images), [m[0] for m in matrices], [m[1] for m in matrices], 0.0, 0)[0]
    box = numpy.concatenate([cloud.min(dim=0)[0].cpu().numpy(), cloud.max(dim=0)[0].cpu().numpy()]).astype(numpy.float64)
    voxel = float((box[3:] - box[:3]).max()) / 12
    out = harness.export_mesh(model, cfg, cameras, tmp_path / 'mesh.ply', device, voxel)
    assert out['depths_device'].cpu().numpy().tobytes() == depths.tobytes() and numpy.array_equal(out['images_device'].cpu().numpy(), images)
    assert out['voxel_size'] == voxel and out['truncation'] == 4 * voxel
    lo, extents = numpy.array(out['lo']), out['extents']
    assert numpy.allclose(lo, box[:3] - 4 * voxel, atol=1e-6 * voxel)
    high = lo + voxel * (numpy.array(extents) - 1)
    assert (high >= box[3:] + 4 * voxel - 1e-9).all() and (high <= box[3:] + 6 * voxel).all()
    assert tuple(out['tsdf'].shape) == extents[::-1] == tuple(out['weight'].shape)
    # the parts are the library's own calls on the renders
    tsdf, weight = geometry.tsdf_volume(on_device(depths), [m[0] for m in matrices], [m[1] for m in matrices], out['lo'], voxel, extents, 4 * voxel)
    assert out['tsdf'].cpu().numpy().tobytes() == tsdf.cpu().numpy().tobytes() and torch.equal(out['weight'], weight)
    vertices, triangles = out['vertices'].cpu().numpy(), out['triangles'].cpu().numpy()
    assert len(vertices) > 0 and len(triangles) > 0
    assert triangles.min() >= 0 and triangles.max() < len(vertices)
    assert (vertices >= lo - 1e-6).all() and (vertices <= high + 1e-6).all()
    coloured = geometry.colour_points(out['vertices'], on_device(depths), on_device(images), [m[0] for m in matrices], [m[1] for m in matrices], voxel)
    assert torch.equal(out['colours'], coloured[0]) and torch.equal(out['views'], coloured[1])
    data = (tmp_path / 'mesh.ply').read_bytes()
    assert data == geometry.ply_mesh_bytes(vertices, out['colours'], triangles)
    records, faces = parse_ply_mesh(data)
    assert len(records) == len(vertices) and len(faces) == len(triangles) and (faces['count'] == 3).all()
    assert max(faces['a'].max(), faces['b'].max(), faces['c'].max()) < len(records)
    # bounds, a depth range and min_weight reach the calls; an existing file is left alone
    inner = harness.export_mesh(model, cfg, cameras, tmp_path / 'inner.ply', device, voxel, truncation=2 * voxel,
                                bounds=(box[:3], box[3:]), min_weight=2, colour_tolerance=0.0,
                                depth_range=(float(numpy.percentile(depths, 10)), float(numpy.percentile(depths, 90))))
    assert inner['lo'] == tuple(box[:3]) and inner['truncation'] == 2 * voxel and int(inner['weight'].max()) <= 3
    assert all(n <= m for n, m in zip(inner['extents'], extents))
    harness.export_mesh(model, cfg, cameras[:2], tmp_path / 'mesh.ply', device, 2 * voxel)
    assert (tmp_path / 'mesh.ply').read_bytes() == data
    with pytest.raises(RuntimeError, match=r'7 nx ny nz <= 2\^31 - 1'):
        harness.export_mesh(model, cfg, cameras, tmp_path / 'huge.ply', device, voxel / 1000)
    assert not (tmp_path / 'huge.ply').exists()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_python_refusals():
    s = ref.scene()
    depth, image = on_device(s['depth']), on_device(s['image'])
    grid = (ref.GRID_LO, ref.GRID_VOXEL, ref.GRID_EXTENTS)
    with pytest.raises(RuntimeError, match='truncation'):
        geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], *grid, 0.0)
    with pytest.raises(RuntimeError, match='voxel_size'):
        geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], ref.GRID_LO, float('nan'), ref.GRID_EXTENTS, 0.5)
    with pytest.raises(RuntimeError, match='extents'):
        geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], ref.GRID_LO, 0.125, (25, 0, 25), 0.5)
    with pytest.raises(RuntimeError, match=r'extents.*2\^31 - 1'):
        geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], ref.GRID_LO, 0.125, (1024, 1024, 1024), 0.5)
    with pytest.raises(RuntimeError, match='lo'):
        geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], (0.0, float('inf'), 0.0), 0.125, ref.GRID_EXTENTS, 0.5)
    with pytest.raises(RuntimeError, match='depth'):
        geometry.tsdf_volume(depth.double(), s['extrinsics'], s['intrinsics'], *grid, 0.5)
    with pytest.raises(RuntimeError, match='extrinsics'):
        geometry.tsdf_volume(depth, s['extrinsics'][:2], s['intrinsics'], *grid, 0.5)
    with pytest.raises(RuntimeError, match='mask'):
        geometry.tsdf_volume(depth, s['extrinsics'], s['intrinsics'], *grid, 0.5, mask=torch.ones((6, 48, 47), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='GPU'):
        geometry.tsdf_volume(depth.cpu(), s['extrinsics'], s['intrinsics'], *grid, 0.5)
    tsdf, weight = (on_device(a) for a in ref.random_field())
    with pytest.raises(RuntimeError, match='min_weight'):
        geometry.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0, 0)
    with pytest.raises(RuntimeError, match='min_weight'):
        geometry.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0, 256)
    with pytest.raises(RuntimeError, match='weight'):
        geometry.extract_mesh(tsdf, weight[:-1], (0.0, 0.0, 0.0), 1.0)
    with pytest.raises(RuntimeError, match='weight'):
        geometry.extract_mesh(tsdf, weight.float(), (0.0, 0.0, 0.0), 1.0)
    with pytest.raises(RuntimeError, match='tsdf'):
        geometry.extract_mesh(tsdf[0], weight[0], (0.0, 0.0, 0.0), 1.0)
    with pytest.raises(RuntimeError, match='voxel_size'):
        geometry.extract_mesh(tsdf, weight, (0.0, 0.0, 0.0), -1.0)
    points = on_device(ref.scene_mesh()[0])
    with pytest.raises(RuntimeError, match='colour_tolerance'):
        geometry.colour_points(points, depth, image, s['extrinsics'], s['intrinsics'], -0.1)
    with pytest.raises(RuntimeError, match='colour_tolerance'):
        geometry.colour_points(points, depth, image, s['extrinsics'], s['intrinsics'], float('nan'))
    with pytest.raises(RuntimeError, match='points'):
        geometry.colour_points(points[:, :2], depth, image, s['extrinsics'], s['intrinsics'], 0.1)
    with pytest.raises(RuntimeError, match='image'):
        geometry.colour_points(points, depth, image[:, :, :, :2], s['extrinsics'], s['intrinsics'], 0.1)


def test_the_librarys_own_refusals_come_as_status_codes():
    """Every call returns the header's status for a bad argument, before any launch: the outputs keep their bytes."""
    lib, C = _lib.load(), _lib.C
    s = ref.scene()
    depth, image = on_device(s['depth']), on_device(s['image'])
    cameras = on_device(geometry.fuse_cameras(s['extrinsics'], s['intrinsics']))
    tsdf_in, weight_in = (on_device(a) for a in ref.scene_volume()[:2])
    tsdf = torch.full((25, 25, 25), 7.0, dtype=torch.float32, device=DEV)
    weight = torch.full((25, 25, 25), 9, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    ws = torch.empty((int(lib.snerf_mesh_workspace_bytes(25, 25, 25)) + 256,), dtype=torch.uint8, device=DEV)
    vertices = torch.full((3736, 3), 7.0, dtype=torch.float32, device=DEV)
    triangles = torch.full((7468, 3), -7, dtype=torch.int32, device=DEV)
    colours = torch.full((3736, 3), 9, dtype=torch.uint8, device=DEV)
    agreeing = torch.full((3736,), 9, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    null, lo = ctypes.c_void_p(0), ref.GRID_LO

    def integrate_status(views=6, voxel=0.125, extents=(25, 25, 25), mu=0.5, depth_pointer=p(depth), tsdf_pointer=p(tsdf), lo_y=lo[1]):
        return lib.snerf_tsdf_integrate(depth_pointer, null, p(cameras), views, 48, 48, voxel, lo[0], lo_y, lo[2], *extents, mu, tsdf_pointer,
                                        p(weight), null)

    assert integrate_status(views=-1) == integrate_status(views=256) == integrate_status(voxel=0.0) == C.SNERF_E_INVALID
    assert integrate_status(voxel=float('inf')) == integrate_status(mu=0.0) == integrate_status(mu=float('nan')) == C.SNERF_E_INVALID
    assert integrate_status(extents=(25, 0, 25)) == integrate_status(depth_pointer=null) == integrate_status(tsdf_pointer=null) == C.SNERF_E_INVALID
    assert integrate_status(lo_y=float('nan')) == C.SNERF_E_INVALID
    assert integrate_status(extents=(1024, 1024, 1024)) == integrate_status(extents=(46341, 46341, 1)) == C.SNERF_E_UNSUPPORTED
    assert b'2^31 - 1' in lib.snerf_last_error()

    def count_status(min_weight=1, voxel=0.125, extents=(25, 25, 25), counts_pointer=p(counts), ws_pointer=p(ws), weight_pointer=p(weight_in)):
        return lib.snerf_mesh_count(p(tsdf_in), weight_pointer, voxel, *lo, *extents, min_weight, counts_pointer, ws_pointer, null)

    assert count_status(min_weight=0) == count_status(min_weight=256) == count_status(voxel=-1.0) == C.SNERF_E_INVALID
    assert count_status(extents=(25, 25, 0)) == count_status(counts_pointer=null) == count_status(weight_pointer=null) == C.SNERF_E_INVALID
    assert count_status(ws_pointer=ctypes.c_void_p(ws.data_ptr() + 8)) == count_status(ws_pointer=null) == C.SNERF_E_INVALID
    assert count_status(counts_pointer=ctypes.c_void_p(counts.data_ptr() + 4)) == C.SNERF_E_INVALID
    assert count_status(extents=(1024, 1024, 1024)) == C.SNERF_E_UNSUPPORTED
    assert lib.snerf_mesh_workspace_bytes(1024, 1024, 1024) == 0 and lib.snerf_mesh_workspace_bytes(25, -1, 25) == 0

    def emit_status(min_weight=1, extents=(25, 25, 25), vertices_pointer=p(vertices), triangles_pointer=p(triangles), counts_pointer=p(counts)):
        return lib.snerf_mesh_emit(p(tsdf_in), p(weight_in), 0.125, *lo, *extents, min_weight, counts_pointer, vertices_pointer, triangles_pointer,
                                   p(ws), null)

    assert emit_status(min_weight=0) == emit_status(extents=(0, 25, 25)) == emit_status(vertices_pointer=null) == C.SNERF_E_INVALID
    assert emit_status(triangles_pointer=null) == emit_status(counts_pointer=null) == C.SNERF_E_INVALID
    assert emit_status(extents=(1024, 1024, 1024)) == C.SNERF_E_UNSUPPORTED

    def colour_status(count=3736, views=6, tolerance=0.125, points_pointer=p(vertices), image_pointer=p(image), colours_pointer=p(colours)):
        return lib.snerf_colour_points(points_pointer, count, p(depth), image_pointer, null, p(cameras), views, 48, 48, tolerance, colours_pointer,
                                       p(agreeing), null)

    assert colour_status(count=-1) == colour_status(views=-1) == colour_status(views=256) == C.SNERF_E_INVALID
    assert colour_status(tolerance=-1.0) == colour_status(tolerance=float('nan')) == C.SNERF_E_INVALID
    assert colour_status(points_pointer=null) == colour_status(image_pointer=null) == colour_status(colours_pointer=null) == C.SNERF_E_INVALID
    assert colour_status(count=2 ** 31) == C.SNERF_E_UNSUPPORTED
    assert colour_status(count=0, points_pointer=null, colours_pointer=null) == C.SNERF_OK      # nothing to do: nothing enqueued
    torch.cuda.synchronize()
    assert (tsdf == 7.0).all() and (weight == 9).all() and (counts == -5).all() and (vertices == 7.0).all() and (triangles == -7).all()
    assert (colours == 9).all() and (agreeing == 9).all()
