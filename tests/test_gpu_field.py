"""The field export on a real MI355X: ``ops.field_grid_points``, ``ops.field_point_views`` and ``ops.field_values`` against the
restatement of tests/field_reference.py (tests/test_field_host.py pins that one), bit for bit -- both sides evaluate the same fp64
expressions in the same order, without contraction, with correctly rounded divisions; what differs is printed, and a difference of
more than one float32 ulp, or of sign, fails.  Weights and chosen views are equal exactly: the restatement reports how far every
decision (c_z against 0, a tie of rint, the frame's edge, the near plane, two equal depths) lies from turning over, and the scenes
are chosen so that none lies within 1e-9.  ``model.query`` is held to the oracle's MLP at the tolerances the forward tests of its
precision hold the same kernels to; ``geometry.density_volume`` and ``harness.export_density_mesh`` to the restatement and to the
library's own calls."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import geometry, harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import field_reference as ref
from tests import mesh_reference, util
from tests.test_gpu_mesh import assert_bits_or_one_ulp, parse_ply_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 1e-9
# tests/test_gpu_kernels.py (test_mlp_forward_matches_reference 'plain', test_mlp_forward_noise_tail_and_multi_sample) holds the fp32
# forward to the oracle at: sigma 1e-5 relative (util.rel_linf), rgb 1e-5 absolute.  tests/test_gpu_bf16.py
# (test_bf16_mlp_against_oracle) holds the bf16 forward to the same fp32 oracle at: sigma 2e-2 relative, rgb 5e-4 absolute -- on
# weights of synth_state_dict(..., 31, 50.0, shift), the gain and seed used here.
FORWARD_TOLERANCE = {'fp32': (1e-5, 1e-5), 'bf16': (2e-2, 5e-4)}


def on_device(array):
    return torch.from_numpy(numpy.array(array)).to(DEV)          # (a copy: the shared fixtures are read-only)


def host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


# ------------------------------------------------------------------------------------------------------------------ 1 grid points
def test_grid_points_and_weights_equal_the_restatement():
    want_points, want_weight, margins = ref.scene_grid_points()
    assert min(margins) >= MARGIN                                                        # nothing is left out on this scene
    table = on_device(ref.scene_table())
    grid = (ref.SMALL_LO, ref.SMALL_VOXEL, ref.SMALL_EXTENTS)
    points, weight = ops.field_grid_points(*grid, table, ref.SCENE_RESOLUTION)
    assert points.dtype == torch.float32 and tuple(points.shape) == (1716, 3) and points.is_cuda
    assert weight.dtype == torch.uint8 and tuple(weight.shape) == (1716,)
    points, weight = host(points, weight)
    assert numpy.array_equal(weight, want_weight)
    assert points.tobytes() == want_points.tobytes()
    for blocks in (((0, 1000), (1000, 716)), tuple((first, min(130, 1716 - first)) for first in range(0, 1716, 130))):
        parts = [host(*ops.field_grid_points(*grid, table, ref.SCENE_RESOLUTION, None, first, count)) for first, count in blocks]
        assert numpy.concatenate([p[0] for p in parts]).tobytes() == points.tobytes()
        assert numpy.concatenate([p[1] for p in parts]).tobytes() == weight.tobytes()
    again = host(*ops.field_grid_points(*grid, table, ref.SCENE_RESOLUTION))
    assert again[0].tobytes() == points.tobytes() and again[1].tobytes() == weight.tobytes()
    none = host(*ops.field_grid_points(*grid, table[:0], ref.SCENE_RESOLUTION))
    assert not none[1].any() and none[0].tobytes() == points.tobytes()
    no_pixels = host(*ops.field_grid_points(*grid, table, (0, 48)))
    assert not no_pixels[1].any()
    empty = ops.field_grid_points(*grid, table, ref.SCENE_RESOLUTION, None, 1716, 0)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0,)


# ------------------------------------------------------------------------------------------------------------------ 2 NDC
NDC_EXTENTS, NDC_VOXEL, NDC_LO = (9, 8, 11), 0.21, (-0.83, -0.71, -2.27)


def test_ndc_grid_points_equal_the_restatement():
    _, table, ndc = ref.fern_cameras()
    margins = []
    want_points, want_weight = ref.grid_points(NDC_LO, NDC_VOXEL, NDC_EXTENTS, table, (48, 64), ndc, 0, None, margins)
    assert min(margins) >= MARGIN
    z = NDC_LO[2] + NDC_VOXEL * numpy.arange(NDC_EXTENTS[2])
    behind = numpy.repeat(~(z <= -ndc[2]), NDC_EXTENTS[0] * NDC_EXTENTS[1])
    assert 100 < int(behind.sum()) < behind.size - 100                                   # the grid straddles the near plane
    points, weight = host(*ops.field_grid_points(NDC_LO, NDC_VOXEL, NDC_EXTENTS, on_device(table), (48, 64), ndc))
    assert not points[behind].any() and not weight[behind].any()
    assert numpy.array_equal(weight, want_weight) and weight[~behind].any() and (weight[~behind] == 0).any()
    assert_bits_or_one_ulp(points, want_points, 'ndc points')
    assert numpy.abs(points[~behind][:, 2]).max() <= 1.0 and (points[~behind][:, 2] >= -1.0).all()
    world = host(*ops.field_grid_points(NDC_LO, NDC_VOXEL, NDC_EXTENTS, on_device(table), (48, 64)))
    assert numpy.array_equal(world[1][~behind], weight[~behind]) and world[1][behind].any()     # without ndc, no near plane


# ------------------------------------------------------------------------------------------------------------------ 3 point views
POINTS_SEED = 0


def test_point_views_equal_the_restatement():
    table = numpy.array(ref.scene_table())
    rng = numpy.random.default_rng(POINTS_SEED)
    unseen = [[50.0, 50.0, 50.0], [-30.0, 20.0, 1.0], [9.0, 9.0, -9.0], [1e30, -1e30, 1e30]]
    points = numpy.concatenate([rng.uniform(-1.5, 1.5, (1000, 3)), unseen]).astype(numpy.float32)
    margins = []
    want = ref.point_views(points, table, ref.SCENE_RESOLUTION, None, margins)
    assert min(margins) >= MARGIN                                                        # the seed is chosen for this: nothing is left out
    got = ops.field_point_views(on_device(points), on_device(table), ref.SCENE_RESOLUTION)
    assert [t.dtype for t in got] == [torch.float32, torch.float32, torch.uint8]
    assert [tuple(t.shape) for t in got] == [(1004, 3), (1004, 3), (1004,)]
    mlp_points, dirs, view = host(*got)
    assert numpy.array_equal(view, want[2]) and mlp_points.tobytes() == points.tobytes()
    assert (view[1000:] == ref.NO_VIEW).all() and (view[:1000] < 6).all() and len(set(view[:1000].tolist())) == 6
    assert_bits_or_one_ulp(dirs, want[1], 'view directions')
    # a point on a camera's centre (the table's own, made a float32 value): whether that view sees it is marginal, its direction is not
    one = table[:1].copy()
    column = [ref.E_INV + 3, ref.E_INV + 7, ref.E_INV + 11]
    one[0, column] = one[0, column].astype(numpy.float32)
    centre = one[0, column][None].astype(numpy.float32)
    at_centre = host(*ops.field_point_views(on_device(centre), on_device(one), ref.SCENE_RESOLUTION))
    assert not at_centre[1].any() and at_centre[0].tobytes() == centre.tobytes() and at_centre[2][0] in (0, ref.NO_VIEW)
    assert not ref.point_views(centre, one, ref.SCENE_RESOLUTION)[1].any()
    # ndc: the mapped points follow the input map, the directions stay in the scene frame
    _, fern, ndc = ref.fern_cameras()
    nodes = ref.grid_points(NDC_LO, NDC_VOXEL, NDC_EXTENTS, fern, (48, 64))[0]
    margins = []
    want = ref.point_views(nodes, fern, (48, 64), ndc, margins)
    assert min(margins) >= MARGIN
    mlp_points, dirs, view = host(*ops.field_point_views(on_device(nodes), on_device(fern), (48, 64), ndc))
    assert numpy.array_equal(view, want[2]) and (view == ref.NO_VIEW).any() and (view < 3).any()
    assert_bits_or_one_ulp(mlp_points, want[0], 'ndc points of a point set')
    assert_bits_or_one_ulp(dirs, want[1], 'view directions under ndc')
    empty = ops.field_point_views(torch.empty((0, 3), device=DEV), on_device(table), ref.SCENE_RESOLUTION)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0,)]


# ------------------------------------------------------------------------------------------------------------------ 4 values
def test_values_equal_the_fp64_formula():
    level = 2.5
    sigma = numpy.array([0.0, level / 2, level, 2 * level, 10 * level, numpy.inf, numpy.nan], dtype=numpy.float32)
    rng = numpy.random.default_rng(4)
    sigma = numpy.concatenate([sigma, sigma, rng.uniform(0.0, 3 * level, 1000).astype(numpy.float32)])
    weight = numpy.concatenate([numpy.zeros(7), numpy.full(7, 3), rng.integers(0, 3, 1000)]).astype(numpy.uint8)
    want = ref.values(sigma, weight, level)
    assert want[:14].tolist() == [1.0] * 7 + [1.0, 0.5, 0.0, -1.0, -1.0, -1.0, 1.0]
    got = ops.field_values(on_device(sigma), on_device(weight), level)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1014,)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    shaped = ops.field_values(on_device(sigma[:1008].reshape(7, 12, 12)), on_device(weight[:1008].reshape(7, 12, 12)), level)
    assert tuple(shaped.shape) == (7, 12, 12) and shaped.cpu().numpy().tobytes() == want[:1008].tobytes()
    assert tuple(ops.field_values(torch.empty((0,), device=DEV), torch.empty((0,), dtype=torch.uint8, device=DEV), level).shape) == (0,)


# ------------------------------------------------------------------------------------------------------------------ 5 model.query
def seeded_model(kind, precision, shift, **mlp_overrides):
    cfg = synth.with_overrides(synth.make_configs(kind), hip_precision=precision)
    for name in ('coarse_mlp', 'fine_mlp'):
        if name in cfg['model']:
            cfg['model'][name].update(mlp_overrides)
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    state = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 31, 50.0, shift).items()}
    model.load_state_dict(state)
    return cfg, model.to(DEV).eval(), state


@pytest.mark.parametrize('kind,precision,shift', [('headline', 'fp32', 2.0), ('headline', 'bf16', 2.0), ('config1', 'fp32', 1.0)])
def test_query_matches_the_oracle(kind, precision, shift):
    cfg, model, state = seeded_model(kind, precision, shift)
    mlp = 'fine_mlp' if 'fine_mlp' in cfg['model'] else 'coarse_mlp'
    rng = numpy.random.RandomState(3)
    points = torch.from_numpy(rng.uniform(-1, 1, (1000, 3)).astype(numpy.float32))
    dirs = torch.from_numpy(rng.standard_normal((1000, 3)).astype(numpy.float32))
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    want = oracle.mlp_forward(state, mlp.replace('_mlp', '_model.'), cfg['model'][mlp], points, dirs)
    assert (want['sigma'] == 0).any() and (want['sigma'] > 0).sum() > 100                # both zero and positive densities
    got = model.query(points.to(DEV), dirs.to(DEV))
    assert sorted(got) == ['rgb', 'sigma'] and tuple(got['sigma'].shape) == (1000,) and tuple(got['rgb'].shape) == (1000, 3)
    e_sigma, e_rgb = util.rel_linf(got['sigma'], want['sigma'][:, 0]), util.linf(got['rgb'], want['rgb'])
    bound = FORWARD_TOLERANCE[precision]
    util.observe(f'field/query/{kind}/{precision}', f'sigma rel {e_sigma:.1e} [{bound[0]}], rgb {e_rgb:.1e} [{bound[1]}]')
    print(f'query {kind} {precision}: sigma rel {e_sigma:.3e}, rgb {e_rgb:.3e}')
    assert e_sigma < bound[0] and e_rgb < bound[1], (e_sigma, e_rgb)
    blocks = model.query(points.to(DEV), dirs.to(DEV), point_block=257)
    assert torch.equal(blocks['sigma'], got['sigma']) and torch.equal(blocks['rgb'], got['rgb'])
    alone = model.query(points.to(DEV))
    assert sorted(alone) == ['sigma'] and torch.equal(alone['sigma'], got['sigma'])
    assert torch.equal(model.query(points.to(DEV), mlp='coarse_mlp')['sigma'], got['sigma']) == (mlp == 'coarse_mlp')
    one = model.query(points[:1].to(DEV), dirs[:1].to(DEV))
    assert util.rel_linf(one['sigma'], want['sigma'][:1, 0]) < bound[0] and util.linf(one['rgb'], want['rgb'][:1]) < bound[1]
    none = model.query(points[:0].to(DEV), dirs[:0].to(DEV))
    assert tuple(none['sigma'].shape) == (0,) and tuple(none['rgb'].shape) == (0, 3)
    with pytest.raises(KeyError, match='mlp'):
        model.query(points.to(DEV), mlp='fine_mlp' if mlp == 'coarse_mlp' else 'other_mlp')
    with pytest.raises(RuntimeError, match='points'):
        model.query(points[:, :2].to(DEV))
    with pytest.raises(RuntimeError, match='view_dirs'):
        model.query(points.to(DEV), dirs[:10].to(DEV))
    with pytest.raises(RuntimeError, match='GPU'):
        model.query(points)


def test_query_refuses_predict_visibility_by_name():
    _, model, _ = seeded_model('config1', 'fp32', 1.0, predict_visibility=True)
    with pytest.raises(NotImplementedError, match='predict_visibility'):
        model.query(torch.zeros((4, 3), device=DEV))


# ------------------------------------------------------------------------------------------------------------------ 6 density volume
def test_density_volume_of_an_analytic_field():
    s = mesh_reference.scene()
    grid = (mesh_reference.GRID_LO, mesh_reference.GRID_VOXEL, mesh_reference.GRID_EXTENTS)
    query = lambda p: 40.0 * torch.clamp(1.0 - p.norm(dim=1) / 1.2, min=0.0)
    sigma, tsdf, weight = geometry.density_volume(query, *grid, s['extrinsics'], s['intrinsics'], ref.SCENE_RESOLUTION, ref.SPHERE_LEVEL,
                                                  point_block=4000)
    assert [tuple(t.shape) for t in (sigma, tsdf, weight)] == [(25, 25, 25)] * 3
    assert [t.dtype for t in (sigma, tsdf, weight)] == [torch.float32, torch.float32, torch.uint8]
    margins = []
    want_points, want_weight = ref.grid_points(*grid, ref.scene_table(), ref.SCENE_RESOLUTION, None, 0, None, margins)
    assert min(margins) >= MARGIN
    assert numpy.array_equal(weight.cpu().numpy().reshape(-1), want_weight) and 3 <= want_weight.min() < want_weight.max() == 6
    assert numpy.abs(sigma.cpu().numpy().reshape(-1) - ref.sphere_density(want_points)).max() <= 1e-4      # (the lambda's own fp32 steps)
    want_tsdf = ref.values(sigma.cpu().numpy(), want_weight.reshape(25, 25, 25), ref.SPHERE_LEVEL)
    assert tsdf.cpu().numpy().tobytes() == want_tsdf.tobytes()
    whole = geometry.density_volume(query, *grid, s['extrinsics'], s['intrinsics'], ref.SCENE_RESOLUTION, ref.SPHERE_LEVEL)
    assert all(torch.equal(a, b) for a, b in zip(whole, (sigma, tsdf, weight)))          # the blocks are the rows of the whole
    want = mesh_reference.extract_mesh(want_tsdf, want_weight.reshape(25, 25, 25), *grid[:2])
    vertices, triangles = host(*geometry.extract_mesh(tsdf, weight, *grid[:2]))
    assert (len(vertices), len(triangles)) == (len(want[0]), len(want[1])) and len(vertices) > 500
    assert numpy.array_equal(triangles, want[1])                                         # every index, in the restatement's order
    assert_bits_or_one_ulp(vertices, want[0], 'vertices')
    mesh_reference.assert_closed_oriented_surface(vertices, triangles)                   # V - E + F = 2
    p = vertices.astype(numpy.float64)
    volume = (p[triangles[:, 0]] * numpy.cross(p[triangles[:, 1]], p[triangles[:, 2]])).sum() / 6
    assert 0.85 * 0.905 < volume < 1.05 * 0.905, volume      # positive: normals out of the dense ball of radius 0.6 (4 pi 0.6^3 / 3)
    radii = numpy.linalg.norm(p, axis=1)
    assert 0.55 <= radii.min() and radii.max() <= 0.65
    # its colours: the field's, seen from the nearest camera
    colours, views = geometry.colour_vertices(lambda q, d: (0.5 - 0.5 * d).contiguous(), on_device(vertices), s['extrinsics'], s['intrinsics'],
                                              ref.SCENE_RESOLUTION)
    want_views = ref.point_views(vertices, ref.scene_table(), ref.SCENE_RESOLUTION)
    assert numpy.array_equal(views.cpu().numpy(), want_views[2]) and (want_views[2] < 6).all()
    assert numpy.abs(colours.cpu().numpy().astype(numpy.float64) - 255 * (0.5 - 0.5 * want_views[1].astype(numpy.float64))).max() <= 0.5 + 1e-3
    with pytest.raises(RuntimeError, match='query'):
        geometry.density_volume(lambda p: p, *grid, s['extrinsics'], s['intrinsics'], ref.SCENE_RESOLUTION, ref.SPHERE_LEVEL)


# ------------------------------------------------------------------------------------------------------------------ 7 the export
EXPORT_VOXEL, EXPORT_BOUNDS = 0.13, ((-1.0, -0.95, -3.4), (1.0, 0.95, -1.6))


@pytest.mark.parametrize('kind,shift', [('config1', 1.0), ('config2', 2.0)])
def test_export_density_mesh(tmp_path, kind, shift):
    cfg, model, _ = seeded_model(kind, 'fp32', shift)
    is_ndc = bool(cfg['data_loader']['ndc'])
    assert is_ndc == (kind == 'config2')
    cameras, table, ndc = ref.fern_cameras()
    ndc = ndc if is_ndc else None
    device = torch.device(DEV)
    extents = (17, 16, 15)
    nodes, seen = ops.field_grid_points(EXPORT_BOUNDS[0], EXPORT_VOXEL, extents, on_device(table), (48, 64), ndc)
    densities = model.query(nodes)['sigma']
    level = float(densities[densities > 0].median())
    out = harness.export_density_mesh(torch.nn.DataParallel(model, device_ids=[0]), cfg, cameras, tmp_path / 'mesh.ply', device, EXPORT_VOXEL,
                                      level, EXPORT_BOUNDS)
    assert sorted(out) == sorted(['vertices', 'colours', 'views', 'triangles', 'sigma', 'tsdf', 'weight', 'lo', 'voxel_size', 'extents',
                                  'level'])
    assert out['lo'] == EXPORT_BOUNDS[0] and out['voxel_size'] == EXPORT_VOXEL and out['extents'] == extents and out['level'] == level
    assert all(tuple(out[k].shape) == extents[::-1] for k in ('sigma', 'tsdf', 'weight'))
    assert torch.equal(out['sigma'].reshape(-1), densities) and torch.equal(out['weight'].reshape(-1), seen)
    assert torch.equal(out['tsdf'], ops.field_values(out['sigma'], out['weight'], level))
    vertices, triangles = out['vertices'], out['triangles']
    assert len(vertices) > 0 and len(triangles) > 0 and int(triangles.min()) >= 0 and int(triangles.max()) < len(vertices)
    mesh = geometry.extract_mesh(out['tsdf'], out['weight'], out['lo'], EXPORT_VOXEL, 1)
    assert torch.equal(mesh[0], vertices) and torch.equal(mesh[1], triangles)
    low = numpy.array(out['lo'])
    high = low + EXPORT_VOXEL * (numpy.array(extents) - 1)
    assert (vertices.cpu().numpy() >= low - 1e-6).all() and (vertices.cpu().numpy() <= high + 1e-6).all()      # the scene frame, also under ndc
    mlp_points, dirs, views = ops.field_point_views(vertices, on_device(table), (48, 64), ndc)
    assert torch.equal(out['views'], views) and (views < 3).any()
    assert torch.equal(out['colours'], ops.to_display(model.query(mlp_points, dirs)['rgb'])[0])
    assert out['colours'].dtype == torch.uint8 and len(torch.unique(out['colours'])) > 3
    data = (tmp_path / 'mesh.ply').read_bytes()
    assert data == geometry.ply_mesh_bytes(vertices, out['colours'], triangles)
    records, faces = parse_ply_mesh(data)
    assert numpy.array_equal(numpy.stack([records['x'], records['y'], records['z']], axis=1), vertices.cpu().numpy())
    assert numpy.array_equal(numpy.stack([records['red'], records['green'], records['blue']], axis=1), out['colours'].cpu().numpy())
    assert numpy.array_equal(numpy.stack([faces['a'], faces['b'], faces['c']], axis=1), triangles.cpu().numpy()) and (faces['count'] == 3).all()
    # min_views and point_block reach the calls; an existing file is left alone
    strict = harness.export_density_mesh(model, cfg, cameras, tmp_path / 'strict.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS, min_views=3,
                                         point_block=1000)
    assert torch.equal(strict['sigma'], out['sigma']) and torch.equal(strict['tsdf'], out['tsdf'])
    assert len(strict['triangles']) < len(triangles)
    harness.export_density_mesh(model, cfg, cameras[:2], tmp_path / 'mesh.ply', device, 2 * EXPORT_VOXEL, level, EXPORT_BOUNDS)
    assert (tmp_path / 'mesh.ply').read_bytes() == data
    # the refusals name their cause
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='level'):
            harness.export_density_mesh(model, cfg, cameras, tmp_path / 'bad.ply', device, EXPORT_VOXEL, bad, EXPORT_BOUNDS)
    with pytest.raises(RuntimeError, match=r'7 nx ny nz <= 2\^31 - 1'):
        harness.export_density_mesh(model, cfg, cameras, tmp_path / 'bad.ply', device, EXPORT_VOXEL / 1000, level, EXPORT_BOUNDS)
    other = dict(cameras[1], intrinsic=cameras[1]['intrinsic'] * numpy.float32(1.25))
    if is_ndc:
        with pytest.raises(RuntimeError, match='ndc.*focal length'):
            harness.export_density_mesh(model, cfg, [cameras[0], other], tmp_path / 'bad.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS)
    else:
        harness.export_density_mesh(model, cfg, [cameras[0], other], tmp_path / 'other.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS)
    visible_cfg, visible, _ = seeded_model('config1', 'fp32', 1.0, predict_visibility=True)
    with pytest.raises(NotImplementedError, match='predict_visibility'):
        harness.export_density_mesh(visible, visible_cfg, cameras, tmp_path / 'bad.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS)
    assert not (tmp_path / 'bad.ply').exists()
