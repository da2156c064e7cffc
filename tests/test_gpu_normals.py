"""Normal maps on a real MI355X: the selection of a render's samples, the compositing of the field's normals, the depth-map normals
and the picture (csrc/normals.hip) against the restatement of tests/normals_reference.py; ``harness.predict_normals`` and the
``normals=True`` exports against the calls composed by hand; the native program.  Fixed-order fp64 arithmetic on both sides: bit for
bit, held to one float32 ulp -- the project's bound for fp64 results rounded to float."""
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import geometry, harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import field_gradient_reference as gref
from tests import normals_reference as nref
from tests import test_normals_host as cases
from tests.test_gpu_field import seeded_model
from tests.test_gpu_mesh import assert_bits_or_one_ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def on_device(array):
    return torch.from_numpy(numpy.array(array)).to(DEV)          # (a copy: the shared fixtures are read-only)


def host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


# ------------------------------------------------------------------------------------------------------------------ 1 the selection
@pytest.mark.parametrize('rays,samples', [(r, s) for r in cases.SELECTION_RAYS for s in cases.SELECTION_SAMPLES] + [cases.SELECTION_WIDE])
def test_selection_equals_the_restatement(rays, samples):
    origins, dirs, z_vals, weights = cases.selection_case(rays, samples)
    assert numpy.isnan(weights).sum() == 1
    if rays >= 7:
        assert not weights[4].any() and (weights[6] >= 0.5).all()
    device = [on_device(a) for a in (origins, dirs, z_vals, weights)]
    for min_weight in (0.0, 0.25):
        want = nref.select_ray_samples(origins, dirs, z_vals, weights, min_weight)
        got = ops.select_ray_samples(*device, min_weight)
        assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32] and all(t.is_cuda for t in got)
        offsets, sample, points = host(*got)
        assert offsets.shape == (rays + 1,) and numpy.array_equal(offsets, want[0])
        assert numpy.array_equal(sample, want[1]) and points.shape == (len(sample), 3)
        assert points.tobytes() == want[2].tobytes()
        again = host(*ops.select_ray_samples(*device, min_weight))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (offsets, sample, points)))
    if rays * samples >= 64:
        assert 0 < len(sample) < rays * samples


def test_selection_of_nothing_and_of_everything():
    none = ops.select_ray_samples(torch.empty((0, 3), device=DEV), torch.empty((0, 3), device=DEV), torch.empty((0, 7), device=DEV),
                                  torch.empty((0, 7), device=DEV))
    assert host(none[0])[0].tolist() == [0] and tuple(none[1].shape) == (0,) and tuple(none[2].shape) == (0, 3)
    origins, dirs, z_vals, weights = cases.selection_case(65, 7)
    empty = ops.select_ray_samples(on_device(origins), on_device(dirs), on_device(z_vals), on_device(weights), 1.0)       # no weight exceeds 1
    assert not host(empty[0])[0].any() and tuple(empty[1].shape) == (0,) and tuple(empty[2].shape) == (0, 3)
    no_samples = ops.select_ray_samples(on_device(origins), on_device(dirs), torch.empty((65, 0), device=DEV), torch.empty((65, 0), device=DEV))
    assert host(no_samples[0])[0].tolist() == [0] * 66 and tuple(no_samples[1].shape) == (0,)
    full = numpy.abs(weights) + numpy.float32(1.0)
    full[numpy.isnan(full)] = 1.0
    everything = host(*ops.select_ray_samples(on_device(origins), on_device(dirs), on_device(z_vals), on_device(full), -1.0))
    assert everything[0].tolist() == list(range(0, 65 * 7 + 1, 7)) and everything[1].tolist() == list(range(65 * 7))
    with pytest.raises(RuntimeError, match='z_vals'):
        ops.select_ray_samples(on_device(origins), on_device(dirs), on_device(z_vals[:, :6]), on_device(weights))
    with pytest.raises(RuntimeError, match='rays_d'):
        ops.select_ray_samples(on_device(origins), on_device(dirs[:64]), on_device(z_vals), on_device(weights))
    with pytest.raises(RuntimeError, match='weights'):
        ops.select_ray_samples(on_device(origins), on_device(dirs), on_device(z_vals), on_device(weights).double())
    with pytest.raises(RuntimeError, match='min_weight'):
        ops.select_ray_samples(on_device(origins), on_device(dirs), on_device(z_vals), on_device(weights), float('nan'))


# ------------------------------------------------------------------------------------------------------------------ 2 the compositing
@pytest.mark.parametrize('with_ndc', [False, True])
def test_compositing_equals_the_restatement(with_ndc):
    points, grad, offsets, sample, weights, ndc = cases.composite_case(with_ndc)
    want_normal, want_strength = nref.composite_normals(points, grad, offsets, sample, weights, ndc)
    device = [on_device(a) for a in (points, grad, offsets, sample, weights)]
    got = ops.composite_normals(*device, ndc)
    assert [t.dtype for t in got] == [torch.float32, torch.float32] and [tuple(t.shape) for t in got] == [(300, 3), (300,)]
    normal, strength = host(*got)
    assert_bits_or_one_ulp(normal, want_normal, f'composited normals, ndc {with_ndc}')
    assert_bits_or_one_ulp(strength, want_strength, f'strength, ndc {with_ndc}')
    nothing = want_strength == 0
    assert numpy.array_equal(strength == 0, nothing) and not normal[nothing].any() and nothing[3] and nothing[40]
    assert 2 <= int(nothing.sum()) < 150
    length = numpy.linalg.norm(normal.astype(numpy.float64), axis=1)
    assert (numpy.abs(length[~nothing] - 1.0) < 1e-6).all()
    if with_ndc:       # the samples at and past the far plane, nearer than the near plane, and the NaN, take no part
        usable = numpy.array([nref.sample_normal([float(v) for v in q], [float(v) for v in g], ndc)[1] for q, g in zip(points, grad)])
        z = points[:, 2].astype(numpy.float64)
        assert not usable[10] and not usable[12] and not usable[(z >= 1.0) | (z < -1.0)].any() and usable[(z < 1.0) & (z >= -1.0)].any()
    again = host(*ops.composite_normals(*device, ndc))
    assert again[0].tobytes() == normal.tobytes() and again[1].tobytes() == strength.tobytes()
    # a ray's bytes do not depend on the other rays of the call
    for first, last in ((0, 100), (100, 101), (37, 300)):
        lo, hi = int(offsets[first]), int(offsets[last])
        part = host(*ops.composite_normals(on_device(points[lo:hi]), on_device(grad[lo:hi]), on_device(offsets[first:last + 1] - lo),
                                           on_device(sample[lo:hi] - first * 16), on_device(weights[first:last]), ndc))
        assert part[0].tobytes() == normal[first:last].tobytes() and part[1].tobytes() == strength[first:last].tobytes()
    none = ops.composite_normals(device[0][:0], device[1][:0], torch.zeros(1, dtype=torch.int32, device=DEV), device[3][:0],
                                 torch.empty((0, 16), device=DEV), ndc)
    assert tuple(none[0].shape) == (0, 3) and tuple(none[1].shape) == (0,)
    with pytest.raises(RuntimeError, match='grad'):
        ops.composite_normals(device[0], device[1][:-1], device[2], device[3], device[4], ndc)
    with pytest.raises(RuntimeError, match='offsets'):
        ops.composite_normals(device[0], device[1], device[2][:-1], device[3], device[4], ndc)
    with pytest.raises(RuntimeError, match='sample'):
        ops.composite_normals(device[0], device[1], device[2], device[3].long(), device[4], ndc)
    with pytest.raises(RuntimeError, match='ndc'):
        ops.composite_normals(*device, (1.0, 1.0, -2.0))


def test_a_planar_slabs_rays_get_the_slabs_normal():
    """Density k max(0, a . x - b) fed as a callable; weights alpha-composited in float64 from it.  Every sample inside has the
    gradient g = k a, so every entering ray's sum is (sum of its selected weights) x (-g / |g|): the normal is -a and the strength the
    float64 sum of the selected weights, each to the rounding of a few fp64 operations and one float32 store -- one float32 ulp."""
    origins, dirs, z_vals, weights, _, inside = cases.slab_case()
    asked = []

    def gradient(points):
        asked.append(int(points.shape[0]))
        return on_device(cases.slab_gradient(points.cpu().numpy()))

    normal, strength, selected = geometry.ray_normals(gradient, on_device(origins), on_device(dirs), on_device(z_vals), on_device(weights))
    assert asked == [selected] and selected == int((weights > 0).sum()) > 0
    normal, strength = host(normal, strength)
    hit = (weights > 0).any(axis=1)
    assert int(hit.sum()) >= 80 and 20 <= int((~hit).sum()) and (hit <= inside.any(axis=1)).all()
    want_normal = numpy.tile(cases.slab_normal().astype(numpy.float32), (int(hit.sum()), 1))
    assert_bits_or_one_ulp(normal[hit], want_normal, 'the slab\'s normal')
    sums = numpy.array([sum(float(w) for w in row if w > 0) for row in weights])
    assert_bits_or_one_ulp(strength[hit], sums[hit].astype(numpy.float32), 'the selected weights\' sum')
    assert not normal[~hit].any() and not strength[~hit].any()
    with pytest.raises(RuntimeError, match='query_gradient'):
        geometry.ray_normals(lambda p: p[:, 0], on_device(origins), on_device(dirs), on_device(z_vals), on_device(weights))
    missing = geometry.ray_normals(gradient, on_device(origins[::6]), on_device(dirs[::6]), on_device(z_vals[::6]), on_device(weights[::6]))
    assert missing[2] == 0 and not missing[0].any() and not missing[1].any() and asked == [selected]       # nothing selected: the field is not asked


# ------------------------------------------------------------------------------------------------------------------ 3 depth normals
@pytest.mark.parametrize('views', [1, 3])
@pytest.mark.parametrize('height,width', cases.DEPTH_FRAMES)
def test_depth_normals_equal_the_restatement(views, height, width):
    depth, mask, cameras, extrinsics, intrinsics = cases.depth_case(views, height, width)
    if depth.size >= 20:
        kinds = depth[mask != 0]
        assert (kinds == 0).any() and (kinds < 0).any() and numpy.isnan(kinds).any() and numpy.isinf(kinds).any() and (mask == 0).any()
    plain = None
    for edge_threshold, use_mask in ((None, False), (None, True), (0.05, True)):
        want = nref.depth_normals(depth, cameras, mask if use_mask else None, edge_threshold)
        got = ops.depth_normals(on_device(depth), on_device(cameras), on_device(mask) if use_mask else None, edge_threshold)
        assert got.dtype == torch.float32 and tuple(got.shape) == (views, height, width, 3) and got.is_cuda
        got = got.cpu().numpy()
        assert_bits_or_one_ulp(got, want, f'depth normals {views} x {height} x {width}, edge {edge_threshold}, mask {use_mask}')
        nothing = ~want.any(axis=-1)
        assert not got[nothing].any()
        invalid = ~(numpy.isfinite(depth) & (depth > 0) & ((mask != 0) | (not use_mask)))
        assert nothing[invalid].all()
        length = numpy.linalg.norm(got.astype(numpy.float64), axis=-1)
        assert (numpy.abs(length[~nothing] - 1.0) < 1e-6).all()
        if min(height, width) == 1:
            assert nothing.all()                                             # a row or a column has no second tangent
        elif depth.size >= 20:
            assert (~nothing).any() and nothing.any()
        if edge_threshold is None and use_mask:
            plain = want
    if height * width >= 500:       # the threshold takes tangents away at the steps: normals change beside them
        assert (want != plain).any()
    through = geometry.depth_normals(on_device(depth), extrinsics, intrinsics, on_device(mask), 0.05).cpu().numpy()
    assert through.tobytes() == got.tobytes()
    boolean = ops.depth_normals(on_device(depth), on_device(cameras), on_device(mask != 0), 0.05).cpu().numpy()
    assert boolean.tobytes() == got.tobytes()


def test_a_fronto_parallel_plane_gives_exactly_the_axis():
    depth, cameras = cases.fronto_parallel_case()
    for edge_threshold in (None, 0.05):
        got = ops.depth_normals(on_device(depth), on_device(cameras), None, edge_threshold).cpu().numpy()
        assert numpy.array_equal(got.reshape(-1, 3), numpy.tile(numpy.float32([0.0, 0.0, -1.0]), (108, 1)))


def test_an_oblique_planes_normals_are_within_the_depth_roundings_reach():
    """The plane n . X = c before an identity pose; its depth d = c / (n . r), r = inv(K) (x, y, 1), is rounded to float32, which
    moves a pixel's point P = d r along its ray by at most half an ulp: |dP| <= 2^-24 |P| <= 2^-24 D, D the farthest point.  A
    tangent is the difference of two points: |dt| <= 2^-23 D.  The cross product c = t_x x t_y, which for the exact points is
    parallel to n, moves by |dc| <= |dt_x| |t_y| + |t_x| |dt_y| + |dt_x| |dt_y| <= 2^-23 D (|t_x| + |t_y|) + (2^-23 D)^2.  For any two
    vectors | a / |a| - b / |b| | <= 2 |a - b| / |b|, so the unit normal moves by at most 2 |dc| / |c|; the fp64 arithmetic adds
    nothing visible, and the float32 store at most 2^-24 a component, less than 2^-23 in length.  tests/test_normals_host.py
    oblique_plane_case evaluates that bound per pixel from the exact points (the border pixels with their one-sided tangents)."""
    depth, cameras, bound = cases.oblique_plane_case()
    got = ops.depth_normals(on_device(depth), on_device(cameras)).cpu().numpy()[0].astype(numpy.float64)
    want = -cases.OBLIQUE_NORMAL if cases.OBLIQUE_NORMAL[2] > 0 else cases.OBLIQUE_NORMAL        # facing the camera at the origin: n . (0 - P) > 0
    assert float(want @ want) == pytest.approx(1.0, abs=1e-15)
    error = numpy.linalg.norm(got - want, axis=-1)
    print(f'oblique plane: worst |normal - n| = {error.max():.3e}, bound there {bound.reshape(-1)[error.argmax()]:.3e}, '
          f'smallest bound {bound.min():.3e}, largest ratio {float((error / bound).max()):.3f}')
    assert bound.max() < 1e-3 and (error <= bound).all()
    restated = nref.depth_normals(depth, cameras)
    assert_bits_or_one_ulp(got.astype(numpy.float32), restated[0], 'oblique plane')


# ------------------------------------------------------------------------------------------------------------------ 4 the picture
def test_the_picture_equals_the_integer_restatement():
    normals, rotation = cases.picture_case()
    for matrix in (None, rotation, torch.from_numpy(rotation)):
        got = ops.normals_to_u8(on_device(normals), matrix)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (500, 3) and got.is_cuda
        want = nref.normals_to_u8(normals, None if matrix is None else rotation)
        assert numpy.array_equal(got.cpu().numpy(), want)
    assert want[0].tolist() == [128, 128, 128] and not want[6].any()
    plain = nref.normals_to_u8(normals)
    assert plain[1].tolist() == [255, 128, 128] and plain[2].tolist() == [128, 0, 128] and plain[4].tolist() == [0, 0, 0] and plain[5].tolist() == [255] * 3
    shaped = ops.normals_to_u8(on_device(normals[:480].reshape(8, 20, 3, 3))[:, :, 0], rotation)          # a strided view of (8, 20, 3)
    assert tuple(shaped.shape) == (8, 20, 3)
    assert numpy.array_equal(shaped.cpu().numpy(), nref.normals_to_u8(normals[:480].reshape(8, 20, 3, 3)[:, :, 0], rotation))
    camera = synth.camera('fern', 1, resolution=(8, 6))
    assert torch.equal(geometry.normals_to_u8(on_device(normals), camera),
                       ops.normals_to_u8(on_device(normals), numpy.asarray(camera['pose'], dtype=numpy.float64)[:3, :3]))
    assert torch.equal(geometry.normals_to_u8(on_device(normals)), ops.normals_to_u8(on_device(normals)))
    assert tuple(ops.normals_to_u8(torch.empty((0, 3), device=DEV)).shape) == (0, 3)
    with pytest.raises(RuntimeError, match='normals'):
        ops.normals_to_u8(on_device(normals[:, :2]))
    with pytest.raises(RuntimeError, match='rotation'):
        ops.normals_to_u8(on_device(normals), numpy.eye(4))


# ------------------------------------------------------------------------------------------------------------------ 5 the model
MODEL_SAMPLES = 12
MODEL_FRAME = (8, 6)


def case_model(precision, ndc, fine=False):
    """The seeded 8 x 128 / 64 case of tests/field_gradient_reference.py as a renderer of few samples; ``fine``: a fine level too,
    seeded the same way."""
    cfg = gref.case_configs('w128_views', precision)
    cfg['data_loader']['ndc'] = bool(ndc)
    cfg['model']['coarse_mlp']['num_samples'] = MODEL_SAMPLES
    if not fine:
        model = get_model(cfg, None)
        model.load_state_dict(gref.case_state('w128_views'))
        return cfg, model.to(DEV).eval()
    cfg['model']['fine_mlp'] = dict(cfg['model']['coarse_mlp'], num_samples=MODEL_SAMPLES + 4)
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    _, seed, gain, shift, _, _ = gref.CASES['w128_views']
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed, gain, shift).items()})
    return cfg, model.to(DEV).eval()


@pytest.mark.parametrize('precision,ndc,fine', [('fp32', False, False), ('fp32', True, False), ('bf16', False, False), ('bf16', True, False),
                                                ('fp32', True, True), ('bf16', False, True)])
def test_predict_normals_is_the_composition_by_hand(precision, ndc, fine):
    cfg, model = case_model(precision, ndc, fine)
    camera = synth.camera('fern', 1, resolution=MODEL_FRAME)
    h, w = MODEL_FRAME
    device = torch.device(DEV)
    out = harness.predict_normals(model, cfg, camera, device)
    assert sorted(out) == ['depth', 'depth_normal', 'depth_normal_image', 'normal', 'normal_image', 'normal_strength', 'selected_fraction']
    # by hand, from one whole-frame render
    suffix = '_fine' if fine else '_coarse'
    batch = harness.frame_batch(camera, ndc, device)
    with torch.no_grad():
        rendered = model(batch, retraw=True)
    weights, z_vals = rendered[f'weights{suffix}'], rendered[f'z_vals{suffix}']
    samples = MODEL_SAMPLES + (MODEL_SAMPLES + 4 if fine else 0)
    assert tuple(weights.shape) == (h * w, samples) == tuple(z_vals.shape)
    rays = (batch['rays_o_ndc'], batch['rays_d_ndc']) if ndc else (batch['rays_o'], batch['rays_d'])
    parameters = geometry.ndc_parameters(camera) if ndc else None
    offsets, sample, points = ops.select_ray_samples(*rays, z_vals, weights, 0.0)
    gradient = model.query_gradient(points)
    normal, strength = ops.composite_normals(points, gradient['grad'], offsets, sample, weights, parameters)
    assert torch.equal(out['normal'], normal.reshape(h, w, 3)) and torch.equal(out['normal_strength'], strength.reshape(h, w))
    shown = harness.display_outputs(cfg, camera['resolution'], rendered)
    assert torch.equal(out['depth'], shown['depth'])
    extrinsic, intrinsic = geometry.camera_matrices(camera)
    depth_normal = geometry.depth_normals(shown['depth'][None], [extrinsic], [intrinsic])[0]
    assert torch.equal(out['depth_normal'], depth_normal)
    assert torch.equal(out['normal_image'], geometry.normals_to_u8(normal.reshape(h, w, 3), camera))
    assert torch.equal(out['depth_normal_image'], geometry.normals_to_u8(depth_normal, camera))
    assert out['normal_image'].dtype == torch.uint8 and tuple(out['normal_image'].shape) == (h, w, 3) == tuple(out['depth_normal_image'].shape)
    fraction = out['selected_fraction']
    assert isinstance(fraction, float) and 0.0 < fraction <= 1.0 and fraction == int(sample.shape[0]) / (h * w * samples)
    length = out['normal'].double().norm(dim=-1)
    assert bool((((length - 1.0).abs() < 1e-6) | (length == 0)).all()) and bool((length > 0).any())
    assert bool(((length == 0) == (out['normal_strength'] == 0)).all())
    depth_length = out['depth_normal'].double().norm(dim=-1)
    assert bool((((depth_length - 1.0).abs() < 1e-6) | (depth_length == 0)).all())
    print(f'{precision} ndc {ndc} fine {fine}: selected {fraction:.3f}, rays with a normal {int((length > 0).sum())} of {h * w}, '
          f'pixels with a depth normal {int((depth_length > 0).sum())}')
    # blocks of rays and of gradient points, a threshold and an edge test reach the calls
    blocks = harness.predict_normals(model, cfg, camera, device, ray_block=17, gradient_block=50)
    for key in out:
        assert torch.equal(blocks[key], out[key]) if isinstance(out[key], torch.Tensor) else blocks[key] == out[key], key
    picky = harness.predict_normals(model, cfg, camera, device, min_weight=0.02, edge_threshold=0.01)
    kept = ops.select_ray_samples(*rays, z_vals, weights, 0.02)
    assert picky['selected_fraction'] == int(kept[1].shape[0]) / (h * w * samples) < fraction
    assert torch.equal(picky['depth_normal'], geometry.depth_normals(shown['depth'][None], [extrinsic], [intrinsic], None, 0.01)[0])
    # the pictures go through the image writers unchanged
    assert len(harness.png_files(out['normal_image'][None])) == 1


def test_a_bf16_models_normals_come_from_the_fp32_field():
    """``query_gradient`` is always fp32: at the same selected points a bf16 model's gradient is its fp32 twin's, byte for byte."""
    _, fp32 = case_model('fp32', False)
    _, bf16 = case_model('bf16', False)
    points = on_device(gref.case('w128_views')['points'])
    assert torch.equal(fp32.query_gradient(points)['grad'], bf16.query_gradient(points)['grad'])


def test_models_without_a_gradient_are_refused_before_anything_is_rendered(tmp_path):
    camera = synth.camera('fern', 1, resolution=MODEL_FRAME)
    device = torch.device(DEV)
    for overrides, match in ((dict(predict_visibility=True), 'predict_visibility'),
                             (dict(points_net_depth=6, points_net_width=96, views_net_width=48), 'fused MLP shapes only.*layered')):
        cfg, model, _ = seeded_model('config1', 'fp32', 1.0, **overrides)
        renders = []
        model.register_forward_pre_hook(lambda *args: renders.append(1))
        with pytest.raises(NotImplementedError, match=match):
            harness.predict_normals(model, cfg, camera, device)
        with pytest.raises(NotImplementedError, match=match):
            harness.export_point_cloud(model, cfg, [camera], tmp_path / 'cloud.ply', device, min_views=0, normals=True)
        with pytest.raises(NotImplementedError, match=match):
            harness.export_mesh(model, cfg, [camera], tmp_path / 'mesh.ply', device, 0.5, normals=True)
        with pytest.raises(NotImplementedError, match=match):
            model.check_query_gradient()
        assert not renders and not (tmp_path / 'cloud.ply').exists() and not (tmp_path / 'mesh.ply').exists()
        harness.predict_frame(model, cfg, camera, device)                       # the model itself renders
        assert renders
    cfg, model = case_model('fp32', False)
    with pytest.raises(RuntimeError, match='ray_block'):
        harness.predict_normals(model, cfg, camera, device, ray_block=0)


# ------------------------------------------------------------------------------------------------------------------ 6 the exports
@pytest.mark.parametrize('kind,shift', [('config1', 4.0), ('config2', 2.0)])
def test_exports_with_normals(tmp_path, kind, shift):
    cfg, model, _ = seeded_model(kind, 'fp32', shift)
    is_ndc = bool(cfg['data_loader']['ndc'])
    cameras = [synth.camera('fern', pose, resolution=(12, 15)) for pose in (0, 1, 2)]
    ndc = geometry.ndc_parameters(cameras[0]) if is_ndc else None
    device = torch.device(DEV)
    field = lambda q: model.query_gradient(q)['grad']
    # the point cloud, thinned: the normals are taken at the written points
    plain = harness.export_point_cloud(model, cfg, cameras, tmp_path / 'cloud.ply', device, 0.5, 0, voxel_size=0.5)
    explicit = harness.export_point_cloud(model, cfg, cameras, tmp_path / 'cloud_false.ply', device, 0.5, 0, 0.5, None, False)
    out = harness.export_point_cloud(model, cfg, cameras, tmp_path / 'cloud_normals.ply', device, 0.5, 0, voxel_size=0.5, normals=True)
    assert 'normals' not in plain and 'normals' not in explicit and sorted(out) == sorted(list(plain) + ['normals'])
    for key in ('points', 'colours', 'counts'):
        assert torch.equal(out[key], plain[key]), key
    points, normals = out['points'], out['normals']
    assert normals.dtype == torch.float32 and tuple(normals.shape) == tuple(points.shape) and 0 < len(points) <= out['fused_points']
    assert torch.equal(normals, geometry.field_normals(field, points, ndc))
    length = normals.double().norm(dim=1)
    assert bool((((length - 1.0).abs() < 1e-6) | (length == 0)).all()) and bool((length > 0).any())
    data = (tmp_path / 'cloud_normals.ply').read_bytes()
    assert data == geometry.ply_bytes(points, out['colours'], normals)
    records = cases.parse_ply_with_normals(data)
    assert len(records) == len(points) and records.dtype.itemsize == 27
    assert numpy.array_equal(numpy.stack([records[k] for k in ('nx', 'ny', 'nz')], axis=1), normals.cpu().numpy())
    assert numpy.array_equal(numpy.stack([records[k] for k in ('x', 'y', 'z')], axis=1), points.cpu().numpy())
    before = (tmp_path / 'cloud.ply').read_bytes()
    assert before == cases.todays_ply_bytes(points.cpu().numpy(), out['colours'].cpu().numpy()) == (tmp_path / 'cloud_false.ply').read_bytes()
    # the mesh
    voxel = float((points.max(dim=0)[0] - points.min(dim=0)[0]).max()) / 12
    plain = harness.export_mesh(model, cfg, cameras, tmp_path / 'mesh.ply', device, voxel)
    explicit = harness.export_mesh(model, cfg, cameras, tmp_path / 'mesh_false.ply', device, voxel, None, None, 1, None, None, False)
    out = harness.export_mesh(model, cfg, cameras, tmp_path / 'mesh_normals.ply', device, voxel, normals=True)
    assert 'normals' not in plain and 'normals' not in explicit and sorted(out) == sorted(list(plain) + ['normals'])
    for key in ('vertices', 'colours', 'views', 'triangles', 'tsdf', 'weight'):
        assert torch.equal(out[key], plain[key]), key
    vertices, normals = out['vertices'], out['normals']
    assert normals.dtype == torch.float32 and tuple(normals.shape) == tuple(vertices.shape) and len(vertices) > 0
    assert torch.equal(normals, geometry.field_normals(field, vertices, ndc))
    data = (tmp_path / 'mesh_normals.ply').read_bytes()
    assert data == geometry.ply_mesh_bytes(vertices, out['colours'], out['triangles'], normals)
    assert len(data.split(b'end_header\n', 1)[1]) == 27 * len(vertices) + 13 * len(out['triangles'])
    before = (tmp_path / 'mesh.ply').read_bytes()
    assert before == geometry.ply_mesh_bytes(vertices, out['colours'], out['triangles']) == (tmp_path / 'mesh_false.ply').read_bytes()
    assert len(before.split(b'end_header\n', 1)[1]) == 15 * len(vertices) + 13 * len(out['triangles'])


# ------------------------------------------------------------------------------------------------------------------ 7 the C ABI alone
def test_normals_abi_program_equals_the_restatement(tmp_path):
    """tests/native/normals_abi_smoke.cpp, compiled against the headers and run without PyTorch in its process, on the fixture of
    tests/test_normals_host.py: the four entry points (the selection is two calls)."""
    exe = cases.compile_smoke(str(tmp_path))
    (tmp_path / 'fixture').write_bytes(cases.native_fixture())
    r = subprocess.run([exe, str(tmp_path / 'fixture')], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'normals_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
    assert f'normals_abi_smoke: {cases.NATIVE_RAYS} rays of {cases.NATIVE_SAMPLES} samples' in r.stdout
    assert 'bytes differ [0]' in r.stdout
