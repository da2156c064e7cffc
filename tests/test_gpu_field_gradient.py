"""The field's gradient on a real MI355X: ``model.query_gradient`` (the storing forward, the fp32 backward chain without its
weight-gradient launches, csrc/mlp_input_grad.hip) against the float64 autograd of the oracle's MLP, ``ops.field_normals`` against
the restatement of tests/field_gradient_reference.py, and ``harness.export_density_mesh(normals=True)`` against the calls composed
by hand.

The gradient of a ReLU network jumps where a hidden pre-activation crosses 0: a point is compared only where the oracle's float64
forward keeps every trunk pre-activation farther from 0 than 1e-5 of its layer's largest (tests/field_gradient_reference.py; the
host tests assert that at most a quarter of a case's points is left out and that most compared ones have sigma > 0).  The bound is
measured, not guessed: the oracle's own float32 autograd against its float64 autograd on the same compared points, relative to
max |grad| -- 2.4e-7 .. 5.3e-7 depending on the case and the host's float32 sums -- times four, the margin of
tests/test_field_host.py.  Measured on an MI355X: the device is 3.1e-7 .. 4.8e-7 from the float64 oracle on those cases."""
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import geometry, harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import field_gradient_reference as gref
from tests import field_reference as ref
from tests import mesh_reference, util
from tests.test_field_gradient_host import compile_smoke, native_fixture, parse_ply_mesh_with_normals, todays_ply_mesh_bytes
from tests.test_gpu_field import EXPORT_BOUNDS, EXPORT_VOXEL, seeded_model
from tests.test_gpu_mesh import assert_bits_or_one_ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIGMA_TOLERANCE = 1e-5          # tests/test_gpu_field.py holds the fp32 ``model.query`` to the oracle at this (util.rel_linf)


def on_device(array):
    return torch.from_numpy(numpy.array(array)).to(DEV)          # (a copy: the shared fixtures are read-only)


def case_model(name, precision='fp32'):
    model = get_model(gref.case_configs(name, precision), None)
    model.load_state_dict(gref.case_state(name))
    return model.to(DEV).eval()


# ------------------------------------------------------------------------------------------------------------------ 1 the gradient
@pytest.mark.parametrize('name', sorted(gref.CASES))
def test_query_gradient_matches_the_oracles_autograd(name):
    case = gref.case(name)
    model = case_model(name)
    points = on_device(case['points'])
    whole = None
    for count in reversed(gref.POINT_COUNTS):
        out = model.query_gradient(points[:count])
        assert sorted(out) == ['grad', 'sigma'] and out['grad'].dtype == out['sigma'].dtype == torch.float32
        assert tuple(out['grad'].shape) == (count, 3) and tuple(out['sigma'].shape) == (count,)
        grad, sigma = out['grad'].cpu().numpy(), out['sigma'].cpu().numpy()
        compared = case['compared'][:count]
        assert numpy.isfinite(grad).all()                                                 # the left-out points too
        error = float(numpy.abs(grad[compared].astype(numpy.float64) - case['grad'][:count][compared]).max()) / case['scale']
        print(f'{name} N = {count}: {int(compared.sum())} compared, error {error:.3e} of max |grad| [{case["bound"]:.3e} = 4 x {case["measured"]:.3e}]')
        if count == gref.POINT_COUNTS[-1]:
            util.observe(f'field/gradient/{name}', f'error {error:.2e} [{case["bound"]:.2e}], {int((~compared).sum())} of {count} left out')
            whole = out
        assert compared.any() and error <= case['bound'], (count, error, case['bound'])
        assert not grad[sigma == 0].any()                                                 # exact zeros where the density's ReLU is closed
        assert util.rel_linf(out['sigma'], model.query(points[:count])['sigma']) < SIGMA_TOLERANCE
        assert torch.equal(out['grad'], whole['grad'][:count]) and torch.equal(out['sigma'], whole['sigma'][:count])    # a point's own
    if name != 'w256_ptsaug':
        assert (whole['sigma'] == 0).any()
    blocks = model.query_gradient(points, point_block=257)
    again = model.query_gradient(points)
    for other in (blocks, again):
        assert torch.equal(other['grad'], whole['grad']) and torch.equal(other['sigma'], whole['sigma'])
    assert torch.equal(model.query_gradient(points, mlp='coarse_mlp')['grad'], whole['grad'])
    none = model.query_gradient(points[:0])
    assert tuple(none['grad'].shape) == (0, 3) and tuple(none['sigma'].shape) == (0,)


def test_a_bf16_model_returns_its_fp32_twins_bytes():
    case = gref.case('w256_views')
    points = on_device(case['points'])
    fp32, bf16 = case_model('w256_views'), case_model('w256_views', 'bf16')
    want, got = fp32.query_gradient(points), bf16.query_gradient(points)
    assert torch.equal(got['grad'], want['grad']) and torch.equal(got['sigma'], want['sigma'])
    # the model's own render stream keeps its precision and mode: a query before and after gives the same bytes
    before = bf16.query(points)['sigma']
    bf16.query_gradient(points[:40])
    assert torch.equal(bf16.query(points)['sigma'], before) and not torch.equal(before, want['sigma'])


def test_input_gradient_scales_with_d_sigma():
    """The entry point itself: d_sigma is a factor per point (powers of two: exact), a caller's workspace is accepted."""
    case = gref.case('w128_views')
    params = [p.to(DEV) for p in synth.abi_param_list(gref.case_state('w128_views'), gref.PREFIX)]
    mlp = ops.PackedMlp(gref.case_configs('w128_views')['model']['coarse_mlp'], DEV)
    mlp.pack(params, ops.PRECISION_FP32, True)
    points = on_device(case['points'][:130])
    down = torch.tensor([0.0, 0.0, -1.0], device=DEV).expand(130, 3).contiguous()
    sigma, _, saved = mlp.forward_train(points, torch.zeros_like(points), down, torch.zeros((130, 1), device=DEV), None, ops.PRECISION_FP32)
    plain = mlp.input_gradient(params, saved, sigma)
    factor = torch.tensor([2.0, -4.0, 0.0, 0.5], device=DEV).repeat(33)[:130]
    work = torch.empty(mlp.input_gradient_workspace_floats(130) + 7, device=DEV)
    scaled = mlp.input_gradient(params, saved, sigma, factor, work)
    assert torch.equal(scaled, plain * factor[:, None]) and plain.abs().max() > 0
    with pytest.raises(RuntimeError, match='work'):
        mlp.input_gradient(params, saved, sigma, factor, work[:100])
    with pytest.raises(RuntimeError, match='saved'):
        mlp.input_gradient(params, saved[:1000], sigma)
    with pytest.raises(RuntimeError, match='parameter tensors'):
        mlp.input_gradient(params[:-1], saved, sigma)


# ------------------------------------------------------------------------------------------------------------------ 2 the normals
def test_field_normals_equal_the_restatement():
    rng = numpy.random.default_rng(11)
    _, _, ndc = ref.fern_cameras()
    near = ndc[2]
    points = rng.uniform(-1.5, 1.5, (1000, 3)).astype(numpy.float32)
    points[:, 2] = rng.uniform(-near - 5.0, -near + 0.4, 1000).astype(numpy.float32)       # some nearer than the near plane
    points[5, 2] = numpy.float32(-near)                                                    # on it (float32 of near: in front or not, both sides agree)
    points[6, 2] = numpy.nan
    grad = (rng.standard_normal((1000, 3)) * 10.0 ** rng.uniform(-3, 3, (1000, 1))).astype(numpy.float32)
    grad[::17] = 0.0                                                                       # closed densities
    grad[3] = [numpy.inf, 1.0, 0.0]
    grad[4] = [numpy.nan, 1.0, 0.0]
    grad[8] = [3.0e38, 3.0e38, 0.0]                                                        # finite in fp64
    behind = ~(points[:, 2].astype(numpy.float64) <= -near)
    assert 20 < int(behind.sum()) < 300
    for parameters in (None, ndc):
        want = gref.normals(points, grad, parameters)
        got = ops.field_normals(on_device(points), on_device(grad), parameters)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1000, 3) and got.is_cuda
        got = got.cpu().numpy()
        assert_bits_or_one_ulp(got, want, f'normals, ndc {parameters is not None}')
        assert not got[::17].any() and not got[3:5].any() and got[8].any()
        length = numpy.linalg.norm(got.astype(numpy.float64), axis=1)
        assert ((numpy.abs(length - 1.0) < 1e-6) | (length == 0)).all()
        if parameters is not None:
            assert not got[behind].any() and got[~behind].any()
        assert torch.equal(ops.field_normals(on_device(points), on_device(grad), parameters).cpu(), torch.from_numpy(got))
    assert tuple(ops.field_normals(torch.empty((0, 3), device=DEV), torch.empty((0, 3), device=DEV)).shape) == (0, 3)
    with pytest.raises(RuntimeError, match='grad'):
        ops.field_normals(on_device(points), on_device(grad[:10]))
    with pytest.raises(RuntimeError, match='ndc'):
        ops.field_normals(on_device(points), on_device(grad), (1.0, 1.0, 0.0))


# ------------------------------------------------------------------------------------------------------------------ 3 the export
def test_the_analytic_balls_normals_agree_with_its_winding():
    s = mesh_reference.scene()
    grid = (mesh_reference.GRID_LO, mesh_reference.GRID_VOXEL, mesh_reference.GRID_EXTENTS)
    query = lambda p: 40.0 * torch.clamp(1.0 - p.norm(dim=1) / 1.2, min=0.0)
    gradient = lambda p: torch.where((p.norm(dim=1, keepdim=True) < 1.2), -(40.0 / 1.2) * p / p.norm(dim=1, keepdim=True), torch.zeros_like(p))
    _, tsdf, weight = geometry.density_volume(query, *grid, s['extrinsics'], s['intrinsics'], ref.SCENE_RESOLUTION, ref.SPHERE_LEVEL)
    vertices, triangles = geometry.extract_mesh(tsdf, weight, *grid[:2])
    normals = geometry.field_normals(gradient, vertices)
    assert normals.dtype == torch.float32 and tuple(normals.shape) == tuple(vertices.shape) and len(vertices) > 500
    p, n, t = vertices.cpu().numpy().astype(numpy.float64), normals.cpu().numpy().astype(numpy.float64), triangles.cpu().numpy()
    assert numpy.abs(n - p / numpy.linalg.norm(p, axis=1, keepdims=True)).max() <= 1e-6       # radial, outwards
    assert_bits_or_one_ulp(normals.cpu().numpy(), gref.normals(vertices.cpu().numpy(), gradient(vertices).cpu().numpy()), 'ball normals')
    winding = numpy.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    proper = numpy.linalg.norm(winding, axis=1) > 0                                        # (marching tetrahedra keeps zero-area triangles)
    assert proper.mean() > 0.9
    for corner in range(3):
        assert ((winding * n[t[:, corner]]).sum(axis=1)[proper] > 0).all()
    with pytest.raises(RuntimeError, match='query_gradient'):
        geometry.field_normals(lambda q: q[:, 0], vertices)
    assert tuple(geometry.field_normals(gradient, vertices[:0]).shape) == (0, 3)


@pytest.mark.parametrize('kind,shift', [('config1', 1.0), ('config2', 2.0)])
def test_export_density_mesh_with_normals(tmp_path, kind, shift):
    cfg, model, _ = seeded_model(kind, 'fp32', shift)
    is_ndc = bool(cfg['data_loader']['ndc'])
    cameras, table, ndc = ref.fern_cameras()
    ndc = ndc if is_ndc else None
    device = torch.device(DEV)
    nodes, _ = ops.field_grid_points(EXPORT_BOUNDS[0], EXPORT_VOXEL, (17, 16, 15), on_device(table), (48, 64), ndc)
    densities = model.query(nodes)['sigma']
    level = float(densities[densities > 0].median())
    plain = harness.export_density_mesh(model, cfg, cameras, tmp_path / 'plain.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS)
    out = harness.export_density_mesh(model, cfg, cameras, tmp_path / 'normals.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS, normals=True)
    assert 'normals' not in plain and sorted(out) == sorted(list(plain) + ['normals'])
    for key in ('vertices', 'colours', 'views', 'triangles', 'sigma', 'tsdf', 'weight'):
        assert torch.equal(out[key], plain[key]), key
    vertices, triangles, normals = out['vertices'], out['triangles'], out['normals']
    assert normals.dtype == torch.float32 and tuple(normals.shape) == tuple(vertices.shape) and len(vertices) > 0
    # the calls composed by hand
    mlp_points = ops.field_point_views(vertices, on_device(table), (48, 64), ndc)[0]
    gradient = model.query_gradient(mlp_points)
    assert torch.equal(normals, ops.field_normals(vertices, gradient['grad'], ndc))
    assert torch.equal(normals, geometry.field_normals(lambda q: model.query_gradient(q, point_block=97)['grad'], vertices, ndc))
    length = normals.double().norm(dim=1)
    assert bool((((length - 1.0).abs() < 1e-6) | (length == 0)).all()) and float((length > 0).float().mean()) > 0.5
    assert bool((length[gradient['sigma'] == 0] == 0).all())
    # the files: with normals it parses back; without, the bytes are what they were before normals existed
    data = (tmp_path / 'normals.ply').read_bytes()
    assert data == geometry.ply_mesh_bytes(vertices, out['colours'], triangles, normals)
    records, faces = parse_ply_mesh_with_normals(data)
    assert numpy.array_equal(numpy.stack([records[k] for k in ('x', 'y', 'z')], axis=1), vertices.cpu().numpy())
    assert numpy.array_equal(numpy.stack([records[k] for k in ('nx', 'ny', 'nz')], axis=1), normals.cpu().numpy())
    assert numpy.array_equal(numpy.stack([records[k] for k in ('red', 'green', 'blue')], axis=1), out['colours'].cpu().numpy())
    assert numpy.array_equal(numpy.stack([faces[k] for k in ('a', 'b', 'c')], axis=1), triangles.cpu().numpy())
    before = (tmp_path / 'plain.ply').read_bytes()
    assert before == todays_ply_mesh_bytes(vertices.cpu().numpy(), out['colours'].cpu().numpy(), triangles.cpu().numpy())
    assert before == geometry.ply_mesh_bytes(vertices, out['colours'], triangles)
    explicit = harness.export_density_mesh(model, cfg, cameras, tmp_path / 'explicit.ply', device, EXPORT_VOXEL, level, EXPORT_BOUNDS, 1, 1 << 20,
                                           False)
    assert 'normals' not in explicit and (tmp_path / 'explicit.ply').read_bytes() == before


# ------------------------------------------------------------------------------------------------------------------ 4 refusals
def test_refusals_name_their_limit():
    points = torch.zeros((4, 3), device=DEV)
    _, visible, _ = seeded_model('config1', 'fp32', 1.0, predict_visibility=True)
    with pytest.raises(NotImplementedError, match='predict_visibility'):
        visible.query_gradient(points)
    _, layered, _ = seeded_model('config1', 'fp32', 1.0, points_net_depth=6, points_net_width=96, views_net_width=48)
    assert tuple(layered.query(points)['sigma'].shape) == (4,)                            # the layered path answers point queries ...
    with pytest.raises(NotImplementedError, match='fused MLP shapes only.*layered'):      # ... but has no input gradient
        layered.query_gradient(points)
    # the entry point itself: a predict_visibility descriptor, and a stream packed for rendering only
    case = gref.case('w128_views')
    params = [p.to(DEV) for p in synth.abi_param_list(gref.case_state('w128_views'), gref.PREFIX)]
    mlp_cfg = gref.case_configs('w128_views')['model']['coarse_mlp']
    mlp = ops.PackedMlp(mlp_cfg, DEV)
    mlp.pack(params, ops.PRECISION_FP32, True)
    pts = on_device(case['points'][:8])
    down = torch.tensor([0.0, 0.0, -1.0], device=DEV).expand(8, 3).contiguous()
    sigma, _, saved = mlp.forward_train(pts, torch.zeros_like(pts), down, torch.zeros((8, 1), device=DEV), None, ops.PRECISION_FP32)
    want = mlp.input_gradient(params, saved, sigma)
    mlp.pack(params, ops.PRECISION_FP32, False)                  # (an fp32 pack writes the chain's transposed stream in either mode)
    assert torch.equal(mlp.input_gradient(params, saved, sigma), want)
    for training in (False, True):                               # a 16-bit render or training stream holds no fp32 operands
        mlp.pack(params, ops.PRECISION_BF16, training)
        with pytest.raises(RuntimeError, match='mlp_input_gradient.*operand formats'):
            mlp.input_gradient(params, saved, sigma)
    seeing = ops.PackedMlp(dict(mlp_cfg, predict_visibility=True), DEV)
    with pytest.raises(NotImplementedError, match='predict_visibility'):
        seeing.input_gradient_workspace_floats(8)


# ------------------------------------------------------------------------------------------------------------------ 5 the C ABI alone
def test_gradient_abi_program_meets_the_oracle(tmp_path):
    """tests/native/gradient_abi_smoke.cpp, compiled against the two headers and run without PyTorch in its process, on the fixture of
    tests/test_field_gradient_host.py: forward-train, input gradient and field normals."""
    exe = compile_smoke(str(tmp_path))
    (tmp_path / 'fixture').write_bytes(native_fixture())
    r = subprocess.run([exe, str(tmp_path / 'fixture')], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and 'gradient_abi_smoke: OK' in r.stdout, r.stdout + r.stderr
    case = gref.case('w128_views')
    assert f'gradient_abi_smoke: 300 points, {int(case["compared"].sum())} compared, {int((case["sigma"] == 0).sum())} closed' in r.stdout
