"""Host side of the visibility masks (qa.visibility_mask, csrc/visibility_mask.hip): the numpy restatement against the fixtures the
reference produced, the index arithmetic of csrc/splat_cells.h walked on the host under sanitizers, the exported symbols and the
refusals -- none of it needs a GPU."""
import os
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import _lib, qa
from tests import mask_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
NAMES = ('snerf_visibility_mask_workspace_bytes', 'snerf_visibility_mask_project', 'snerf_visibility_mask_list_starts',
         'snerf_visibility_mask_gather', 'snerf_visibility_mask_combine')


def fixture(case, shape):
    with numpy.load(os.path.join(GOLDEN, f'visibility_mask_{case}_{shape[0]}x{shape[1]}.npz')) as data:
        return {k: data[k] for k in data.files}


@pytest.mark.parametrize('shape', mask_reference.SHAPES)
@pytest.mark.parametrize('case', mask_reference.CASES)
def test_restatement_equals_the_reference(case, shape):
    """tests/mask_reference.py against what the reference's MaskComputer / Warper returned for the case: warping_mask equal on every
    pixel, warped_depth to 1e-12 relative (1e-8 for same_pose), every mask equal outside the fragile pixels."""
    want = fixture(case, shape)
    assert want['depth_train'].dtype == numpy.float32 and want['depth_train'].shape == (3,) + tuple(shape)
    assert want['warped_depth'].dtype == numpy.float64 and want['mask'].shape == tuple(shape)
    scene = mask_reference.occlusion_scene(*shape, case)               # the fixture's inputs are the build-owned scene
    for key, value in scene.items():
        assert numpy.array_equal(want[key], value), key
    got = mask_reference.visibility_mask(want['depth_train'], want['depth_test'], want['extrinsics_train'], want['extrinsic_test'],
                                         want['intrinsics_train'], want['intrinsic_test'], float(want['depth_error_threshold']))
    figures = mask_reference.compare(got, want, want['depth_test'], want['thresholds'], 1e-8 if case == 'same_pose' else 1e-12)
    print(case, shape, figures)
    assert figures['fragile'] <= 0.005 * want['warping_mask'].size
    assert numpy.array_equal(want['mask'], want['mask_views'].sum(0) > 1)
    if case == 'generic':           # the case must exercise both outcomes, and holes
        assert 0.05 < 1 - want['mask'].mean() < 0.5 and 0.05 < 1 - want['warping_mask'].mean() < 0.5
    # the same intrinsic passed as "missing": the training view's own
    again = mask_reference.visibility_mask(want['depth_train'], want['depth_test'], want['extrinsics_train'], want['extrinsic_test'],
                                           want['intrinsics_train'], None, float(want['depth_error_threshold']))
    assert all(numpy.array_equal(again[k], got[k]) for k in got)


def test_restatement_min_views_and_unpinned_sources():
    scene = mask_reference.occlusion_scene(24, 32, 'generic')
    args = (scene['depth_train'], scene['depth_test'], scene['extrinsics_train'], scene['extrinsic_test'], scene['intrinsics_train'])
    views = mask_reference.visibility_mask(*args)['mask_views']
    assert numpy.array_equal(mask_reference.visibility_mask(*args, min_views=3)['mask'], views.all(0))
    assert numpy.array_equal(mask_reference.visibility_mask(*args, min_views=1)['mask'], views.any(0))
    # a view of zero depth: every Z is 0, max L = 0 -- nothing lands; a NaN depth: that source alone is dropped
    depth = scene['depth_train'].copy()
    depth[0] = 0.0
    depth[1, 5, 7] = numpy.nan
    out = mask_reference.visibility_mask(depth, *args[1:])
    assert not out['warping_mask'][0].any() and numpy.all(out['weight_sum'][0] == 0)
    assert numpy.isfinite(out['warped_depth']).all() and out['warping_mask'][1].mean() > 0.5


def special_sources(h, w):
    """(X, Y, Z, expected key) of sources placed by hand; key = fy (w + 1) + fx, or the discard key (h + 1)(w + 1)."""
    discard = (h + 1) * (w + 1)
    key = lambda fy, fx: fy * (w + 1) + fx
    return [
        (5.0, 7.0, 2.0, key(7, 5)),                     # exactly on an integer: floor == ceil, four weights of 1 on one cell
        (1.0, 1.0, 2.0, key(1, 1)),
        (float(w), float(h), 2.0, key(h, w)),           # the last interior cell, on the integer
        (0.25, 3.5, 2.0, key(3, 0)),                    # X in (0, 1): floor on the cropped border, ceil interior
        (w + 0.5, 3.5, 2.0, key(3, w)),                 # X in (w, w + 1): floor interior, ceil on the border
        (3.5, 0.75, 2.0, key(0, 3)),
        (3.5, h + 0.25, 2.0, key(h, 3)),
        (-0.5, 3.5, 2.0, discard),                      # X < 0: both cells clip onto the border
        (-7.0, 3.5, 2.0, discard),
        (w + 1.5, 3.5, 2.0, discard),                   # X > w + 1
        (w + 1.0, 3.5, 2.0, discard),                   # floor = w + 1: the border column
        (3.5, -2.25, 2.0, discard),
        (3.5, h + 9.0, 2.0, discard),
        (float('nan'), 3.5, 2.0, discard),              # unpinned: contribute nothing
        (3.5, float('inf'), 2.0, discard),
        (-float('inf'), 3.5, 2.0, discard),
        (1e300, 3.5, 2.0, discard),
        (3.5, -3e9, 2.0, discard),
        (3.5, 3.5, float('nan'), discard),
        (4.5, 3.5, -1.5, key(3, 4)),                    # behind the camera: splats, with the largest weight
    ]


@pytest.mark.parametrize('shape', [(24, 32), (37, 53), (64, 80), (9, 8)])
def test_cell_walk_on_the_host_under_sanitizers(tmp_path, shape):
    """tests/native/splat_cells_test.cpp keys, indexes and gathers a frame of sources through csrc/splat_cells.h, built with
    AddressSanitizer + UBSan: no index leaves its buffer, the keys of hand-placed sources (an integer position, each border band,
    the discard key) are the expected ones, no discarded source reaches a pixel, and the gathered sums equal both the program's own
    scatter and the restatement's."""
    exe = str(tmp_path / 'splat_cells_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(REPO, 'tests', 'native', 'splat_cells_test.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h, w = shape
    rng = numpy.random.default_rng(h * 1000 + w)
    # a warped frame: positions around the pixel grid, shifted and minified so that lists hold 0, 1 or several sources and some
    # sources fall off every side
    ys, xs = numpy.mgrid[0:h, 0:w].astype(numpy.float64)
    x = 0.8 * xs + 2.5 + rng.normal(0, 1.5, (h, w))
    y = 1.1 * ys - 3.0 + rng.normal(0, 1.5, (h, w))
    z = rng.uniform(0.5, 9.0, (h, w))
    whole = rng.random((h, w)) < 0.2                    # a fifth on integer positions
    x[whole], y[whole] = numpy.round(x[whole]), numpy.round(y[whole])
    special = special_sources(h, w)
    for i, (sx, sy, sz, _) in enumerate(special):
        x.flat[i], y.flat[i], z.flat[i] = sx, sy, sz
    numpy.stack([x, y, z]).tofile(tmp_path / 'in.f64')
    r = subprocess.run([exe, str(h), str(w), str(tmp_path / 'in.f64'), str(tmp_path / 'out.f64')], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 0 and 'splat_cells_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    keys = numpy.array([line for line in r.stdout.splitlines() if line.startswith('keys:')][0][5:].split(), dtype=numpy.int64)
    assert keys.shape == (h * w,)
    assert keys[:len(special)].tolist() == [s[3] for s in special]
    with numpy.errstate(invalid='ignore'):
        fx, fy = numpy.floor(x).reshape(-1), numpy.floor(y).reshape(-1)
        keyed = numpy.isfinite(x + y + z).reshape(-1) & (fx >= 0) & (fx <= w) & (fy >= 0) & (fy <= h)
    want_keys = numpy.where(keyed, numpy.where(keyed, fy, 0) * (w + 1) + numpy.where(keyed, fx, 0), (h + 1) * (w + 1))
    assert numpy.array_equal(keys, want_keys.astype(numpy.int64))
    assert 0.02 < (keys == (h + 1) * (w + 1)).mean() < 0.6      # the discard list is used, and is not everything
    got_zw, got_ws = numpy.fromfile(tmp_path / 'out.f64', dtype=numpy.float64).reshape(2, h, w)
    want_zw, want_ws = mask_reference.splat(x, y, z)
    assert numpy.array_equal(got_ws > 0, want_ws > 0) and 0.2 < (want_ws > 0).mean() < 1.0
    assert numpy.abs(got_ws - want_ws).max() <= 1e-12 * want_ws.max()
    assert numpy.all(numpy.abs(got_zw - want_zw) <= 1e-11 * numpy.maximum(want_ws, 1e-300))


def test_library_exports_the_mask_entry_points():
    header = open(os.path.join(REPO, 'include', 'simplenerf_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    assert lib.snerf_visibility_mask_workspace_bytes(3, 756, 1008) == 3 * 1024 * 16
    assert lib.snerf_visibility_mask_workspace_bytes(0, 4, 4) == 0 and lib.snerf_visibility_mask_workspace_bytes(3, 0, 4) == 0
    assert lib.snerf_visibility_mask_workspace_bytes(3, 30000, 30000) == 0          # keys beyond int32
    # refused before anything is enqueued (NULL pointers)
    assert lib.snerf_visibility_mask_combine(None, 3, 4, 4, 2, None, None) != 0
    assert b'visibility_mask_combine: NULL pointer' in lib.snerf_last_error()


def test_visibility_mask_refuses_what_it_cannot_take():
    class Stub(torch.Tensor):
        """A host tensor that claims to live on the GPU: reaches the checks that follow the device check."""
        is_cuda = True

    def stub(shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype).as_subclass(Stub)

    e3, e1, k3, k1 = numpy.tile(numpy.eye(4), (3, 1, 1)), numpy.eye(4), numpy.tile(numpy.eye(3), (3, 1, 1)), numpy.eye(3)
    with pytest.raises(RuntimeError, match='depth_train: expected a tensor on the GPU'):
        qa.visibility_mask(torch.zeros((3, 8, 8)), torch.zeros((8, 8)), e3, e1, k3)
    with pytest.raises(RuntimeError, match='depth_train: expected a tensor on the GPU'):
        qa.visibility_mask(numpy.zeros((3, 8, 8), dtype=numpy.float32), stub((8, 8)), e3, e1, k3)
    with pytest.raises(RuntimeError, match='depth_train: expected float32, got torch.float64'):
        qa.visibility_mask(stub((3, 8, 8), torch.float64), stub((8, 8)), e3, e1, k3)
    with pytest.raises(RuntimeError, match=r'depth_train: expected a non-empty shape \(views, h, w\), got \(8, 8\)'):
        qa.visibility_mask(stub((8, 8)), stub((8, 8)), e3, e1, k3)
    with pytest.raises(RuntimeError, match='depth_test: expected float32, got torch.float16'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8), torch.float16), e3, e1, k3)
    with pytest.raises(RuntimeError, match=r'depth_test: expected shape \(8, 8\), got \(8, 9\)'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 9)), e3, e1, k3)
    with pytest.raises(RuntimeError, match='depth_test: expected a tensor on the GPU'):
        qa.visibility_mask(stub((3, 8, 8)), torch.zeros((8, 8)), e3, e1, k3)
    for bad in (0, 4, -1, 1.5, True):
        with pytest.raises(RuntimeError, match=r'min_views: expected 1\.\.3 \(the number of training views\)'):
            qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3, e1, k3, min_views=bad)
    with pytest.raises(RuntimeError, match='depth_error_threshold: expected a non-negative number'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3, e1, k3, depth_error_threshold=float('nan'))
    with pytest.raises(RuntimeError, match=r'extrinsics_train: expected shape \(3, 4, 4\), got \(2, 4, 4\)'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3[:2], e1, k3)
    with pytest.raises(RuntimeError, match=r'extrinsic_test: expected shape \(4, 4\), got \(3, 4\)'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3, e1[:3], k3)
    with pytest.raises(RuntimeError, match=r'intrinsics_train: expected shape \(3, 3, 3\), got \(3, 3\)'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3, e1, k1)
    with pytest.raises(RuntimeError, match=r'intrinsic_test: expected shape \(3, 3\), got \(4, 4\)'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3, e1, k3, e1)
    with pytest.raises(RuntimeError, match='intrinsics_train: expected a floating-point matrix, got int64'):
        qa.visibility_mask(stub((3, 8, 8)), stub((8, 8)), e3, e1, k3.astype(numpy.int64))
    # the host-side table: inverse intrinsic | rows 0..2 of E_test inv(E_train) | test (or the view's own) intrinsic
    scene = mask_reference.occlusion_scene(24, 32, 'generic')
    table = qa.visibility_cameras(scene['extrinsics_train'], torch.from_numpy(scene['extrinsic_test']), scene['intrinsics_train'])
    assert table.shape == (3, 30) and table.dtype == numpy.float64
    assert numpy.array_equal(table[1, 21:], scene['intrinsics_train'][1].reshape(-1))
    assert numpy.allclose(table[1, :9].reshape(3, 3) @ scene['intrinsics_train'][1], numpy.eye(3), atol=1e-13)
    assert numpy.allclose(table[2, 9:21].reshape(3, 4) @ scene['extrinsics_train'][2], scene['extrinsic_test'][:3], atol=1e-13)
