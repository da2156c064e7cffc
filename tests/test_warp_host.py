"""Host side of the Warper (qa.forward_warp, qa.bilinear_splatting, qa.bilinear_interpolation; csrc/warp.hip): the numpy restatement
against the fixtures the reference's Warper produced (tests/golden/warp_*.npz, tools/make_golden_warp.py), the cell and tap
arithmetic of csrc/warp_cells.h walked on the host under sanitizers, the exported symbols and the refusals -- none of it needs a GPU."""
import os
import subprocess

import numpy
import pytest
import torch

from simplenerf_amd import _lib, qa
from tests import mask_reference, warp_reference
from tests.warp_reference import GOLDEN, VIEW, fixture, small_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snerf_warp_workspace_bytes', 'snerf_warp_project', 'snerf_warp_positions_from_flow', 'snerf_warp_splat_gather',
         'snerf_warp_interpolate')


@pytest.mark.parametrize('shape', mask_reference.SHAPES)
@pytest.mark.parametrize('case', mask_reference.CASES)
def test_restatement_equals_the_reference(case, shape):
    """tests/warp_reference.py against what the reference's Warper returned: masks equal on every pixel, warped_depth2 to 1e-12
    relative in every case (both sides are numpy on the host), the flow to 1e-12 of max(1, |position|), the float splats to 1e-12 relative,
    the uint8 colour equal outside the 1e-9 tie band, the backward warp bit for bit."""
    want = fixture(case, shape)
    scene = mask_reference.occlusion_scene(*shape, case)
    h, w = shape
    assert os.path.getsize(os.path.join(GOLDEN, f'warp_{case}_{h}x{w}.npz')) < 1 << 20
    assert want['frame1'].shape == (3, h, w, 3) and want['frame1'].dtype == numpy.uint8 and want['mask1'].dtype == bool
    assert want['mask1'].all() == (case == 'same_pose') and (case == 'same_pose' or 0.05 < 1 - want['mask1'].mean() < 0.15)
    assert want['values4'].min() >= 0 and want['values4'].shape == (h, w, 4)
    for v in range(3):
        camera = (scene['extrinsics_train'][v], scene['extrinsic_test'], scene['intrinsics_train'][v], scene['intrinsic_test'])
        colour, mask2, depth2, flow12 = warp_reference.forward_warp(want['frame1'][v], scene['depth_train'][v], *camera, mask1=want['mask1'][v])
        assert colour.dtype == numpy.uint8 and mask2.dtype == bool and depth2.dtype == flow12.dtype == numpy.float64
        assert numpy.array_equal(mask2, want['mask2'][v])
        assert warp_reference.relative(depth2, want['warped_depth2'][v]) <= 1e-12
        assert warp_reference.flow_deviation(flow12, want['flow12'][v]) <= 1e-12
        wrong, inside = warp_reference.colour_difference(colour, want['warped_frame2'][v], want['colour_unrounded'][v])
        assert wrong == 0 and inside <= 1
        # the positions the flow gives are the mask restatement's
        x, y, z = mask_reference.project(scene['depth_train'][v], *camera)
        assert all(numpy.array_equal(a, b, equal_nan=True) for a, b in zip(warp_reference.positions(flow12), (x, y)))
        # what the generator asserted, on the stored data
        assert float(warp_reference.near_tie(want['colour_unrounded'][v])[want['mask2'][v]].mean()) <= 1e-3
        assert numpy.abs(z).min() > 0.1
        if case != 'same_pose':
            px, py = warp_reference.positions(want['flow12'][v])
            assert numpy.abs(px - numpy.round(px)).min() > 1e-9 and numpy.abs(py - numpy.round(py)).min() > 1e-9
    got, got_mask = warp_reference.bilinear_splatting(want['values4'], scene['depth_train'][VIEW], want['flow12'][VIEW], want['mask1'][VIEW],
                                                      want['splat_flow_mask'])
    assert numpy.array_equal(got_mask, want['splat4_mask2']) and warp_reference.relative(got, want['splat4']) <= 1e-12
    assert 0.2 < got_mask.mean() < 1.0
    image, known, depth = want['warped_frame2'][VIEW], want['mask2'][VIEW], want['warped_depth2'][VIEW][..., None]
    for name, frame, is_image in (('back_image', image, True), ('back_float', depth, False)):
        for suffix, masks in (('', (known, want['back_flow_mask'])), ('_plain', (None, None))):
            got, got_mask = warp_reference.bilinear_interpolation(frame, want['back_flow'], *masks, is_image=is_image)
            assert got.dtype == want[name + suffix].dtype and got.tobytes() == want[name + suffix].tobytes(), name + suffix
            assert numpy.array_equal(got_mask, want[name + suffix + '_mask1']), name + suffix


@pytest.mark.parametrize('shape_channels', [((24, 32), 3), ((19, 23), 4), ((9, 8), 1)])
def test_cell_and_tap_walk_on_the_host_under_sanitizers(tmp_path, shape_channels):
    """tests/native/warp_cells_test.cpp splats a frame of sources and backward-warps a frame through csrc/warp_cells.h, built with
    AddressSanitizer + UBSan: no index leaves its buffer, corner_weights hands out add_source's weights, every tap equals the
    zero-padded copy's, and the outputs equal the restatement's -- the backward warp bit for bit."""
    (h, w), c = shape_channels
    exe = str(tmp_path / 'warp_cells_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(REPO, 'tests', 'native', 'warp_cells_test.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    case = small_case(c, h, w)
    rng = numpy.random.RandomState(h * w)
    with numpy.errstate(invalid='ignore'):
        x, y = warp_reference.positions(case['flow12'])
        back_flow = case['flow12'][::-1, ::-1].copy()
        bx, by = warp_reference.positions(back_flow)
    z = rng.uniform(0.5, 9.0, (h, w))
    z[1, 1], z[3, 2] = numpy.nan, -1.5
    known = case['mask1']
    numpy.concatenate([a.reshape(-1) for a in (x, y, z, case['frame'], bx, by, case['frame'], known.astype(numpy.float64))]).tofile(tmp_path / 'in.f64')
    r = subprocess.run([exe, str(h), str(w), str(c), str(tmp_path / 'in.f64'), str(tmp_path / 'out.f64')], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 0 and 'warp_cells_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    out = numpy.fromfile(tmp_path / 'out.f64', dtype=numpy.float64)
    n = h * w
    splat, ws, back, dr = out[:n * c].reshape(h, w, c), out[n * c:n * c + n].reshape(h, w), out[n * c + n:2 * n * c + n].reshape(h, w, c), out[2 * n * c + n:]
    with numpy.errstate(invalid='ignore'):
        want, want_mask, want_ws = warp_reference.bilinear_splatting(case['frame'], z, case['flow12'], return_weights=True)
        want_back, want_mask1 = warp_reference.bilinear_interpolation(case['frame'], back_flow, known)
    assert numpy.array_equal(ws > 0, want_mask) and 0.3 < want_mask.mean() < 1.0
    assert numpy.abs(ws - want_ws).max() <= 1e-12 * want_ws.max()
    assert numpy.all(numpy.abs(splat - want) <= 1e-11 * numpy.maximum(numpy.abs(want), 1.0))      # (values of both signs: sums may cancel)
    assert back.tobytes() == want_back.tobytes() and numpy.array_equal(dr.reshape(h, w) > 0, want_mask1)


def test_library_exports_the_warp_entry_points():
    header = open(os.path.join(REPO, 'include', 'simplenerf_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    assert 'SNERF_WARP_U8 = 0, SNERF_WARP_F32 = 1, SNERF_WARP_F64 = 2' in header
    assert lib.snerf_warp_workspace_bytes(756, 1008) == 1024 * 16 == lib.snerf_visibility_mask_workspace_bytes(1, 756, 1008)
    assert lib.snerf_warp_workspace_bytes(0, 4) == 0 and lib.snerf_warp_workspace_bytes(50000, 50000) == 0      # keys beyond int32
    # refused before anything is enqueued
    assert lib.snerf_warp_interpolate(None, 0, 3, None, None, None, 1, 4, 4, None, None, None) != 0
    assert b'warp_interpolate: NULL pointer' in lib.snerf_last_error()
    assert lib.snerf_warp_splat_gather(None, None, None, None, None, 0, 3, 1, 4, 4, None, None, None) != 0
    assert b'warp_splat_gather: NULL pointer' in lib.snerf_last_error()


def test_warp_functions_refuse_what_they_cannot_take():
    class Stub(torch.Tensor):
        """A host tensor that claims to live on the GPU: reaches the checks that follow the device check."""
        is_cuda = True

    def stub(shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype).as_subclass(Stub)

    e, k = numpy.eye(4), numpy.eye(3)
    frame, depth, flow = stub((8, 9, 3), torch.uint8), stub((8, 9)), stub((8, 9, 2), torch.float64)
    # forward_warp
    with pytest.raises(RuntimeError, match='frame1: expected a tensor on the GPU'):
        qa.forward_warp(torch.zeros((8, 9, 3), dtype=torch.uint8), depth, e, e, k)
    with pytest.raises(RuntimeError, match='frame1: is_image expects a uint8 frame .*got torch.float32'):
        qa.forward_warp(stub((8, 9, 3)), depth, e, e, k)
    with pytest.raises(RuntimeError, match=r'frame1: expected shape \(h, w, 3\), got \(8, 9, 4\)'):
        qa.forward_warp(stub((8, 9, 4), torch.uint8), depth, e, e, k)
    with pytest.raises(RuntimeError, match=r'frame1: expected a non-empty shape \(h, w, c\), got \(8, 9\)'):
        qa.forward_warp(stub((8, 9), torch.uint8), depth, e, e, k)
    with pytest.raises(RuntimeError, match='depth1: expected a tensor on the GPU'):
        qa.forward_warp(frame, torch.zeros((8, 9)), e, e, k)
    with pytest.raises(RuntimeError, match='depth1: expected float32, got torch.float64'):
        qa.forward_warp(frame, stub((8, 9), torch.float64), e, e, k)
    with pytest.raises(RuntimeError, match=r'depth1: expected shape \(8, 9\), got \(9, 8\)'):
        qa.forward_warp(frame, stub((9, 8)), e, e, k)
    with pytest.raises(RuntimeError, match=r'mask1: expected shape \(8, 9\), got \(8, 8\)'):
        qa.forward_warp(frame, depth, e, e, k, mask1=stub((8, 8), torch.bool))
    with pytest.raises(RuntimeError, match='mask1: expected bool or uint8, got torch.float32'):
        qa.forward_warp(frame, depth, e, e, k, mask1=stub((8, 9)))
    with pytest.raises(RuntimeError, match=r'extrinsic1: expected shape \(4, 4\), got \(3, 3\)'):
        qa.forward_warp(frame, depth, k, e, k)
    with pytest.raises(RuntimeError, match=r'extrinsic2: expected shape \(4, 4\), got \(3, 4\)'):
        qa.forward_warp(frame, depth, e, e[:3], k)
    with pytest.raises(RuntimeError, match=r'intrinsic1: expected shape \(3, 3\), got \(4, 4\)'):
        qa.forward_warp(frame, depth, e, e, e)
    with pytest.raises(RuntimeError, match=r'intrinsic2: expected shape \(3, 3\), got \(4, 4\)'):
        qa.forward_warp(frame, depth, e, e, k, e)
    with pytest.raises(RuntimeError, match="sorter: expected 'torch' or 'library', got 'numpy'"):
        qa.forward_warp(frame, depth, e, e, k, sorter='numpy')
    # an operand on another device than the frame's (here: a stub on the meta device beside stubs on the host)
    elsewhere = torch.zeros((8, 9), dtype=torch.bool, device='meta').as_subclass(Stub)
    with pytest.raises(RuntimeError, match='mask1: expected a tensor on cpu, the device of the call.s first operand, got one on meta'):
        qa.forward_warp(frame, depth, e, e, k, mask1=elsewhere)
    with pytest.raises(RuntimeError, match='flow12_mask: expected a tensor on cpu, .*got one on meta'):
        qa.bilinear_splatting(stub((8, 9, 2)), depth, flow, flow12_mask=elsewhere)
    with pytest.raises(RuntimeError, match='mask2: expected a tensor on cpu, .*got one on meta'):
        qa.bilinear_interpolation(stub((8, 9, 3)), flow, mask2=elsewhere)
    # bilinear_splatting
    with pytest.raises(RuntimeError, match='frame1: expected a tensor on the GPU'):
        qa.bilinear_splatting(torch.zeros((8, 9, 3)), depth, flow)
    with pytest.raises(RuntimeError, match='frame1: is_image expects a uint8 frame .*got torch.float64'):
        qa.bilinear_splatting(stub((8, 9, 3), torch.float64), depth, flow, is_image=True)
    with pytest.raises(RuntimeError, match='frame1: expected float32 or float64 without is_image, got torch.uint8'):
        qa.bilinear_splatting(frame, depth, flow)
    with pytest.raises(RuntimeError, match='frame1: expected uint8 or float32 or float64, got torch.float16'):
        qa.bilinear_splatting(stub((8, 9, 3), torch.float16), depth, flow)
    for channels in (0, 5):
        with pytest.raises(RuntimeError, match=rf'frame1: expected .*\(h, w, c\).*{channels}'):
            qa.bilinear_splatting(stub((8, 9, channels)), depth, flow)
    with pytest.raises(RuntimeError, match=r'depth1: expected shape \(8, 9\), got \(8, 10\)'):
        qa.bilinear_splatting(stub((8, 9, 2)), stub((8, 10)), flow)
    with pytest.raises(RuntimeError, match='flow12: expected float64, got torch.float32'):
        qa.bilinear_splatting(stub((8, 9, 2)), depth, stub((8, 9, 2)))
    with pytest.raises(RuntimeError, match=r'flow12: expected shape \(8, 9, 2\), got \(8, 9, 3\)'):
        qa.bilinear_splatting(stub((8, 9, 2)), depth, stub((8, 9, 3), torch.float64))
    with pytest.raises(RuntimeError, match='flow12: expected a tensor on the GPU'):
        qa.bilinear_splatting(stub((8, 9, 2)), depth, torch.zeros((8, 9, 2), dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r'flow12_mask: expected shape \(8, 9\), got \(9, 9\)'):
        qa.bilinear_splatting(stub((8, 9, 2)), depth, flow, flow12_mask=stub((9, 9), torch.bool))
    with pytest.raises(RuntimeError, match="sorter: expected 'torch' or 'library'"):
        qa.bilinear_splatting(stub((8, 9, 2)), depth, flow, sorter=None)
    # bilinear_interpolation
    with pytest.raises(RuntimeError, match='frame2: expected a tensor on the GPU'):
        qa.bilinear_interpolation(numpy.zeros((8, 9, 3)), flow)
    with pytest.raises(RuntimeError, match='frame2: is_image expects a uint8 frame .*got torch.float32'):
        qa.bilinear_interpolation(stub((8, 9, 3)), flow, is_image=True)
    with pytest.raises(RuntimeError, match=r'frame2: expected 1\.\.4 channels \(h, w, c\), got 6'):
        qa.bilinear_interpolation(stub((8, 9, 6)), flow)
    with pytest.raises(RuntimeError, match=r'flow12: expected shape \(8, 9, 2\), got \(9, 8, 2\)'):
        qa.bilinear_interpolation(stub((8, 9, 3)), stub((9, 8, 2), torch.float64))
    with pytest.raises(RuntimeError, match=r'mask2: expected shape \(8, 9\), got \(8, 9, 1\)'):
        qa.bilinear_interpolation(stub((8, 9, 3)), flow, mask2=stub((8, 9, 1), torch.bool))
    with pytest.raises(RuntimeError, match='flow12_mask: expected a tensor on the GPU'):
        qa.bilinear_interpolation(stub((8, 9, 3)), flow, flow12_mask=torch.ones((8, 9), dtype=torch.bool))
