"""The Warper on the device (csrc/warp.hip -> ops -> qa.forward_warp / bilinear_splatting / bilinear_interpolation) against the
fixtures the reference's Warper produced (tests/golden/warp_*.npz, tools/make_golden_warp.py) and, where there is no fixture, the
numpy restatement held to them (tests/warp_reference.py).  Both sides compute in fp64.  The gates: every mask equal on every pixel;
warped_depth2 to 1e-12 relative (1e-8 where a training view equals the test view: a coordinate that rounds across an integer moves a
~1e-13 weight to the neighbouring cell) -- the mask tests' own gates on these shapes; the flow to 1e-12 x max(1, |position|) (fp64
rounding over about twenty operations at positions below 130 with |Z| > 0.1); the uint8 colour equal on every value whose unrounded
colour is not within 1e-9 of a rounding tie, and within 1 there; the float splat of non-negative values to 1e-12 relative; the
backward warp bit for bit."""
import numpy
import pytest
import torch

from tests import mask_reference, warp_reference
from tests.warp_reference import VIEW, fixture, small_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SORTERS = ('torch', 'library')
CAMERA_KEYS = ('extrinsics_train', 'extrinsic_test', 'intrinsics_train', 'intrinsic_test')


def dev(array):
    return None if array is None else torch.as_tensor(numpy.ascontiguousarray(array)).to(DEV)


def host(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def camera_of(scene, v):
    return scene['extrinsics_train'][v], scene['extrinsic_test'], scene['intrinsics_train'][v], scene['intrinsic_test']


@pytest.mark.parametrize('sorter', SORTERS)
@pytest.mark.parametrize('shape', mask_reference.SHAPES)
@pytest.mark.parametrize('case', mask_reference.CASES)
def test_forward_warp_equals_the_reference(case, shape, sorter):
    from simplenerf_amd import qa
    want = fixture(case, shape)
    scene = mask_reference.occlusion_scene(*shape, case)
    worst = {'depth': 0.0, 'flow': 0.0, 'ties': 0}
    for v in range(3):
        out = qa.forward_warp(dev(want['frame1'][v]), dev(scene['depth_train'][v]), *camera_of(scene, v), mask1=dev(want['mask1'][v]),
                              sorter=sorter)
        assert [t.dtype for t in out] == [torch.uint8, torch.bool, torch.float64, torch.float64]
        assert [tuple(t.shape) for t in out] == [shape + (3,), shape, shape, shape + (2,)]
        colour, mask2, depth2, flow12 = host(out)
        assert numpy.array_equal(mask2, want['mask2'][v]), int((mask2 != want['mask2'][v]).sum())
        assert numpy.array_equal(depth2[~mask2], want['warped_depth2'][v][~mask2])      # zeros
        worst['depth'] = max(worst['depth'], warp_reference.relative(depth2, want['warped_depth2'][v]))
        worst['flow'] = max(worst['flow'], warp_reference.flow_deviation(flow12, want['flow12'][v]))
        wrong, inside = warp_reference.colour_difference(colour, want['warped_frame2'][v], want['colour_unrounded'][v])
        worst['ties'] += int(warp_reference.near_tie(want['colour_unrounded'][v])[want['mask2'][v]].sum())
        assert wrong == 0 and inside <= 1, (v, wrong, inside)
    print(case, shape, sorter, 'largest deviation: warped_depth2', worst['depth'], 'flow12', worst['flow'], 'values in the tie band', worst['ties'])
    assert worst['depth'] <= (1e-8 if case == 'same_pose' else 1e-12), worst
    assert worst['flow'] <= 1e-12, worst


@pytest.mark.parametrize('sorter', SORTERS)
@pytest.mark.parametrize('shape', mask_reference.SHAPES)
@pytest.mark.parametrize('case', mask_reference.CASES)
def test_float_splat_along_the_stored_flow_equals_the_reference(case, shape, sorter):
    """Four non-negative float64 channels along the reference's own flow, with a source mask and a flow mask: the positions are the
    reference's bit for bit, the sums do not cancel."""
    from simplenerf_amd import qa
    want = fixture(case, shape)
    depth = mask_reference.occlusion_scene(*shape, case)['depth_train'][VIEW]
    args = (dev(want['flow12'][VIEW]), dev(want['mask1'][VIEW]), dev(want['splat_flow_mask']))
    got = qa.bilinear_splatting(dev(want['values4']), dev(depth), *args, sorter=sorter)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.bool and tuple(got[0].shape) == shape + (4,)
    warped, mask2 = host(got)
    assert numpy.array_equal(mask2, want['splat4_mask2'])
    deviation = warp_reference.relative(warped, want['splat4'])
    print(case, shape, sorter, 'largest relative deviation of the float splat', deviation)
    assert deviation <= 1e-12
    # a float64 depth1 is the float32 one widened: the same bits; a float32 frame is widened too
    again = host(qa.bilinear_splatting(dev(want['values4']), dev(depth.astype(numpy.float64)), *args, sorter=sorter))
    assert again[0].tobytes() == warped.tobytes() and numpy.array_equal(again[1], mask2)
    single = host(qa.bilinear_splatting(dev(want['values4'].astype(numpy.float32)), dev(depth), *args, sorter=sorter))
    assert single[0].tobytes() == warped.tobytes()          # (values4 holds 16 significant bits: exact in float32)


@pytest.mark.parametrize('shape', mask_reference.SHAPES)
@pytest.mark.parametrize('case', mask_reference.CASES)
def test_backward_warp_equals_the_reference_bit_for_bit(case, shape):
    from simplenerf_amd import qa
    want = fixture(case, shape)
    image, known, depth = want['warped_frame2'][VIEW], want['mask2'][VIEW], want['warped_depth2'][VIEW][..., None]
    flow = dev(want['back_flow'])
    for name, frame, is_image in (('back_image', image, True), ('back_float', depth, False)):
        for suffix, masks in (('', (dev(known), dev(want['back_flow_mask']))), ('_plain', (None, None))):
            got = qa.bilinear_interpolation(dev(frame), flow, *masks, is_image=is_image)
            assert got[0].dtype == (torch.uint8 if is_image else torch.float64) and got[1].dtype == torch.bool
            warped, mask1 = host(got)
            assert numpy.array_equal(mask1, want[name + suffix + '_mask1']), name + suffix
            assert warped.shape == want[name + suffix].shape and warped.tobytes() == want[name + suffix].tobytes(), name + suffix


@pytest.mark.parametrize('case,shape', [(case, (37, 53)) for case in mask_reference.CASES] + [('generic', (64, 80))])
def test_forward_warp_is_the_mask_stages_of_the_same_view(case, shape):
    """warped_depth2 and mask2 of forward_warp (no mask1) are, bit for bit, the warped depth and the warping mask qa.visibility_mask's
    stages compute for the view: one projection kernel, one key rule, one walk order."""
    from simplenerf_amd import qa
    scene = mask_reference.occlusion_scene(*shape, case)
    frame = dev(fixture(case, shape)['frame1'][0])
    _, _, warped_depth, weight_sum = qa.visibility_mask(dev(scene['depth_train']), dev(scene['depth_test']),
                                                        *(scene[k] for k in CAMERA_KEYS), return_views=True)
    for v in range(3):
        for sorter in SORTERS:
            _, mask2, depth2, _ = qa.forward_warp(frame, dev(scene['depth_train'][v]), *camera_of(scene, v), sorter=sorter)
            assert torch.equal(mask2, weight_sum[v] > 0)
            assert depth2.cpu().numpy().tobytes() == warped_depth[v].cpu().numpy().tobytes()


def test_two_calls_return_the_same_bits():
    from simplenerf_amd import qa
    want = fixture('behind', (64, 80))
    scene = mask_reference.occlusion_scene(64, 80, 'behind')
    forward = lambda: host(qa.forward_warp(dev(want['frame1'][2]), dev(scene['depth_train'][2]), *camera_of(scene, 2), mask1=dev(want['mask1'][2])))
    splat = lambda: host(qa.bilinear_splatting(dev(want['values4']), dev(scene['depth_train'][VIEW]), dev(want['flow12'][VIEW]),
                                               dev(want['mask1'][VIEW]), dev(want['splat_flow_mask']), sorter='library'))
    back = lambda: host(qa.bilinear_interpolation(dev(want['values4']), dev(want['back_flow']), dev(want['mask2'][VIEW]), dev(want['back_flow_mask'])))
    for call in (forward, splat, back):
        first, second = call(), call()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


@pytest.mark.parametrize('channels', [1, 4])
def test_small_case_equals_the_restatement(channels):
    """(19, 23) without a fixture: a block of exactly integer positions (four weights of 1 on one cell), a band off every side of the
    frame, non-finite flows, masks with holes, and a depth of zeros (nothing splats).  The positions are numpy's bit for bit, so the
    masks are pinned on every pixel.  The frame holds values of both signs in (-3, 9), so the bound is absolute: a pixel sums at
    most a few dozen contributions whose weights carry the rounding of one log, one exp and three divisions scaled by 50 L / max L
    (a relative 1e-14), hence |got - want| <= 1e-12 x max |v|.  The backward warp is bit-equal."""
    from simplenerf_amd import qa
    case = small_case(channels)
    flow, mask1, flow_mask = dev(case['flow12']), dev(case['mask1']), dev(case['flow12_mask'])
    bound = 1e-12 * float(numpy.abs(case['frame']).max())
    with numpy.errstate(invalid='ignore'):
        want = warp_reference.bilinear_splatting(case['frame'], case['depth1'], case['flow12'], case['mask1'], case['flow12_mask'])
        want_plain = warp_reference.bilinear_splatting(case['frame'], case['depth1'], case['flow12'])
        want_image = warp_reference.bilinear_splatting(case['image'], case['depth1'], case['flow12'], case['mask1'], is_image=True)
        unrounded = warp_reference.bilinear_splatting(case['image'], case['depth1'], case['flow12'], case['mask1'])[0]
    for sorter in SORTERS:
        got = host(qa.bilinear_splatting(dev(case['frame']), dev(case['depth1']), flow, mask1, flow_mask, sorter=sorter))
        assert numpy.array_equal(got[1], want[1]) and 0.3 < want[1].mean() < 1.0
        print(channels, sorter, 'largest deviation', float(numpy.abs(got[0] - want[0]).max()), 'bound', bound)
        assert numpy.isfinite(got[0]).all() and numpy.abs(got[0] - want[0]).max() <= bound
        got = host(qa.bilinear_splatting(dev(case['frame']), dev(case['depth1']), flow, sorter=sorter))
        assert numpy.array_equal(got[1], want_plain[1]) and numpy.abs(got[0] - want_plain[0]).max() <= bound
        # the block of integer positions: (y, x) in 4..8 x 5..10 moved by (2, integer) -- whole weights on the cell each lands on
        ys, xs = numpy.mgrid[4:9, 5:11]
        assert got[1][ys + case['flow12'][4:9, 5:11, 1].astype(int), xs + 2].all()
        got = host(qa.bilinear_splatting(dev(case['image']), dev(case['depth1']), flow, mask1, is_image=True, sorter=sorter))
        assert got[0].dtype == numpy.uint8 and numpy.array_equal(got[1], want_image[1])
        wrong, inside = warp_reference.colour_difference(got[0], want_image[0], unrounded)
        assert wrong == 0 and inside <= 1
        # a lone source on an integer position (every other flow is NaN): four weights of 1 on ONE cell, whose value is the source's
        lone_flow = numpy.full((19, 23, 2), numpy.nan)
        lone_flow[7, 8] = (2.0, -3.0)
        lone = host(qa.bilinear_splatting(dev(case['frame']), dev(case['depth1']), dev(lone_flow), sorter=sorter))
        assert lone[1].sum() == 1 and lone[1][4, 10] and numpy.allclose(lone[0][4, 10], case['frame'][7, 8], rtol=1e-15, atol=0)
        # a depth of zeros: max L = 0, nothing splats
        nothing = host(qa.bilinear_splatting(dev(case['frame']), dev(numpy.zeros((19, 23), dtype=numpy.float32)), flow, sorter=sorter))
        assert not nothing[1].any() and not nothing[0].any()
    with numpy.errstate(invalid='ignore'):
        for frame, is_image in ((case['frame'], False), (case['frame'].astype(numpy.float32), False), (case['image'], True)):
            for masks in ((case['mask1'], case['flow12_mask']), (None, None)):
                want_back = warp_reference.bilinear_interpolation(frame, case['flow12'], *masks, is_image=is_image)
                got = host(qa.bilinear_interpolation(dev(frame), flow, *(dev(m) for m in masks), is_image=is_image))
                assert got[0].dtype == want_back[0].dtype and got[0].tobytes() == want_back[0].tobytes()
                assert numpy.array_equal(got[1], want_back[1]) and not got[1][2, 3] and 0.3 < got[1].mean() < 1.0
