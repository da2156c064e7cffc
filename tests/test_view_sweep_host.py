"""The view sweep without a GPU: its C ABI (a third header group), every refusal and the empty calls, the workspace query, the numpy
restatement of its formula (tests/view_sweep_reference.py) against the reference's own colours (tests/golden/view_sweep.npz,
tools/make_golden_view_sweep.py), and create_test_data's standing refusals."""
import ctypes
import os
import re

import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import _lib, harness, ops, synth
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor
from tests import util
from tests import view_sweep_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'snerf_view_sweep', 'snerf_view_sweep_workspace_floats'}
RGB_TOL = 1e-4


def desc_of(**overrides):
    return ops.mlp_desc(synth.mlp_config(**overrides))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_points_are_a_third_header_group_declared_bound_and_exported():
    assert [os.path.relpath(path, REPO) for path in _lib.SWEEP_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_sweep.h')]
    header = open(_lib.SWEEP_HEADERS[0]).read()
    declared = set(re.findall(r'\b(snerf_view_[a-z_0-9]+)\s*\(', header))
    assert declared == set(_lib.SWEEP_SIGNATURES) == NAMES
    assert not NAMES & set(_lib.SIGNATURES) and not NAMES & set(_lib.ADDED_SIGNATURES)
    assert len(_lib.SIGNATURES) == 81 and len(_lib.ADDED_SIGNATURES) == 2          # the pinned groups did not grow
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SWEEP_SIGNATURES[name][1], name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    restype, argtypes = _lib.SWEEP_SIGNATURES['snerf_view_sweep_workspace_floats']
    assert restype is ctypes.c_size_t and argtypes[1:] == [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    restype, argtypes = _lib.SWEEP_SIGNATURES['snerf_view_sweep']
    pointer = ctypes.c_void_p
    assert restype is ctypes.c_int and argtypes[2:] == [ctypes.c_int, pointer, pointer, pointer, pointer, ctypes.c_longlong, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, pointer, pointer, pointer]
    assert argtypes[0] is ctypes.POINTER(_lib.MlpDesc) and argtypes[1] is ctypes.POINTER(ctypes.c_void_p)
    assert callable(ops.view_sweep) and callable(ops.render_keep_activations)


def sweep(desc, num_params=None, params=True, acts=16, weights=16, acc=0, dirs=16, n=5, s=8, v=2, white=0, out=16, work=16):
    """snerf_view_sweep on pointers that are never dereferenced -> (status, message)."""
    lib = _lib.load()
    count = lib.snerf_mlp_num_params(ctypes.byref(desc)) if (desc is not None and num_params is None) else (num_params or 0)
    table = (ctypes.c_void_p * max(count, 1))(*([16] * max(count, 1))) if params else None
    st = lib.snerf_view_sweep(None if desc is None else ctypes.byref(desc), table, count, *(ctypes.c_void_p(p) for p in (acts, weights, acc, dirs)),
                              n, s, v, white, ctypes.c_void_p(out), ctypes.c_void_p(work), ctypes.c_void_p(0))
    return st, lib.snerf_last_error().decode()


def test_bad_arguments_are_refused_without_a_device():
    good = desc_of()
    assert sweep(None)[0] == _lib.C.SNERF_E_INVALID and 'NULL descriptor' in sweep(None)[1]
    for kw, word in (({'params': False}, 'NULL params'), ({'acts': 0}, 'NULL pointer'), ({'weights': 0}, 'NULL pointer'),
                     ({'dirs': 0}, 'NULL pointer'), ({'out': 0}, 'NULL pointer'), ({'work': 0}, 'NULL pointer'),
                     ({'v': -1}, 'num_views'), ({'n': -1}, 'num_rays'), ({'s': 0}, 'num_samples'), ({'white': 1}, 'white_bkgd needs acc'),
                     ({'num_params': 3}, 'parameter tensors'), ({'work': 20}, 'aligned')):
        st, message = sweep(good, **kw)
        assert st == _lib.C.SNERF_E_INVALID and word in message, (kw, st, message)


@pytest.mark.parametrize('overrides, word', [({'views_depth': 2}, 'layered shape'), ({'width': 192}, 'layered shape'),
                                             ({'predict_visibility': True}, 'predict_visibility'),
                                             ({'sigma_pe_degree': 3}, 'sigma_pe_degree'),
                                             ({'use_view_dirs': False, 'view_dependent_rgb': False}, 'no views head'),
                                             ({'width': 256, 'views_width': 64}, '256 / 64')])
def test_unsupported_descriptors_are_refused_by_name(overrides, word):
    desc = desc_of(**overrides)
    st, message = sweep(desc)
    assert st == _lib.C.SNERF_E_UNSUPPORTED and word in message, (st, message)
    assert _lib.load().snerf_view_sweep_workspace_floats(ctypes.byref(desc), 77, 192, 3) == 0


def test_empty_calls_succeed_without_a_device():
    for desc in (desc_of(), desc_of(depth=4, width=128, views_width=64)):
        assert sweep(desc, n=0, acts=0, weights=0, dirs=0, out=0, work=0)[0] == 0
        assert sweep(desc, v=0, acts=0, weights=0, dirs=0, out=0, work=0)[0] == 0
        assert sweep(desc, n=0, v=0, white=1, params=False)[0] == 0


def test_workspace_query_grows_with_every_count():
    query = _lib.load().snerf_view_sweep_workspace_floats
    for desc in (desc_of(), desc_of(depth=4, width=128, views_width=64)):
        d = ctypes.byref(desc)
        base = query(d, 77, 50, 3)
        assert base >= 3 * 3 * 77 * 50
        for n, s, v in ((78, 50, 3), (77, 51, 3), (77, 50, 4), (4096, 192, 120)):
            assert query(d, n, s, v) >= base, (n, s, v)
        series = [query(d, n, 192, 16) for n in (0, 1, 31, 32, 33, 1000, 4096)]
        assert series == sorted(series)
        assert query(d, -1, 50, 3) == 0 and query(d, 77, 0, 3) == 0 and query(d, 77, 50, -1) == 0


# ------------------------------------------------------------------------------------------------ the formula
@pytest.mark.parametrize('tag', ref.CASES)
def test_restatement_reproduces_the_reference_colours(tag):
    """The formula in float64, fed the feature vectors of the oracle's MLP on the fixture's rays at the reference's fine depths
    and the reference's own weights_fine, gives the reference's rgb_fine under each of the three view cameras."""
    g, configs, _, _ = ref.load_case(tag)
    params = {k: v.double() for k, v in util.golden_params(configs, g).items()}
    ndc = configs['data_loader']['ndc']
    origins, directions = (g['batch_rays_o_ndc'], g['batch_rays_d_ndc']) if ndc else (g['batch_rays_o'], g['batch_rays_d'])
    points = oracle.ray_points(torch.from_numpy(origins).double(), torch.from_numpy(directions).double(),
                               torch.from_numpy(g['out_z_vals_fine']).double())
    feature = ref.feature_vectors(params, 'fine_model.', configs['model']['fine_mlp'], points).numpy()
    assert feature.shape == (77, 192, 256)
    out = ref.view_sweep(*ref.head_arrays(params, 'fine_model.'), feature, g['out_weights_fine'], g['view_dirs'], g['out_acc_fine'],
                         configs['model']['white_bkgd'], numpy.float64)
    assert out.shape == (3, 77, 3)
    worst = util.linf(out, g['out_rgb_fine'])
    assert worst < RGB_TOL, worst
    assert util.linf(g['out_rgb_fine'][0], g['out_rgb_fine'][1]) > 50 * RGB_TOL          # the view cameras do change the colour
    # the float32 restatement stays close to the float64 one: what the device test scales its tolerance from
    single = ref.view_sweep(*ref.head_arrays(params, 'fine_model.'), feature, g['out_weights_fine'], g['view_dirs'], g['out_acc_fine'],
                            configs['model']['white_bkgd'], numpy.float32)
    assert single.dtype == numpy.float32 and util.linf(single, out) < 1e-5


# ------------------------------------------------------------------------------------------------ what stays refused
def test_create_test_data_still_refuses_other_cameras_and_names_the_new_calls():
    g, _, saved, scene_configs = ref.load_case('ndc')
    tester = DataPreprocessor(scene_configs, 'test', model_configs=saved)
    with pytest.raises(NotImplementedError, match='view_pose') as info:
        tester.create_test_data(g['pose'], view_pose=g['view_poses'][0])
    assert 'view_camera' in str(info.value)
    with pytest.raises(NotImplementedError, match='secondary_poses') as info:
        tester.create_test_data(g['pose'], secondary_poses=list(g['secondary_poses']))
    assert 'secondary_cameras' in str(info.value)
    camera = tester.camera(g['pose'], g['intrinsic'])
    assert camera['resolution'] == (7, 11) and camera['pose'].dtype == numpy.float32 and camera['intrinsic'].dtype == numpy.float32
    assert {'near', 'far', 'near_ndc', 'far_ndc'} <= set(camera)
    raw = tester.camera(camera['pose'], preprocess_pose=False)
    assert numpy.array_equal(raw['pose'], camera['pose']) and numpy.array_equal(raw['intrinsic'], numpy.float32(saved['intrinsic']))
    assert callable(harness.predict_view_sweep) and callable(harness.save_static_camera_frames)
