"""The 16-bit view sweep without a GPU: its C ABI (a fourth header group), every refusal and the empty calls, the two queries, and the
helpers the device tests decode and round with (tests/view_sweep16_reference.py)."""
import ctypes
import os
import re

import numpy
import pytest
import torch

from simplenerf_amd import _lib, ops, synth
from tests import view_sweep16_reference as ref16

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'snerf_view_sweep_half', 'snerf_view_sweep_half_workspace_floats', 'snerf_view_sweep_half_acts_floats'}
SMALL = dict(depth=4, width=128, views_width=64)


def desc_of(**overrides):
    return ops.mlp_desc(synth.mlp_config(**overrides))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_points_are_a_fourth_header_group_declared_bound_and_exported():
    assert [os.path.relpath(path, REPO) for path in _lib.SWEEP16_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_sweep16.h')]
    header = open(_lib.SWEEP16_HEADERS[0]).read()
    declared = set(re.findall(r'^(?:size_t|int)\s+(snerf_[a-z_0-9]+)\s*\(', header, flags=re.M))
    assert declared == set(_lib.SWEEP16_SIGNATURES) == NAMES
    for group in (_lib.SIGNATURES, _lib.ADDED_SIGNATURES, _lib.SWEEP_SIGNATURES):
        assert not NAMES & set(group)
    assert len(_lib.SIGNATURES) == 81 and len(_lib.ADDED_SIGNATURES) == 2 and len(_lib.SWEEP_SIGNATURES) == 2      # the older groups did not grow
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SWEEP16_SIGNATURES[name][1], name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    restype, argtypes = _lib.SWEEP16_SIGNATURES['snerf_view_sweep_half_workspace_floats']
    assert restype is ctypes.c_size_t and argtypes[1:] == [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    restype, argtypes = _lib.SWEEP16_SIGNATURES['snerf_view_sweep_half_acts_floats']
    assert restype is ctypes.c_size_t and argtypes[1:] == [ctypes.c_longlong, ctypes.c_int]
    restype, argtypes = _lib.SWEEP16_SIGNATURES['snerf_view_sweep_half']
    pointer = ctypes.c_void_p
    assert restype is ctypes.c_int and argtypes[2:] == [ctypes.c_int, pointer, pointer, pointer, pointer, ctypes.c_longlong, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer, pointer, pointer]
    assert argtypes[0] is ctypes.POINTER(_lib.MlpDesc) and argtypes[1] is ctypes.POINTER(ctypes.c_void_p)
    # the sweep's own arguments are snerf_view_sweep's with `precision` in front of the outputs
    older = _lib.SWEEP_SIGNATURES['snerf_view_sweep'][1]
    assert argtypes[:11] == older[:11] and argtypes[12:] == older[11:]
    assert callable(ops.view_sweep_half)


def sweep(desc, num_params=None, params=True, acts=16, weights=16, acc=0, dirs=16, n=5, s=8, v=2, white=0, precision=None, out=16, work=16):
    """snerf_view_sweep_half on pointers that are never dereferenced -> (status, message)."""
    lib = _lib.load()
    count = lib.snerf_mlp_num_params(ctypes.byref(desc)) if (desc is not None and num_params is None) else (num_params or 0)
    table = (ctypes.c_void_p * max(count, 1))(*([16] * max(count, 1))) if params else None
    precision = ops.PRECISION_BF16 if precision is None else precision
    st = lib.snerf_view_sweep_half(None if desc is None else ctypes.byref(desc), table, count,
                                   *(ctypes.c_void_p(p) for p in (acts, weights, acc, dirs)), n, s, v, white, precision,
                                   ctypes.c_void_p(out), ctypes.c_void_p(work), ctypes.c_void_p(0))
    return st, lib.snerf_last_error().decode()


def test_bad_arguments_are_refused_without_a_device():
    good = desc_of()
    assert sweep(None)[0] == _lib.C.SNERF_E_INVALID and 'NULL descriptor' in sweep(None)[1]
    for kw, word in (({'params': False}, 'NULL params'), ({'acts': 0}, 'NULL pointer'), ({'weights': 0}, 'NULL pointer'),
                     ({'dirs': 0}, 'NULL pointer'), ({'out': 0}, 'NULL pointer'), ({'work': 0}, 'NULL pointer'),
                     ({'v': -1}, 'num_views'), ({'n': -1}, 'num_rays'), ({'s': 0}, 'num_samples'), ({'white': 1}, 'white_bkgd needs acc'),
                     ({'num_params': 3}, 'parameter tensors'), ({'work': 20}, 'aligned'), ({'acts': 20}, 'aligned')):
        for precision in (ops.PRECISION_F16, ops.PRECISION_BF16):
            st, message = sweep(good, precision=precision, **kw)
            assert st == _lib.C.SNERF_E_INVALID and word in message and 'view_sweep_half' in message, (kw, st, message)


@pytest.mark.parametrize('precision', [ops.PRECISION_FP32, ops.PRECISION_F16X3, ops.PRECISION_F16S8, ops.PRECISION_BF16S8, -1, 99])
def test_a_bad_precision_is_refused_by_name(precision):
    for kw in ({}, {'n': 0}, {'v': 0}):          # an empty call with a precision the call cannot read is no empty call
        st, message = sweep(desc_of(), precision=precision, **kw)
        assert st == _lib.C.SNERF_E_INVALID, (st, message)
        assert f'precision {precision}' in message and 'SNERF_PRECISION_F16' in message and 'SNERF_PRECISION_BF16' in message
        assert re.search(r'\bsnerf_view_sweep reads fp32 activations', message), message


@pytest.mark.parametrize('overrides, word', [({'views_depth': 2}, 'layered shape'), ({'width': 192}, 'layered shape'),
                                             ({'predict_visibility': True}, 'predict_visibility'),
                                             ({'sigma_pe_degree': 3}, 'sigma_pe_degree'),
                                             ({'use_view_dirs': False, 'view_dependent_rgb': False}, 'no views head'),
                                             ({'width': 256, 'views_width': 64}, '256 / 64')])
def test_unsupported_descriptors_are_refused_by_name_and_the_queries_are_zero(overrides, word):
    desc = desc_of(**overrides)
    st, message = sweep(desc)
    assert st == _lib.C.SNERF_E_UNSUPPORTED and word in message, (st, message)
    assert _lib.load().snerf_view_sweep_half_workspace_floats(ctypes.byref(desc), 77, 192, 3) == 0
    assert _lib.load().snerf_view_sweep_half_acts_floats(ctypes.byref(desc), 77, 192) == 0


def test_empty_calls_succeed_without_a_device():
    for desc in (desc_of(), desc_of(**SMALL)):
        for precision in (ops.PRECISION_F16, ops.PRECISION_BF16):
            assert sweep(desc, n=0, acts=0, weights=0, dirs=0, out=0, work=0, precision=precision)[0] == 0
            assert sweep(desc, v=0, acts=0, weights=0, dirs=0, out=0, work=0, precision=precision)[0] == 0
            assert sweep(desc, n=0, v=0, white=1, params=False, precision=precision)[0] == 0


def test_queries_grow_with_every_count_and_fit_the_saved_activations():
    lib = _lib.load()
    work, acts, saved = lib.snerf_view_sweep_half_workspace_floats, lib.snerf_view_sweep_half_acts_floats, lib.snerf_mlp_saved_floats
    for cfg in ({}, SMALL):
        desc = desc_of(**cfg)
        d = ctypes.byref(desc)
        base = work(d, 77, 50, 3)
        assert base >= 3 * 3 * 77 * 50
        for n, s, v in ((78, 50, 3), (77, 51, 3), (77, 50, 4), (4096, 192, 120)):
            assert work(d, n, s, v) >= base, (n, s, v)
        series = [work(d, n, 192, 16) for n in (0, 1, 31, 32, 33, 1000, 4096)]
        assert series == sorted(series)
        assert work(d, -1, 50, 3) == 0 and work(d, 77, 0, 3) == 0 and work(d, 77, 50, -1) == 0
        # what the call reads: nothing of an empty call, whole blocks but the last, never more than the forward allocates
        mlp_cfg = synth.mlp_config(**cfg)
        rows, width, depth = ref16.block_rows(mlp_cfg), mlp_cfg['points_net_width'], mlp_cfg['points_net_depth']
        assert acts(d, 0, 50) == 0 and acts(d, -1, 50) == 0 and acts(d, 77, 0) == 0
        for n, s in ((1, 5), (1, 32), (1, 33), (77, 50), (64, 32), (4096, 192)):
            blocks = (n * s + 31) // 32
            assert acts(d, n, s) == ((blocks - 1) * rows + 96 + depth * width + width) * 16, (n, s)
            assert acts(d, n, s) <= saved(d, n, s), (n, s)


# ------------------------------------------------------------------------------------------------ the helpers
@pytest.mark.parametrize('mode', ['f16', 'bf16'])
def test_the_decoder_inverts_the_layout_the_header_describes(mode):
    """Pieces written here by the header's sentence -- slot 2 j + h of piece k, element e = feature 16 k + 8 (e >> 2) + 4 h + (e & 3)
    of sample j -- come back as the (n,S,W) array they were made from, partial last block included."""
    mlp_cfg = synth.mlp_config(**SMALL)
    n, s, width, depth = 3, 23, 128, 4
    rows = ref16.block_rows(mlp_cfg)
    rng = numpy.random.RandomState(5)
    feature = ref16.rounded(rng.standard_normal((n * s, width)), mode)
    blocks = (n * s + 31) // 32
    halves = torch.zeros(blocks * rows * 32, dtype=ref16.FORMATS[mode])
    for i in range(n * s):
        b, j = divmod(i, 32)
        for f in range(width):
            k, r = divmod(f, 16)
            h, e = (r >> 2) & 1, (r & 3) + 4 * (r >> 3)
            halves[(b * rows + 96 + depth * width) * 32 + k * 512 + (2 * j + h) * 8 + e] = float(feature[i, f])
    saved = halves.view(torch.float32).numpy()
    back = ref16.saved_feature(saved, mlp_cfg, n, s, mode)
    assert back.shape == (n, s, width) and numpy.array_equal(back.reshape(n * s, width), feature)


@pytest.mark.parametrize('mode', ['f16', 'bf16'])
def test_settled_directions_move_little_and_only_what_is_ambiguous(mode):
    rng = numpy.random.RandomState(11)
    dirs = rng.standard_normal((37, 64, 3)).astype(numpy.float32)
    dirs /= numpy.linalg.norm(dirs, axis=-1, keepdims=True)
    settled = ref16.settled_directions(dirs, 4, mode)
    moved = settled != dirs
    # (expected share: 8 sines and cosines per component, each within 2^-20 of a midpoint on either side out of a spacing of 2^-11
    # (f16) or 2^-8 (bf16) relative: 8 x 2^-8 = 3 % at most)
    assert settled.dtype == numpy.float32 and moved.mean() < 0.05 and numpy.abs(settled - dirs).max() <= 4 * 2.0 ** -10
    assert numpy.array_equal(ref16.settled_directions(settled, 4, mode), settled)
    # settled: the float32 and the float64 encodings round to the same 16-bit values
    single = ref16.rounded(ref16.ref.encode(settled, 4), mode)
    double = ref16.rounded(ref16.ref.encode(settled.astype(numpy.float64), 4).astype(numpy.float32), mode)
    assert numpy.array_equal(single, double)
