"""ctypes binding of the C-ABI shared library (include/simplenerf_hip.h, include/simplenerf_train.h).

The HIP library is the only implementation of the path: if it is missing or a call fails, a RuntimeError is raised --
there is no PyTorch or CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import types

from . import _cdecl
from .build import INCLUDE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libsimplenerf_hip.so')

# The headers are the binding's only source (the two under include/, then ADDED_HEADERS, SWEEP_HEADERS, SWEEP16_HEADERS, PNG_HEADERS, JPEG_HEADERS, FUSE_HEADERS, MESH_HEADERS, FIELD_HEADERS, GRADIENT_HEADERS and NORMALS_HEADERS below): every prototype, struct layout, #define and enumerator below is read from them
# (_cdecl.py), in inclusion order.  snerf_iteration records live in pinned host and device memory and are passed by address.
HEADERS = ('simplenerf_hip.h', 'simplenerf_train.h')
_decls = _cdecl.Header(by_address=('snerf_iteration',))
for _name in HEADERS:
    with open(os.path.join(INCLUDE, _name)) as _f:
        _decls.read(_f.read(), _name)

C = types.SimpleNamespace(**_decls.constants)      # C.SNERF_PRECISION_BF16, C.SNERF_E_RANGE, ...
STRUCTS = _decls.structs                           # typedef name -> ctypes.Structure class
SIGNATURES = dict(_decls.functions)                # name -> (restype, argtypes): the prototypes of the two headers under include/
# Entry points declared beside those headers (their prototypes are a pinned set): read by the same reader, after them, and bound
# by load() like the rest.
ADDED_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_maps.h'),)
for _name in ADDED_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
ADDED_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in SIGNATURES}
# The view sweep (csrc/simplenerf_sweep.h): a third group, since the "added" group is pinned as well -- read after it, bound with it.
SWEEP_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_sweep.h'),)
for _name in SWEEP_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
SWEEP_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in SIGNATURES and _name not in ADDED_SIGNATURES}
# The view sweep from 16-bit activations (csrc/simplenerf_sweep16.h): a fourth group, since the sweep's group is pinned too.
SWEEP16_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_sweep16.h'),)
for _name in SWEEP16_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
SWEEP16_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items()
                      if _name not in SIGNATURES and _name not in ADDED_SIGNATURES and _name not in SWEEP_SIGNATURES}
# The PNG frame encoder (csrc/simplenerf_png.h): a fifth group, read after the others and bound with them.
PNG_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_png.h'),)
_earlier = set(_decls.functions)
for _name in PNG_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
PNG_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
# The JPEG frame encoder (csrc/simplenerf_jpeg.h): a sixth group, read after the others and bound with them.
JPEG_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_jpeg.h'),)
_earlier = set(_decls.functions)
for _name in JPEG_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
JPEG_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
# The point-cloud export (csrc/simplenerf_fuse.h): a seventh group, read after the others and bound with them.
FUSE_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_fuse.h'),)
_earlier = set(_decls.functions)
for _name in FUSE_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
FUSE_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
# The mesh export (csrc/simplenerf_mesh.h): an eighth group, read after the others and bound with them.
MESH_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_mesh.h'),)
_earlier = set(_decls.functions)
for _name in MESH_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
MESH_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
# The field export (csrc/simplenerf_field.h): a ninth group, read after the others and bound with them.
FIELD_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_field.h'),)
_earlier = set(_decls.functions)
for _name in FIELD_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
FIELD_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
# The field's gradient and the normals it gives (csrc/simplenerf_gradient.h): a tenth group, read after the others and bound with them.
GRADIENT_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_gradient.h'),)
_earlier = set(_decls.functions)
for _name in GRADIENT_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
GRADIENT_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
# The normal maps (csrc/simplenerf_normals.h): an eleventh group, read after the others and bound with them.
NORMALS_HEADERS = (os.path.join(_HERE, 'csrc', 'simplenerf_normals.h'),)
_earlier = set(_decls.functions)
for _name in NORMALS_HEADERS:
    with open(_name) as _f:
        _decls.read(_f.read(), os.path.basename(_name))
NORMALS_SIGNATURES = {_name: _sig for _name, _sig in _decls.functions.items() if _name not in _earlier}
C = types.SimpleNamespace(**_decls.constants)      # (again: with the #defines of the headers read after the first two)
ABI_VERSION = C.SNERF_ABI_VERSION
RENDER_LEVELS, CAMERA_FLOATS = C.SNERF_RENDER_LEVELS, C.SNERF_CAMERA_FLOATS
LOSS_MAX_TERMS, LOSS_MAX_GROUPS = C.SNERF_LOSS_MAX_TERMS, C.SNERF_LOSS_MAX_GROUPS
(MlpDesc, LossTerm, Batch, RenderConfig, RenderMlp, RenderRays, RenderLevelOut, RenderOutputs, RenderSlot, RenderLayout,
 RenderLevelGrads) = (STRUCTS['snerf_' + _name] for _name in (
    'mlp_desc', 'loss_term', 'batch', 'render_config', 'render_mlp', 'render_rays', 'render_level_out', 'render_outputs',
    'render_slot', 'render_layout', 'render_level_grads'))
LEVEL_OUT_FIELDS = tuple(_name for _name, _ in RenderLevelOut._fields_)
ITERATION_WORDS = ctypes.sizeof(STRUCTS['snerf_iteration']) // 8      # struct snerf_iteration as 64-bit words

_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: the HIP renderer has not been built. Run `python -m simplenerf_amd.build` '
            f'(needs hipcc; cross-compiles for gfx950 without a GPU). There is no fallback implementation.')
    # The process must hold ONE HIP runtime.  PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as
    # /opt/rocm's); importing torch first makes the dynamic linker bind this library to that already-loaded copy, so
    # device pointers, streams and the primary context are shared with torch's allocator.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**SIGNATURES, **ADDED_SIGNATURES, **SWEEP_SIGNATURES, **SWEEP16_SIGNATURES,
                                      **PNG_SIGNATURES, **JPEG_SIGNATURES, **FUSE_SIGNATURES, **MESH_SIGNATURES, **FIELD_SIGNATURES,
                                      **GRADIENT_SIGNATURES, **NORMALS_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.snerf_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f'{LIB_PATH}: ABI version {got}, binding expects {ABI_VERSION}; rebuild the library')
    _lib = lib
    return lib


class Fp16RangeError(RuntimeError):
    """SNERF_E_RANGE: an earlier fp16-mode launch on this device met an activation, encoded input or weight outside the fp16
    range (|v| > 65504); its outputs are invalid.  Reported once, by the next fp16-mode call (include/simplenerf_hip.h)."""


def check(status: int, what: str) -> None:
    if status == C.SNERF_E_RANGE:
        msg = load().snerf_last_error()
        raise Fp16RangeError(msg.decode() if msg else f'{what}: fp16 range exceeded')
    if status != 0:
        msg = load().snerf_last_error()
        raise RuntimeError(f'{what} failed ({status}): {msg.decode() if msg else "unknown error"}')
