"""Tensor-level wrappers over the C ABI.  PyTorch supplies device memory and the current HIP stream; every
computation happens in the HIP library.  Inputs must be CUDA(HIP) float32 tensors; outputs are allocated here."""
from __future__ import annotations

import ctypes
import functools
import math
from typing import Dict, List, Optional

import numpy
import torch

from . import _lib
from ._lib import MlpDesc

Tensor = torch.Tensor
C = _lib.C           # the headers' #defines and enumerators
# enum snerf_precision (include/simplenerf_hip.h says what each mode computes in and keeps)
PRECISION_FP32 = C.SNERF_PRECISION_FP32      # fp32 MFMA
PRECISION_F16X3 = C.SNERF_PRECISION_F16X3    # fp16 hi/lo split, 3 MFMAs per product, fp32 accumulate: fp32-grade results
PRECISION_F16 = C.SNERF_PRECISION_F16        # 16-bit mode: one fp16 MFMA per product, fp32 accumulate / master weights
PRECISION_BF16 = C.SNERF_PRECISION_BF16      # the 16-bit mode on bf16 operands (BASELINE config 5's literal dtype): no range limit
PRECISION_F16S8 = C.SNERF_PRECISION_F16S8    # 'f16' with the saved trunk activations as fp8 e4m3: only the weight gradients differ
PRECISION_BF16S8 = C.SNERF_PRECISION_BF16S8  # 'bf16' with the saved trunk activations as fp8 e4m3: only the weight gradients differ
PRECISIONS = {'fp32': PRECISION_FP32, 'f16x3': PRECISION_F16X3, 'f16': PRECISION_F16, 'bf16': PRECISION_BF16, 'f16s8': PRECISION_F16S8,
              'bf16s8': PRECISION_BF16S8}
FP16_RANGE_PRECISIONS = (PRECISION_F16X3, PRECISION_F16, PRECISION_F16S8)     # the modes whose operands must stay below 65504 (Fp16RangeError)


def _stream() -> ctypes.c_void_p:
    # raw hipStream_t of torch's current stream on the current device (the C-level getter: ~30x cheaper than building a
    # torch.cuda.Stream object, and this runs ~50 times per training iteration)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _dev(t: Optional[Tensor], name: str, shape=None) -> Optional[Tensor]:
    """Validate a device operand; returns a contiguous fp32 view (copying only if the caller's tensor is strided)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'{name}: expected a tensor on the GPU (the HIP renderer has no CPU path), got '
                           f'{type(t).__name__}{"" if not isinstance(t, torch.Tensor) else " on " + str(t.device)}')
    if t.dtype != torch.float32:
        raise RuntimeError(f'{name}: expected float32, got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    # (the common case -- a contiguous tensor outside autograd -- passes through without creating two tensor objects;
    # this function runs ~100 times per training forward)
    if t.requires_grad or not t.is_contiguous():
        return t.detach().contiguous()
    return t


def _ptr(t: Optional[Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _enqueue(name: str, dev, *args) -> None:
    """Call the entry point ``name`` with ``args`` and torch's current stream of ``dev`` as its last argument; a failure is
    reported under ``name``.  (The per-step callers -- ray generation, the render op, the MLP, the loss table, Adam, the draws, batch
    assembly -- make the same three steps inline: they run ~50 times per training iteration.)"""
    with torch.cuda.device(dev):
        st = getattr(_lib.load(), name)(*args, _stream())
    _lib.check(st, name)


# device scratch of the library calls, one buffer per (kind, device), grown on demand; a kind's calls on one device are ordered by
# the stream they are enqueued on, and every call writes its scratch before it reads it (but 'loss', which needs zeros at first)
_workspaces: Dict[tuple, Tensor] = {}


def _workspace(kind, dev: torch.device, need: int, zeroed: bool = False) -> Tensor:
    ws = _workspaces.get((kind, dev))
    if ws is None or ws.numel() < need:
        ws = _workspaces[(kind, dev)] = (torch.zeros if zeroed else torch.empty)((need,), dtype=torch.uint8, device=dev)
    return ws


# ---------------------------------------------------------------------------------------------- fp16 range flag
Fp16RangeError = _lib.Fp16RangeError
RANGE_ACTIVATION, RANGE_WEIGHT = 1, 2


def range_status(clear: bool = False) -> int:
    """The current device's fp16 range flag (snerf_range_status): 0 = clean, bit 0 = an activation / encoded input of an
    fp16-mode launch left the fp16 range, bit 1 = a weight did.  Launches are asynchronous: synchronise first to be sure
    every enqueued launch has reported.  (Without a query the flag surfaces as Fp16RangeError from the next fp16-mode call.)"""
    status = _lib.load().snerf_range_status(int(bool(clear)))
    if status < 0:
        _lib.check(status, 'snerf_range_status')
    return status


# ---------------------------------------------------------------------------------------------- measurement hook
PROFILE_MLP_FORWARD, PROFILE_MLP_BACKWARD = C.SNERF_PROFILE_MLP_FORWARD, C.SNERF_PROFILE_MLP_BACKWARD


def profile_enable(capacity: int) -> None:
    """Start (capacity > 0) or stop (0) the library's event timing of its MLP forward launches / backward calls
    (snerf_profile_enable): the events are recorded by the library on the stream each launch is enqueued on, also for
    launches issued from inside the one-call render ops."""
    _lib.check(_lib.load().snerf_profile_enable(int(capacity)), 'snerf_profile_enable')


def profile_reset() -> None:
    _lib.check(_lib.load().snerf_profile_reset(), 'snerf_profile_reset')


def profile_dropped() -> int:
    """Launches since the last enable / reset that found the event table full and were therefore not timed."""
    return int(_lib.load().snerf_profile_dropped())


def profile_collect(kind: int, capacity: int = 65536):
    """-> (milliseconds, samples): per recorded launch of ``kind`` its duration and its number of (ray, sample) rows.
    Waits for the events."""
    ms = (ctypes.c_float * capacity)()
    samples = (ctypes.c_longlong * capacity)()
    count = _lib.load().snerf_profile_collect(int(kind), ms, samples, capacity)
    if count < 0:
        _lib.check(count, 'snerf_profile_collect')
    return list(ms[:count]), list(samples[:count])


# ---------------------------------------------------------------------------------------------- K1
def generate_rays(resolution, intrinsic, pose, near: float, ndc: bool, device, first_ray: int = 0,
                  num_rays: Optional[int] = None, pixel_offset: float = 0.0) -> Dict[str, Tensor]:
    """rays_o, rays_d, view_dirs (+ rays_o_ndc, rays_d_ndc) for pixels [first_ray, first_ray+num_rays) of a frame.
    intrinsic (3,3) and pose (4,4, processed camera-to-world) are host arrays."""
    h, w = int(resolution[0]), int(resolution[1])
    if num_rays is None:
        num_rays = h * w - first_ray
    k = numpy.ascontiguousarray(numpy.asarray(intrinsic, dtype=numpy.float32).reshape(3, 3))
    p = numpy.ascontiguousarray(numpy.asarray(pose, dtype=numpy.float32).reshape(4, 4))
    out = {name: torch.empty((num_rays, 3), dtype=torch.float32, device=device)
           for name in (('rays_o', 'rays_d', 'view_dirs') + (('rays_o_ndc', 'rays_d_ndc') if ndc else ()))}
    if num_rays == 0:
        return out
    lib = _lib.load()
    with torch.cuda.device(out['rays_o'].device):      # (inline, not _enqueue: once per step of a sharded render)
        st = lib.snerf_generate_rays(h, w, k.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                     p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(pixel_offset), int(ndc),
                                     float(near), int(first_ray), int(num_rays), _ptr(out['rays_o']), _ptr(out['rays_d']),
                                     _ptr(out['view_dirs']), _ptr(out.get('rays_o_ndc')), _ptr(out.get('rays_d_ndc')),
                                     _stream())
    _lib.check(st, 'snerf_generate_rays')
    return out


# ---------------------------------------------------------------------------------------------- K2
def coarse_depths(near: Tensor, far: Tensor, num_samples: int, lindisp: bool = False,
                  t_rand: Optional[Tensor] = None) -> Tensor:
    n = near.shape[0]
    near = _dev(near.reshape(-1), 'near', (n,))
    far = _dev(far.reshape(-1), 'far', (n,))
    t_rand = _dev(t_rand, 't_rand', (n, num_samples))
    out = torch.empty((n, num_samples), dtype=torch.float32, device=near.device)
    if n == 0:
        return out
    _enqueue('snerf_coarse_depths', near.device, _ptr(near), _ptr(far), n, int(num_samples), int(bool(lindisp)), _ptr(t_rand),
             _ptr(out))
    return out


# ---------------------------------------------------------------------------------------------- K3
def mlp_desc(mlp_cfg: dict) -> MlpDesc:
    """snerf_mlp_desc from a reference-style per-MLP config dict (keys of src/models/SimpleNeRF01.py:567-584)."""
    return MlpDesc(
        points_net_depth=int(mlp_cfg['points_net_depth']), points_net_width=int(mlp_cfg['points_net_width']),
        views_net_depth=int(mlp_cfg.get('views_net_depth', 1)), views_net_width=int(mlp_cfg.get('views_net_width', 0)),
        points_pe_degree=int(mlp_cfg['points_positional_encoding_degree']),
        views_pe_degree=int(mlp_cfg.get('views_positional_encoding_degree', 0)),
        sigma_pe_degree=int(mlp_cfg.get('points_sigma_positional_encoding_degree', -1)),
        use_view_dirs=int(bool(mlp_cfg['use_view_dirs'])), view_dependent_rgb=int(bool(mlp_cfg['view_dependent_rgb'])),
        predict_visibility=int(bool(mlp_cfg.get('predict_visibility', False))))


class PackedMlp:
    """Device-resident packed weight stream of one MLP (see csrc/mlp_layout.h)."""


    def __init__(self, mlp_cfg: dict, device):
        lib = _lib.load()
        self.desc = mlp_desc(mlp_cfg)
        self.num_params = lib.snerf_mlp_num_params(ctypes.byref(self.desc))
        floats = lib.snerf_mlp_packed_floats(ctypes.byref(self.desc))
        if self.num_params == 0 or floats == 0:
            msg = lib.snerf_last_error()
            raise NotImplementedError(f'MLP configuration not built for the HIP path: {msg.decode() if msg else mlp_cfg}')
        self.buffer = torch.zeros(floats, dtype=torch.float32, device=device)
        self.use_view_dirs = bool(self.desc.view_dependent_rgb)

    def pack(self, params: List[Tensor], precision: Optional[int] = None, training: bool = False) -> None:
        """params in C-ABI order: pts_linears.{i}.weight/.bias ..., pts_output_linear.*, [feature_linear.*,
        views_linears.0.*, views_output_linear.*].  ``precision`` None: every operand format (snerf_mlp_pack); a PRECISION_*
        value: only what calls at that precision in that mode read (snerf_mlp_pack_for) -- re-pack before using the stream
        at another precision or mode."""
        lib = _lib.load()
        if len(params) != self.num_params:
            raise RuntimeError(f'expected {self.num_params} parameter tensors, got {len(params)}')
        held = [_dev(p, f'param[{i}]') for i, p in enumerate(params)]
        arr = (ctypes.c_void_p * len(held))(*[p.data_ptr() for p in held])
        with torch.cuda.device(self.buffer.device):
            if precision is None:
                what = 'snerf_mlp_pack'
                st = lib.snerf_mlp_pack(ctypes.byref(self.desc), arr, len(held), _ptr(self.buffer), _stream())
            else:
                what = 'snerf_mlp_pack_for'
                st = lib.snerf_mlp_pack_for(ctypes.byref(self.desc), arr, len(held), _ptr(self.buffer), int(precision),
                                            1 if training else 0, _stream())
        _lib.check(st, what)

    def forward(self, origins: Tensor, dirs: Tensor, view_dirs: Optional[Tensor], depths: Tensor,
                sigma_noise: Optional[Tensor] = None, precision: int = PRECISION_FP32):
        """-> sigma (n,S,1), rgb (n,S,3).  precision: a PRECISION_* value (enum snerf_precision), see the C header."""
        lib = _lib.load()
        n, s = depths.shape
        origins = _dev(origins, 'origins', (n, 3))
        dirs = _dev(dirs, 'dirs', (n, 3))
        depths = _dev(depths, 'depths')
        view_dirs = _dev(view_dirs, 'view_dirs', (n, 3)) if self.use_view_dirs else None
        if self.use_view_dirs and view_dirs is None:
            raise KeyError('view_dirs')
        if sigma_noise is not None:
            sigma_noise = _dev(sigma_noise.reshape(n, s), 'sigma_noise', (n, s))
        sigma = torch.empty((n, s, 1), dtype=torch.float32, device=depths.device)
        rgb = torch.empty((n, s, 3), dtype=torch.float32, device=depths.device)
        if n == 0:
            return sigma, rgb
        with torch.cuda.device(depths.device):
            st = lib.snerf_mlp_forward(ctypes.byref(self.desc), _ptr(self.buffer), _ptr(origins), _ptr(dirs),
                                       _ptr(view_dirs), _ptr(depths), n, s, _ptr(sigma_noise), _ptr(sigma), _ptr(rgb),
                                       int(precision), _stream())
        _lib.check(st, 'snerf_mlp_forward')
        return sigma, rgb


    # ---- training ------------------------------------------------------------------------------------------
    def forward_train(self, origins: Tensor, dirs: Tensor, view_dirs: Optional[Tensor], depths: Tensor,
                      sigma_noise: Optional[Tensor] = None, precision: int = PRECISION_FP32):
        """Forward that also keeps every layer's input for backward().  -> sigma (n,S,1), rgb (n,S,3), saved"""
        lib = _lib.load()
        n, s = depths.shape
        origins = _dev(origins, 'origins', (n, 3))
        dirs = _dev(dirs, 'dirs', (n, 3))
        depths = _dev(depths, 'depths')
        view_dirs = _dev(view_dirs, 'view_dirs', (n, 3)) if self.use_view_dirs else None
        if self.use_view_dirs and view_dirs is None:
            raise KeyError('view_dirs')
        if sigma_noise is not None:
            sigma_noise = _dev(sigma_noise.reshape(n, s), 'sigma_noise', (n, s))
        dev = depths.device
        sigma = torch.empty((n, s, 1), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, s, 3), dtype=torch.float32, device=dev)
        saved = torch.empty(lib.snerf_mlp_saved_floats(ctypes.byref(self.desc), n, s), dtype=torch.float32, device=dev)
        if n == 0:
            return sigma, rgb, saved
        with torch.cuda.device(dev):
            st = lib.snerf_mlp_forward_train(ctypes.byref(self.desc), _ptr(self.buffer), _ptr(origins), _ptr(dirs),
                                             _ptr(view_dirs), _ptr(depths), n, s, _ptr(sigma_noise), _ptr(sigma), _ptr(rgb),
                                             _ptr(saved), int(precision), _stream())
        _lib.check(st, 'snerf_mlp_forward_train')
        return sigma, rgb, saved

    def backward_workspace_floats(self, n: int, s: int) -> int:
        return int(_lib.load().snerf_mlp_backward_workspace_floats(ctypes.byref(self.desc), n, s))

    def backward(self, saved: Tensor, sigma: Tensor, rgb: Tensor, d_sigma: Tensor, d_rgb: Tensor,
                 param_shapes: List[tuple], precision: int = PRECISION_FP32, into: Optional[List[Tensor]] = None,
                 work: Optional[Tensor] = None) -> List[Tensor]:
        """dL/dparam for every parameter (C-ABI order), given dL/dsigma (n,S[,1]) and dL/drgb (n,S,3).  ``into``: existing
        gradient tensors to ADD to (the kernel accumulates; no separate add launches) instead of fresh ones.  ``work``: the
        caller's scratch (at least ``backward_workspace_floats(n, s)`` floats) instead of a fresh allocation."""
        lib = _lib.load()
        n, s = sigma.shape[0], sigma.shape[1]
        dev = sigma.device
        sigma = _dev(sigma.reshape(n, s), 'sigma', (n, s))
        rgb = _dev(rgb, 'rgb', (n, s, 3))
        d_sigma = _dev(d_sigma.reshape(n, s), 'd_sigma', (n, s))
        d_rgb = _dev(d_rgb, 'd_rgb', (n, s, 3))
        if len(param_shapes) != self.num_params:
            raise RuntimeError(f'expected {self.num_params} parameter shapes, got {len(param_shapes)}')
        if n == 0:
            return into if into is not None else [torch.zeros(tuple(shape), dtype=torch.float32, device=dev) for shape in param_shapes]
        if into is not None:
            for g, shape in zip(into, param_shapes):
                if tuple(g.shape) != tuple(shape) or g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
                    raise RuntimeError(f'backward(into=...): expected a contiguous float32 GPU tensor of shape {tuple(shape)}')
        grads = into if into is not None else [torch.empty(tuple(shape), dtype=torch.float32, device=dev) for shape in param_shapes]
        need = self.backward_workspace_floats(n, s)
        if work is None:
            work = torch.empty(need, dtype=torch.float32, device=dev)
        elif work.dtype != torch.float32 or not work.is_cuda or not work.is_contiguous() or work.numel() < need:
            raise RuntimeError(f'backward(work=...): expected a contiguous float32 GPU tensor of at least {need} floats')
        arr = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        with torch.cuda.device(dev):
            st = lib.snerf_mlp_backward(ctypes.byref(self.desc), _ptr(self.buffer), _ptr(saved), _ptr(sigma), _ptr(rgb),
                                        _ptr(d_sigma), _ptr(d_rgb), n, s, _ptr(work), arr, len(grads), int(precision),
                                        int(into is not None), _stream())
        _lib.check(st, 'snerf_mlp_backward')
        return grads

    def input_gradient_workspace_floats(self, n: int) -> int:
        """Floats of scratch ``input_gradient`` needs for ``n`` points; raises NotImplementedError, naming the limit, for an MLP the
        call is not built for (a layered shape, ``predict_visibility``)."""
        lib = _lib.load()
        need = int(lib.snerf_mlp_input_gradient_workspace_floats(ctypes.byref(self.desc), int(n)))
        if need == 0:
            msg = lib.snerf_last_error()
            raise NotImplementedError(msg.decode() if msg else 'mlp_input_gradient: not built for this MLP')
        return need

    def input_gradient(self, params: List[Tensor], saved: Tensor, sigma: Tensor, d_sigma: Optional[Tensor] = None,
                       work: Optional[Tensor] = None) -> Tensor:
        """-> float32 (n,3): ``d_sigma`` . d sigma / d point for the n points of a ``forward_train(points, zeros, view_dirs, zeros
        (n,1), None, PRECISION_FP32)`` call that returned ``sigma`` (n,1,1) and ``saved`` (snerf_mlp_input_gradient,
        csrc/simplenerf_gradient.h).  ``params``: the tensors this stream was packed from (C-ABI order), with
        ``pack(params, PRECISION_FP32, training=True)``; the first layer's and the skip layer's weights are read from them.
        ``d_sigma`` (n,) defaults to ones: the plain gradient.  fp32 and the fused MLP shapes only.  ``work``: the caller's scratch
        (at least ``input_gradient_workspace_floats(n)`` floats) instead of a fresh allocation."""
        lib = _lib.load()
        if len(params) != self.num_params:
            raise RuntimeError(f'expected {self.num_params} parameter tensors, got {len(params)}')
        held = [_dev(p, f'param[{i}]') for i, p in enumerate(params)]
        n = int(sigma.numel())
        dev = sigma.device
        sigma = _dev(sigma.reshape(n), 'sigma', (n,))
        saved = _dev(saved, 'saved')
        d_sigma = torch.ones((n,), dtype=torch.float32, device=dev) if d_sigma is None else _dev(d_sigma.reshape(-1), 'd_sigma', (n,))
        _warp_together(dev, saved=saved, d_sigma=d_sigma, buffer=self.buffer, **{f'param[{i}]': p for i, p in enumerate(held)})
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        need = self.input_gradient_workspace_floats(max(n, 1))
        if n == 0:
            return out
        have = int(lib.snerf_mlp_saved_floats(ctypes.byref(self.desc), n, 1))
        if saved.numel() < have:
            raise RuntimeError(f'saved: expected the {have} floats forward_train keeps for {n} points, got {saved.numel()}')
        if work is None:
            work = torch.empty(need, dtype=torch.float32, device=dev)
        elif work.dtype != torch.float32 or not work.is_cuda or not work.is_contiguous() or work.numel() < need or work.device != dev:
            raise RuntimeError(f'input_gradient(work=...): expected a contiguous float32 tensor of at least {need} floats on {dev}')
        arr = (ctypes.c_void_p * len(held))(*[p.data_ptr() for p in held])
        with torch.cuda.device(dev):
            st = lib.snerf_mlp_input_gradient(ctypes.byref(self.desc), _ptr(self.buffer), arr, len(held), _ptr(saved), _ptr(sigma),
                                              _ptr(d_sigma), n, _ptr(work), _ptr(out), _stream())
        _lib.check(st, 'snerf_mlp_input_gradient')
        return out


def check_input_gradient(mlp_cfg: dict) -> None:
    """Raises NotImplementedError, naming the limit, for an MLP config ``PackedMlp.input_gradient`` is not built for (a layered
    shape, ``predict_visibility``): the descriptor's own check on the host, without a device buffer or a launch."""
    lib = _lib.load()
    desc = mlp_desc(mlp_cfg)
    if int(lib.snerf_mlp_input_gradient_workspace_floats(ctypes.byref(desc), 1)) == 0:
        msg = lib.snerf_last_error()
        raise NotImplementedError(msg.decode() if msg else 'mlp_input_gradient: not built for this MLP')


# ---------------------------------------------------------------------------------------------- one-call render ops
PER_SAMPLE_BITS = {'alpha': 1, 'visibility': 2, 'weights': 4}     # the per-sample request mask of snerf_render_layout_query


class RenderLayout:
    """A ``snerf_render_layout`` (csrc/render_layout.h owns the rules) read into plain Python once: it does not depend on the ray
    count.  A slot is (pool, unit offset, trailing shape, strides of (n,) + trailing shape): pools[pool].as_strided((n,) + shape,
    strides, n * offset) is the output."""

    def __init__(self, c: _lib.RenderLayout):
        self.c = c
        self.samples, self.num_fine = tuple(c.samples), int(c.num_fine)
        self.pool_unit_floats, self.needs_workspace = tuple(c.pool_unit_floats), bool(c.needs_workspace)
        self.depths_coarse = self._slot(c.depths_coarse)
        self.depths_fine = self._slot(c.depths_fine) if c.depths_fine.present else None
        # (level, field name, slot) of every output the caller sees, in level and field order
        self.returned = tuple((l, name, self._slot(c.level[l][f])) for l in range(_lib.RENDER_LEVELS)
                              for f, name in enumerate(_lib.LEVEL_OUT_FIELDS) if c.level[l][f].returned)

    @staticmethod
    def _slot(slot):
        dims = tuple(slot.dims[:slot.rank])
        return slot.pool, int(slot.unit_offset), dims, tuple(math.prod(dims[i:]) for i in range(len(dims) + 1))


@functools.lru_cache(maxsize=None)
def render_layout(ndc: bool, num_coarse: int, num_fine: int, keep_activations: bool, levels: tuple, num_other: int,
                  per_sample_mask: int, fine_depths_given: bool) -> RenderLayout:
    """snerf_render_layout_query, cached per configuration.  ``levels``: per level None (absent) or whether its MLP predicts
    visibility -- all the query reads of an MLP."""
    cfg = _lib.RenderConfig(ndc=int(ndc), num_coarse=num_coarse, num_fine=num_fine, keep_activations=int(keep_activations))
    descs = [None if v is None else MlpDesc(predict_visibility=int(v)) for v in levels]
    mlps = (_lib.RenderMlp * _lib.RENDER_LEVELS)()
    for l, d in enumerate(descs):
        if d is not None:
            mlps[l].desc = ctypes.pointer(d)
    c = _lib.RenderLayout()
    _lib.check(_lib.load().snerf_render_layout_query(ctypes.byref(cfg), mlps, num_other, per_sample_mask, int(fine_depths_given),
                                                     ctypes.byref(c)), 'snerf_render_layout_query')
    return RenderLayout(c)


class RenderCall:
    """One ``snerf_render_forward`` (and, for training, its ``snerf_render_backward``): the whole of SimpleNeRF.render_rays
    (src/models/SimpleNeRF01.py:108-270) enqueued by ONE call into the library.  Output tensors are carved out of three
    allocations -- per-ray outputs, per-sample outputs, and (training) one saved-activation buffer per level -- instead
    of ~20 separate ones; which outputs there are and where they lie is the library's ``snerf_render_layout``.

    ``mlps``: six entries (C-ABI level order: main / points-aug / views-aug at the coarse level, then at the fine level),
    ``PackedMlp`` or None.  ``rays``: the reference's input_batch tensors.  ``draws``: t_rand, u, per-level sigma noise,
    optional fine-depth override.  ``per_sample``: which (n,S) composite outputs to produce ('alpha', 'visibility',
    'weights')."""

    def __init__(self, mlps: List[Optional['PackedMlp']], ndc: bool, white_bkgd: bool, lindisp: bool, num_coarse: int,
                 num_fine: int, precision: int, keep_activations: bool, per_sample=('alpha',), fused: bool = False):
        lib = _lib.load()
        self.lib = lib
        self.mlps = list(mlps) + [None] * (_lib.RENDER_LEVELS - len(mlps))
        self.ndc, self.keep = bool(ndc), bool(keep_activations)
        self.cfg = _lib.RenderConfig(int(bool(ndc)), int(bool(white_bkgd)), int(bool(lindisp)), int(num_coarse), int(num_fine),
                                     int(precision), int(self.keep), int(bool(fused) and not self.keep))
        self.c_mlps = (_lib.RenderMlp * _lib.RENDER_LEVELS)()
        for l, m in enumerate(self.mlps):
            if m is not None:
                self.c_mlps[l].desc = ctypes.pointer(m.desc)
                self.c_mlps[l].packed = m.buffer.data_ptr()
        self.per_sample_mask = sum(PER_SAMPLE_BITS[name] for name in set(per_sample))
        self.levels = [l for l, m in enumerate(self.mlps) if m is not None]
        self.c_rays = _lib.RenderRays()
        self.c_out = _lib.RenderOutputs()
        self.held: list = []      # tensors whose pointers sit in the structs

    def forward(self, rays: Dict[str, Tensor], draws: Dict[str, Optional[Tensor]]):
        """-> (z_vals_coarse, z_vals_fine or None, {level: {name: tensor}})"""
        lib = self.lib
        n = rays['rays_o'].shape[0]
        dev = rays['rays_o'].device
        self.n, self.device = n, dev
        r = self.c_rays
        held = self.held = []
        # predict_visibility: secondary camera centres (n, K, 3), K = num_frames - 1 (sec_views_vis)
        predicts = tuple(None if m is None else bool(m.desc.predict_visibility) for m in self.mlps)
        rays_o2 = rays.get('rays_o2') if any(predicts) else None
        k_other = 0 if rays_o2 is None else int(rays_o2.shape[1])
        override = draws.get('z_vals_fine')
        lay = self.layout = render_layout(self.ndc, self.cfg.num_coarse, self.cfg.num_fine, self.keep, predicts, k_other,
                                          self.per_sample_mask, override is not None)
        self.cfg.num_fine = lay.num_fine
        samples = lay.samples

        def put(name, t, shape):
            t = _dev(t, name, shape)
            held.append(t)
            return 0 if t is None else t.data_ptr()

        r.rays_o, r.rays_d = put('rays_o', rays['rays_o'], (n, 3)), put('rays_d', rays['rays_d'], (n, 3))
        need_dirs = any(self.mlps[l].desc.use_view_dirs for l in self.levels)
        if need_dirs and rays.get('view_dirs') is None:
            raise KeyError('view_dirs')
        r.view_dirs = put('view_dirs', rays.get('view_dirs'), (n, 3)) if need_dirs else 0
        if self.ndc:
            r.rays_o_ndc, r.rays_d_ndc = put('rays_o_ndc', rays['rays_o_ndc'], (n, 3)), put('rays_d_ndc', rays['rays_d_ndc'], (n, 3))
            near, far = rays['near_ndc'], rays['far_ndc']
        else:
            r.rays_o_ndc = r.rays_d_ndc = 0
            near, far = rays['near'], rays['far']
        r.near, r.far = put('near', near.reshape(-1), (n,)), put('far', far.reshape(-1), (n,))
        r.t_rand = put('t_rand', draws.get('t_rand'), (n, samples[0]))
        r.u = put('u', draws.get('u'), (n, lay.num_fine)) if lay.num_fine else 0
        for l in range(_lib.RENDER_LEVELS):
            noise = draws.get(('noise', l)) if l in self.levels else None
            r.sigma_noise[l] = put('sigma_noise', None if noise is None else noise.reshape(n, samples[l]), (n, samples[l]))
        r.depths_fine = put('z_vals_fine', override if lay.num_fine else None, (n, samples[3]))
        fine_in = held[-1]        # the validated (contiguous fp32) override, or None: returned as z_vals_fine below
        r.rays_o2 = put('rays_o2', rays_o2, (n, k_other, 3)) if k_other else 0
        r.num_other = k_other

        # ---- outputs: one allocation per pool, one view per output the caller sees (as_strided: slice + view would be two ops)
        pools = [torch.empty((unit * n,), dtype=torch.float32, device=dev) for unit in lay.pool_unit_floats]

        def view(slot):
            pool, offset, dims, strides = slot
            return pools[pool].as_strided((n,) + dims, strides, n * offset)

        o = self.c_out
        _lib.check(lib.snerf_render_layout_bind(ctypes.byref(lay.c), n, _ptr(pools[0]), _ptr(pools[1]), ctypes.byref(o)),
                   'snerf_render_layout_bind')
        z_coarse = view(lay.depths_coarse)
        z_fine = fine_in if lay.depths_fine is None else view(lay.depths_fine)
        out: Dict[int, Dict[str, Tensor]] = {l: {} for l in self.levels}
        for l, name, slot in lay.returned:
            out[l][name] = view(slot)
        saved = [torch.empty((lib.snerf_mlp_saved_floats(ctypes.byref(self.mlps[l].desc), n, samples[l]),), dtype=torch.float32,
                             device=dev) for l in self.levels] if self.keep else []
        self.saved = dict(zip(self.levels, saved))      # level -> its saved activations (keep_activations only)
        for l, t in self.saved.items():
            o.level[l].saved_acts = t.data_ptr()
        work = None
        if lay.needs_workspace:
            work = torch.empty((lib.snerf_render_workspace_floats(ctypes.byref(self.cfg), n),), dtype=torch.float32, device=dev)
        if n > 0:
            with torch.cuda.device(dev):
                st = lib.snerf_render_forward(ctypes.byref(self.cfg), self.c_mlps, ctypes.byref(r), n, ctypes.byref(o), _ptr(work),
                                              _stream())
            _lib.check(st, 'snerf_render_forward')
        # what backward() needs alive is the memory behind the pointers in the structs: the two pools, the saved
        # activations and the inputs.  The output VIEWS are not kept here: under autograd they carry the node that owns
        # this object, and holding them would close a reference cycle that only the cycle collector frees (GBs per call)
        held += pools + saved
        return z_coarse, z_fine, out

    def backward(self, grads: Dict[int, Dict[str, Optional[Tensor]]], param_grads: Dict[int, List[Tensor]],
                 accumulate: Dict[int, bool]) -> None:
        """``grads[level]``: dL/d(rgb, acc, depth, depth_ndc, sigma, raw_rgb) (missing/None = zero);
        ``param_grads[level]``: the level's gradient tensors in C-ABI order, overwritten or (``accumulate[level]``) added to."""
        lib = self.lib
        n, dev = self.n, self.device
        if n == 0:
            return
        c_grads = (_lib.RenderLevelGrads * _lib.RENDER_LEVELS)()
        keep = []
        for l in self.levels:
            g = grads.get(l) or {}
            if l not in param_grads or not any(g.get(k) is not None for k in ('rgb', 'acc', 'depth', 'depth_ndc', 'sigma', 'raw_rgb')):
                continue
            s = self.layout.samples[l]
            cg = c_grads[l]
            for name, shape in (('rgb', (n, 3)), ('acc', (n,)), ('depth', (n,)), ('depth_ndc', (n,)), ('sigma', (n, s, 1)),
                                ('raw_rgb', (n, s, 3))):
                t = g.get(name)
                if t is not None:
                    t = _dev(t.reshape(shape), f'grad {name}', shape)
                    keep.append(t)
                setattr(cg, name, 0 if t is None else t.data_ptr())
            tensors = param_grads[l]
            if len(tensors) != self.mlps[l].num_params:
                raise RuntimeError(f'level {l}: expected {self.mlps[l].num_params} gradient tensors, got {len(tensors)}')
            arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            keep.append(arr)
            cg.param_grads = arr
            cg.num_params = len(tensors)
            cg.accumulate = int(bool(accumulate.get(l, False)))
        work = torch.empty((lib.snerf_render_backward_workspace_floats(ctypes.byref(self.cfg), self.c_mlps, n),),
                           dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = lib.snerf_render_backward(ctypes.byref(self.cfg), self.c_mlps, ctypes.byref(self.c_rays), n,
                                           ctypes.byref(self.c_out), c_grads, _ptr(work), _stream())
        _lib.check(st, 'snerf_render_backward')


# ---------------------------------------------------------------------------------------------- view sweep
SWEEP_BASE_PRECISION = {PRECISION_F16S8: PRECISION_F16, PRECISION_BF16S8: PRECISION_BF16}      # the 8-bit modes render as their base mode


@torch.no_grad()
def render_keep_activations(mlps: List[Optional['PackedMlp']], rays: Dict[str, Tensor], ndc: bool, white_bkgd: bool, lindisp: bool,
                            num_coarse: int, num_fine: int, z_vals_fine: Optional[Tensor] = None,
                            precision: int = PRECISION_FP32) -> Dict[str, object]:
    """One ``snerf_render_forward`` that keeps the activations without recording a backward: no jitter, no density noise.
    ``mlps`` as ``RenderCall`` takes them, packed for the training layout at ``precision`` (the storing forward reads it).
    ``precision``: 'f16s8' / 'bf16s8' run as 'f16' / 'bf16' -- their rendering is the base mode's bit for bit, and what a sweep
    reads of the activations must not depend on how the 8-bit forwards keep their trunk tiles.  Returns, for the level a
    frame is displayed from (the fine MLP's, the coarse one's without a fine MLP): 'level', 'num_samples', 'saved_acts',
    'weights' (n,S), 'acc' (n,) and 'outputs', that level's per-ray outputs by name (rgb, acc, depth, depth_var, ...)."""
    call = RenderCall(mlps, ndc, white_bkgd, lindisp, num_coarse, num_fine, SWEEP_BASE_PRECISION.get(precision, precision), keep_activations=True,
                      per_sample=('alpha', 'weights'))
    draws = {} if z_vals_fine is None else {'z_vals_fine': z_vals_fine}
    _, _, levels = call.forward(rays, draws)
    level = 3 if call.mlps[3] is not None else 0
    out = levels[level]
    return {'level': level, 'num_samples': call.layout.samples[level], 'saved_acts': call.saved[level], 'weights': out['weights'],
            'acc': out['acc'], 'outputs': out}


def view_sweep(mlp: 'PackedMlp', params: List[Tensor], saved_acts: Tensor, weights: Tensor, acc: Optional[Tensor], view_dirs: Tensor,
               white_bkgd: bool = False) -> Tensor:
    """snerf_view_sweep (csrc/simplenerf_sweep.h): the colour (V,n,3) of n composited rays under V sets of view directions
    (V,n,3), from the fp32 activations ``saved_acts`` a storing forward of ``mlp`` kept for these rays, their ``weights`` (n,S) and
    -- with ``white_bkgd`` -- ``acc`` (n,).  ``params``: the MLP's parameter tensors in C-ABI order, as ``PackedMlp.pack`` takes them."""
    lib = _lib.load()
    n, s = weights.shape
    v = view_dirs.shape[0]
    weights = _dev(weights, 'weights', (n, s))
    acc = _dev(acc, 'acc', (n,)) if white_bkgd else None
    view_dirs = _dev(view_dirs, 'view_dirs', (v, n, 3))
    saved_acts = _dev(saved_acts, 'saved_acts')
    dev = weights.device
    need = int(lib.snerf_mlp_saved_floats(ctypes.byref(mlp.desc), n, s))
    if saved_acts.numel() < need:
        raise RuntimeError(f'saved_acts: {saved_acts.numel()} floats, {n} rays x {s} samples of this MLP keep {need}')
    if len(params) != mlp.num_params:
        raise RuntimeError(f'expected {mlp.num_params} parameter tensors, got {len(params)}')
    held = [_dev(p, f'param[{i}]') for i, p in enumerate(params)]
    arr = (ctypes.c_void_p * len(held))(*[p.data_ptr() for p in held])
    out = torch.empty((v, n, 3), dtype=torch.float32, device=dev)
    floats = int(lib.snerf_view_sweep_workspace_floats(ctypes.byref(mlp.desc), n, s, v))
    work = _workspace('view_sweep', dev, 4 * floats) if floats else None
    _enqueue('snerf_view_sweep', dev, ctypes.byref(mlp.desc), arr, len(held), _ptr(saved_acts), _ptr(weights), _ptr(acc),
             _ptr(view_dirs), n, s, v, int(bool(white_bkgd)), _ptr(out), _ptr(work))
    return out


def view_sweep_half(mlp: 'PackedMlp', params: List[Tensor], saved_acts: Tensor, weights: Tensor, acc: Optional[Tensor],
                    view_dirs: Tensor, white_bkgd: bool = False, precision: int = PRECISION_BF16) -> Tensor:
    """snerf_view_sweep_half (csrc/simplenerf_sweep16.h): ``view_sweep`` from the 16-bit activations a storing forward of ``mlp``
    kept at ``precision`` (PRECISION_F16 or PRECISION_BF16; the 8-bit modes keep ``feature`` like their base mode and are mapped to
    it), with the views layer's operands rounded to that format as the mode's own render rounds them."""
    lib = _lib.load()
    n, s = weights.shape
    v = view_dirs.shape[0]
    weights = _dev(weights, 'weights', (n, s))
    acc = _dev(acc, 'acc', (n,)) if white_bkgd else None
    view_dirs = _dev(view_dirs, 'view_dirs', (v, n, 3))
    saved_acts = _dev(saved_acts, 'saved_acts')
    dev = weights.device
    need = int(lib.snerf_view_sweep_half_acts_floats(ctypes.byref(mlp.desc), n, s))
    if saved_acts.numel() < need:
        raise RuntimeError(f'saved_acts: {saved_acts.numel()} floats, the sweep of {n} rays x {s} samples of this MLP reads {need}')
    if len(params) != mlp.num_params:
        raise RuntimeError(f'expected {mlp.num_params} parameter tensors, got {len(params)}')
    held = [_dev(p, f'param[{i}]') for i, p in enumerate(params)]
    arr = (ctypes.c_void_p * len(held))(*[p.data_ptr() for p in held])
    out = torch.empty((v, n, 3), dtype=torch.float32, device=dev)
    floats = int(lib.snerf_view_sweep_half_workspace_floats(ctypes.byref(mlp.desc), n, s, v))
    work = _workspace('view_sweep_half', dev, 4 * floats) if floats else None
    precision = SWEEP_BASE_PRECISION.get(int(precision), int(precision))
    _enqueue('snerf_view_sweep_half', dev, ctypes.byref(mlp.desc), arr, len(held), _ptr(saved_acts), _ptr(weights), _ptr(acc),
             _ptr(view_dirs), n, s, v, int(bool(white_bkgd)), precision, _ptr(out), _ptr(work))
    return out


# ---------------------------------------------------------------------------------------------- K4
def composite(sigma: Tensor, rgb: Tensor, depths: Tensor, march_dirs: Tensor, ndc: bool, white_bkgd: bool = False,
              rays_o: Optional[Tensor] = None, rays_d: Optional[Tensor] = None,
              per_sample: bool = True) -> Dict[str, Tensor]:
    """Keys as the reference's volume_rendering: rgb, acc, alpha, visibility, weights, depth, depth_var
    (+ depth_ndc, depth_var_ndc when ndc).  per_sample=False skips alpha/visibility/weights."""
    n, s = depths.shape
    sigma = _dev(sigma.reshape(n, s), 'sigma', (n, s))
    rgb = _dev(rgb, 'rgb', (n, s, 3))
    depths = _dev(depths, 'depths')
    march_dirs = _dev(march_dirs, 'march_dirs', (n, 3))
    dev = depths.device
    out = {'rgb': torch.empty((n, 3), dtype=torch.float32, device=dev)}
    for k in ('acc', 'depth', 'depth_var') + (('depth_ndc', 'depth_var_ndc') if ndc else ()):
        out[k] = torch.empty((n,), dtype=torch.float32, device=dev)
    if per_sample:
        for k in ('alpha', 'visibility', 'weights'):
            out[k] = torch.empty((n, s), dtype=torch.float32, device=dev)
    if ndc:
        rays_o = _dev(rays_o, 'rays_o', (n, 3))
        rays_d = _dev(rays_d, 'rays_d', (n, 3))
    if n == 0:
        return out
    _enqueue('snerf_composite', dev, _ptr(sigma), _ptr(rgb), _ptr(depths), _ptr(march_dirs), _ptr(rays_o if ndc else None),
             _ptr(rays_d if ndc else None), n, s, int(bool(ndc)), int(bool(white_bkgd)), _ptr(out['rgb']), _ptr(out['acc']),
             _ptr(out.get('alpha')), _ptr(out.get('visibility')), _ptr(out.get('weights')), _ptr(out['depth']),
             _ptr(out['depth_var']), _ptr(out.get('depth_ndc')), _ptr(out.get('depth_var_ndc')))
    return out


# ---------------------------------------------------------------------------------------------- K6
def composite_backward(sigma: Tensor, rgb: Tensor, depths: Tensor, march_dirs: Tensor, ndc: bool, white_bkgd: bool,
                       rays_o: Optional[Tensor], rays_d: Optional[Tensor], grad_rgb: Optional[Tensor],
                       grad_acc: Optional[Tensor], grad_depth: Optional[Tensor], grad_depth_ndc: Optional[Tensor]):
    """-> d_sigma (n,S), d_rgb (n,S,3) from the per-ray gradients (None = zero)."""
    n, s = depths.shape
    sigma = _dev(sigma.reshape(n, s), 'sigma', (n, s))
    rgb = _dev(rgb, 'rgb', (n, s, 3))
    depths = _dev(depths, 'depths')
    march_dirs = _dev(march_dirs, 'march_dirs', (n, 3))
    if ndc:
        rays_o = _dev(rays_o, 'rays_o', (n, 3))
        rays_d = _dev(rays_d, 'rays_d', (n, 3))
    grad_rgb = _dev(grad_rgb, 'grad_rgb', (n, 3))
    grad_acc = _dev(grad_acc, 'grad_acc', (n,))
    grad_depth = _dev(grad_depth, 'grad_depth', (n,))
    grad_depth_ndc = _dev(grad_depth_ndc, 'grad_depth_ndc', (n,))
    dev = depths.device
    d_sigma = torch.empty((n, s), dtype=torch.float32, device=dev)
    d_rgb = torch.empty((n, s, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return d_sigma, d_rgb
    _enqueue('snerf_composite_backward', dev, _ptr(sigma), _ptr(rgb), _ptr(depths), _ptr(march_dirs),
             _ptr(rays_o if ndc else None), _ptr(rays_d if ndc else None), n, s, int(bool(ndc)), int(bool(white_bkgd)),
             _ptr(grad_rgb), _ptr(grad_acc), _ptr(grad_depth), _ptr(grad_depth_ndc), _ptr(d_sigma), _ptr(d_rgb))
    return d_sigma, d_rgb


# ---------------------------------------------------------------------------------------------- K5
def resample_depths(depths_coarse: Tensor, weights_coarse: Tensor, num_fine: int, u: Optional[Tensor] = None) -> Tensor:
    n, s_c = depths_coarse.shape
    depths_coarse = _dev(depths_coarse, 'depths_coarse')
    weights_coarse = _dev(weights_coarse, 'weights_coarse', (n, s_c))
    u = _dev(u, 'u', (n, num_fine))
    out = torch.empty((n, s_c + num_fine), dtype=torch.float32, device=depths_coarse.device)
    if n == 0:
        return out
    _enqueue('snerf_resample_depths', depths_coarse.device, _ptr(depths_coarse), _ptr(weights_coarse), n, s_c, int(num_fine),
             _ptr(u), _ptr(out))
    return out


# ---------------------------------------------------------------------------------------------- f3
def to_display(rgb: Optional[Tensor], depth: Optional[Tensor] = None, colour: bool = True):
    """-> uint8 image (n,3) [clip to [0,1], round(255 x) half-to-even] and depth clipped at 0 (or None).
    ``colour=False`` converts only the depth column (image is None)."""
    n = rgb.shape[0] if colour else depth.shape[0]
    rgb = _dev(rgb, 'rgb', (n, 3)) if colour else None
    depth = _dev(depth, 'depth', (n,))
    dev = rgb.device if colour else depth.device
    image = torch.empty((n, 3), dtype=torch.uint8, device=dev) if colour else None
    depth_out = None if depth is None else torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0:
        return image, depth_out
    _enqueue('snerf_to_display', dev, _ptr(rgb), _ptr(depth), n, ctypes.c_void_p(0 if image is None else image.data_ptr()),
             _ptr(depth_out))
    return image, depth_out


MAP_SCALE_255, MAP_SCALE_MAX = 0, 1      # the modes of snerf_maps_to_u8: rint(x * 255); rint(x / max(x) * 255)
_map_modes: Dict[tuple, Tensor] = {}


def maps_to_u8(maps: Tensor, modes):
    """-> (uint8 (K, n), int32 status (K)) on the device, for ``maps`` (K, n) float32 and one mode per map: 0 = ``rint(x * 255)``
    (the reference's save_image; a colour frame is three rows of mode 0), 1 = ``rint(x / max(x) * 255)`` (its save_numpy_array
    preview), in numpy's float32 arithmetic, saturating to 0..255.  Status 1: a mode-1 map whose maximum is not a positive finite
    number (its row is zeros).  All K maps go through two launches; a contiguous view is taken as it is, wherever it starts."""
    maps = _dev(maps, 'maps')
    if maps.dim() != 2:
        raise RuntimeError(f'maps: expected shape (K, n), got {tuple(maps.shape)}')
    modes = tuple(int(m) for m in modes)
    count, n = int(maps.shape[0]), int(maps.shape[1])
    if len(modes) != count or any(m not in (MAP_SCALE_255, MAP_SCALE_MAX) for m in modes):
        raise RuntimeError(f'modes: expected {count} values of 0 or 1, got {modes}')
    dev = maps.device
    out = torch.empty((count, n), dtype=torch.uint8, device=dev)
    status = torch.zeros((count,), dtype=torch.int32, device=dev)
    if count == 0 or n == 0:
        return out, status
    on_device = _map_modes.get((modes, dev))
    if on_device is None:
        if len(_map_modes) > 64:
            _map_modes.clear()
        on_device = _map_modes[(modes, dev)] = torch.tensor(modes, dtype=torch.int32, device=dev)
    workspace = _workspace('maps_u8', dev, int(_lib.load().snerf_maps_to_u8_workspace_bytes(count)))
    _enqueue('snerf_maps_to_u8', dev, _ptr(maps), _ptr(on_device), count, n, _ptr(out), _ptr(status), _ptr(workspace))
    return out, status


PNG_FILTER_ADAPTIVE = C.SNERF_PNG_FILTER_ADAPTIVE      # filter_mode of snerf_png_deflate: the cheapest type per row; 0..4: that type on every row


def png_deflate(images: Tensor, filter_mode: int = PNG_FILTER_ADAPTIVE):
    """-> (streams uint8 (K, bound), sizes int64 (K)) on the device for ``images`` uint8 (K, h, w) grey or (K, h, w, 3) RGB on the
    device: ``streams[i, :sizes[i]]`` is the complete zlib stream of frame i's IDAT chunk -- PNG row filtering (``filter_mode``),
    run-length tokens and one dynamic Huffman block per 32 KiB of filtered bytes (csrc/simplenerf_png.h has the contract).  The PNG
    container around a stream is the caller's (``harness.png_files``).  All K frames go through one call of four launches."""
    images = _typed(images, 'images', (torch.uint8,))
    if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] != 3):
        raise RuntimeError(f'images: expected shape (K, h, w) or (K, h, w, 3), got {tuple(images.shape)}')
    count, h, w = (int(v) for v in images.shape[:3])
    channels = 3 if images.dim() == 4 else 1
    dev, lib = images.device, _lib.load()
    bound = int(lib.snerf_png_deflate_bound_bytes(h, w, channels))
    streams = torch.empty((count, bound), dtype=torch.uint8, device=dev)
    sizes = torch.zeros((count,), dtype=torch.int64, device=dev)
    workspace = _workspace('png', dev, int(lib.snerf_png_deflate_workspace_bytes(count, h, w, channels))) if count and bound else None
    # (an image the library does not take -- an empty one, 2 GiB of rows -- has bound 0 and no workspace: the call names the reason)
    _enqueue('snerf_png_deflate', dev, _ptr(images), count, h, w, channels, int(filter_mode), _ptr(streams), _ptr(sizes),
             _ptr(workspace))
    return streams, sizes


JPEG_BINDINGS = ('ctypes', 'torch_ext')


def jpeg_scan(images: Tensor, quality: int = 90, binding: str = 'ctypes'):
    """-> (scans uint8 (K, bound), sizes int64 (K)) on the device for ``images`` uint8 (K, h, w) grey or (K, h, w, 3) RGB on the
    device: ``scans[i, :sizes[i]]`` is the entropy-coded segment of frame i's baseline JPEG scan at ``quality`` 1..100 -- YCbCr
    4:2:0 (or one grey component), integer DCT, the Annex K tables, one restart interval per MCU row (csrc/simplenerf_jpeg.h has the
    contract).  The markers around a segment are the caller's (``harness.jpeg_files``).  All K frames go through one call of three
    launches.  ``binding``: 'ctypes' (the torch-free binding) or 'torch_ext' (``torch.ops.snerf.jpeg_scan``); the same bytes."""
    if binding not in JPEG_BINDINGS:
        raise RuntimeError(f"binding: expected 'ctypes' or 'torch_ext', got {binding!r}")
    images = _typed(images, 'images', (torch.uint8,))
    if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] != 3):
        raise RuntimeError(f'images: expected shape (K, h, w) or (K, h, w, 3), got {tuple(images.shape)}')
    if binding == 'torch_ext':
        from . import _torch_ext
        with torch.cuda.device(images.device):
            return tuple(_torch_ext.load().jpeg_scan(images, int(quality)))
    count, h, w = (int(v) for v in images.shape[:3])
    channels = 3 if images.dim() == 4 else 1
    dev, lib = images.device, _lib.load()
    bound = int(lib.snerf_jpeg_scan_bound_bytes(h, w, channels))
    scans = torch.empty((count, bound), dtype=torch.uint8, device=dev)
    sizes = torch.zeros((count,), dtype=torch.int64, device=dev)
    workspace = _workspace('jpeg', dev, int(lib.snerf_jpeg_scan_workspace_bytes(count, h, w, channels))) if count and bound else None
    # (an image the library does not take -- an empty one, a side above 65535 -- has bound 0 and no workspace: the call names the reason)
    _enqueue('snerf_jpeg_scan', dev, _ptr(images), count, h, w, channels, int(quality), _ptr(scans), _ptr(sizes), _ptr(workspace))
    return scans, sizes


# ---------------------------------------------------------------------------------------------- Q1 frame metrics
def _typed(t, name: str, dtypes, shape=None) -> Tensor:
    """Validate a device operand of one of ``dtypes`` (the metric inputs are uint8 / bool / float32); contiguous on return."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'{name}: expected a tensor on the GPU (the HIP renderer has no CPU path), got '
                           f'{type(t).__name__}{"" if not isinstance(t, torch.Tensor) else " on " + str(t.device)}')
    if t.dtype not in dtypes:
        raise RuntimeError(f'{name}: expected {" or ".join(str(d).replace("torch.", "") for d in dtypes)}, got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    return t.detach().contiguous()


SSIM_WINDOW = 11     # taps of the Gaussian window (sigma 1.5, truncate 3.5): the shortest side an image may have


def _metric_workspace(dev: torch.device, height: int, width: int) -> Tensor:
    """Scratch of the metric reductions (per-workgroup partial sums)."""
    return _workspace('metric', dev, int(_lib.load().snerf_metrics_workspace_bytes(int(height), int(width))))


def _image_pair(gt: Tensor, image: Tensor, mask: Optional[Tensor]):
    gt = _typed(gt, 'gt_image', (torch.uint8,))
    if gt.dim() != 3 or gt.shape[2] != 3:
        raise RuntimeError(f'gt_image: expected shape (h, w, 3), got {tuple(gt.shape)}')
    h, w = int(gt.shape[0]), int(gt.shape[1])
    image = _typed(image, 'eval_image', (torch.uint8,), (h, w, 3))
    if mask is not None:
        mask = _typed(mask, 'mask', (torch.bool, torch.uint8), (h, w))
    return gt, image, mask, h, w


def image_error_sums(gt: Tensor, image: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """-> int64 (3) on the device: sum (gt - eval)^2 over h*w*3, the same over the masked pixels, the masked pixel count."""
    gt, image, mask, h, w = _image_pair(gt, image, mask)
    if h < 1 or w < 1:
        raise RuntimeError(f'gt_image: empty image {tuple(gt.shape)}')
    sums = torch.empty((3,), dtype=torch.int64, device=gt.device)
    _enqueue('snerf_image_error_sums', gt.device, _ptr(gt), _ptr(image), _ptr(mask), h, w, _ptr(sums),
             _ptr(_metric_workspace(gt.device, h, w)))
    return sums


def ssim_sums(gt: Tensor, image: Tensor, mask: Optional[Tensor] = None, return_map: bool = False):
    """-> float64 (2) on the device: sum of the SSIM map S cropped by 5 pixels per side; sum of S over the masked pixels (every
    pixel without a mask) -- with a mask, S is that of (gt, where(mask, eval, gt)).  ``return_map``: also S, float64 (h,w,3)."""
    gt, image, mask, h, w = _image_pair(gt, image, mask)
    if min(h, w) < SSIM_WINDOW:
        raise RuntimeError(f'gt_image: the {SSIM_WINDOW}-tap SSIM window exceeds the image extent {h} x {w}: every side must be '
                           f'at least {SSIM_WINDOW}')
    sums = torch.empty((2,), dtype=torch.float64, device=gt.device)
    s_map = torch.empty((h, w, 3), dtype=torch.float64, device=gt.device) if return_map else None
    _enqueue('snerf_ssim_sums', gt.device, _ptr(gt), _ptr(image), _ptr(mask), h, w, _ptr(sums), _ptr(s_map),
             _ptr(_metric_workspace(gt.device, h, w)))
    return (sums, s_map) if return_map else sums


def depth_error_sums(gt: Tensor, depth: Tensor, gt_scale: float = 1.0, eval_scale: float = 1.0, mask: Optional[Tensor] = None,
                     sorted_gt: Optional[Tensor] = None) -> Tensor:
    """-> float64 (4) on the device: sum |e|, sum e^2, pixels counted, median(gt * gt_scale) (NaN without ``sorted_gt``) for
    e = gt * gt_scale - eval * eval_scale on the masked (or all) pixels."""
    gt = _typed(gt, 'gt_depth', (torch.float32,))
    depth = _typed(depth, 'eval_depth', (torch.float32,), tuple(gt.shape))
    n = gt.numel()
    if n < 1:
        raise RuntimeError(f'gt_depth: empty depth map {tuple(gt.shape)}')
    if mask is not None:
        mask = _typed(mask, 'mask', (torch.bool, torch.uint8), tuple(gt.shape))
    if sorted_gt is not None:
        sorted_gt = _typed(sorted_gt, 'sorted_gt', (torch.float32,), (n,))
    sums = torch.full((4,), float('nan'), dtype=torch.float64, device=gt.device)
    _enqueue('snerf_depth_error_sums', gt.device, _ptr(gt), _ptr(depth), float(gt_scale), float(eval_scale), _ptr(mask), n,
             _ptr(sorted_gt), _ptr(sums), _ptr(_metric_workspace(gt.device, 1, 1)))
    return sums


def rank_correlation_sums(x: Tensor, y: Tensor, sorted_x: Tensor, sorted_y: Tensor) -> Tensor:
    """-> float64 (3) on the device: sum rx ry, sum rx^2, sum ry^2 of the centred tie-averaged ranks of the flat x, y."""
    x = _typed(x, 'x', (torch.float32,))
    n = x.numel()
    if x.dim() != 1 or n < 1:
        raise RuntimeError(f'x: expected a non-empty flat tensor, got {tuple(x.shape)}')
    y = _typed(y, 'y', (torch.float32,), (n,))
    sorted_x = _typed(sorted_x, 'sorted_x', (torch.float32,), (n,))
    sorted_y = _typed(sorted_y, 'sorted_y', (torch.float32,), (n,))
    sums = torch.empty((3,), dtype=torch.float64, device=x.device)
    _enqueue('snerf_rank_correlation_sums', x.device, _ptr(x), _ptr(y), _ptr(sorted_x), _ptr(sorted_y), n, _ptr(sums),
             _ptr(_metric_workspace(x.device, 1, 1)))
    return sums


# ---------------------------------------------------------------------------------------------- Q2 visibility masks
VISIBILITY_CAMERA = 30     # doubles per training view: inv(K_train) 3x3 | rows 0..2 of E_test inv(E_train) 3x4 | K_test 3x3


def _visibility_extent(views: int, h: int, w: int, name: str) -> int:
    """Keys per view; refuses what the int32 keys cannot hold."""
    per_view = (h + 1) * (w + 1) + 1
    if views < 1 or h < 1 or w < 1 or views > 65535 or views * per_view >= 2 ** 31 - 1:
        raise RuntimeError(f'{name}: {views} views of {h} x {w} are empty or exceed the int32 keys of the splat')
    return per_view


def visibility_mask_project(depth_train: Tensor, cameras: Tensor):
    """Project every pixel of the (T,h,w) float32 training depths into the test view.  ``cameras``: float64 (T,30) on the device,
    per view inv(K_train) | rows 0..2 of E_test inv(E_train) | K_test, row-major.  -> points float64 (T,3,h,w) (padded position
    X, Y and transformed depth Z), keys int32 (T,h,w) (the list of every source), stats float64 (T,2) (max log-depth, max depth)."""
    depth_train = _typed(depth_train, 'depth_train', (torch.float32,))
    if depth_train.dim() != 3:
        raise RuntimeError(f'depth_train: expected shape (views, h, w), got {tuple(depth_train.shape)}')
    views, h, w = (int(s) for s in depth_train.shape)
    _visibility_extent(views, h, w, 'depth_train')
    cameras = _typed(cameras, 'cameras', (torch.float64,), (views, VISIBILITY_CAMERA))
    dev = depth_train.device
    points = torch.empty((views, 3, h, w), dtype=torch.float64, device=dev)
    keys = torch.empty((views, h, w), dtype=torch.int32, device=dev)
    stats = torch.empty((views, 2), dtype=torch.float64, device=dev)
    ws = _workspace('visibility', dev, int(_lib.load().snerf_visibility_mask_workspace_bytes(views, h, w)))
    _enqueue('snerf_visibility_mask_project', dev, _ptr(depth_train), _ptr(cameras), views, h, w, _ptr(points), _ptr(keys),
             _ptr(stats), _ptr(ws))
    return points, keys, stats


def visibility_mask_list_starts(sorted_keys: Tensor, views: int, h: int, w: int) -> Tensor:
    """-> int32 (T * keys_per_view + 1) on the device: where the list of every key begins in the flat ascending ``sorted_keys``."""
    views, h, w = int(views), int(h), int(w)
    per_view = _visibility_extent(views, h, w, 'sorted_keys')
    sorted_keys = _typed(sorted_keys, 'sorted_keys', (torch.int32,), (views * h * w,))
    starts = torch.empty((views * per_view + 1,), dtype=torch.int32, device=sorted_keys.device)
    _enqueue('snerf_visibility_mask_list_starts', sorted_keys.device, _ptr(sorted_keys), views, h, w, _ptr(starts))
    return starts


def visibility_mask_gather(points: Tensor, order: Tensor, starts: Tensor, stats: Tensor, depth_test: Tensor,
                           depth_error_threshold: float = 0.05, return_views: bool = False):
    """Sum every test pixel's sources through the inverted index (``order``: the int64 permutation of the STABLE sort of the keys,
    ``starts``: visibility_mask_list_starts) and apply the depth test.  -> uint8 (T,h,w) per-view masks; ``return_views``: also the
    float64 (T,h,w) warped depths and weight sums."""
    points = _typed(points, 'points', (torch.float64,))
    if points.dim() != 4 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected shape (views, 3, h, w), got {tuple(points.shape)}')
    views, h, w = int(points.shape[0]), int(points.shape[2]), int(points.shape[3])
    per_view = _visibility_extent(views, h, w, 'points')
    order = _typed(order, 'order', (torch.int64,), (views * h * w,))
    starts = _typed(starts, 'starts', (torch.int32,), (views * per_view + 1,))
    stats = _typed(stats, 'stats', (torch.float64,), (views, 2))
    depth_test = _typed(depth_test, 'depth_test', (torch.float32,), (h, w))
    dev = points.device
    mask_views = torch.empty((views, h, w), dtype=torch.uint8, device=dev)
    warped = torch.empty((views, h, w), dtype=torch.float64, device=dev) if return_views else None
    weights = torch.empty((views, h, w), dtype=torch.float64, device=dev) if return_views else None
    _enqueue('snerf_visibility_mask_gather', dev, _ptr(points), _ptr(order), _ptr(starts), _ptr(stats), _ptr(depth_test),
             float(depth_error_threshold), views, h, w, _ptr(mask_views), _ptr(warped), _ptr(weights))
    return (mask_views, warped, weights) if return_views else mask_views


def visibility_mask_combine(mask_views: Tensor, min_views: int = 2) -> Tensor:
    """-> bool (h,w) on the device: at least ``min_views`` of the uint8 / bool (T,h,w) per-view masks are set."""
    mask_views = _typed(mask_views, 'mask_views', (torch.uint8, torch.bool))
    if mask_views.dim() != 3:
        raise RuntimeError(f'mask_views: expected shape (views, h, w), got {tuple(mask_views.shape)}')
    views, h, w = (int(s) for s in mask_views.shape)
    _visibility_extent(views, h, w, 'mask_views')
    if not 1 <= int(min_views) <= views:
        raise RuntimeError(f'min_views: expected 1..{views} (the number of training views), got {min_views}')
    mask = torch.empty((h, w), dtype=torch.bool, device=mask_views.device)
    _enqueue('snerf_visibility_mask_combine', mask_views.device, _ptr(mask_views), views, h, w, int(min_views), _ptr(mask))
    return mask


# ---------------------------------------------------------------------------------------------- Q4 sorts and mask compaction
SORT_MAX_COUNT = 2 ** 31 - 1


def _sort_workspace(dev: torch.device, need: int) -> Tensor:
    """Scratch of the sorts and the compaction (second key / index buffers, digit counters); never an empty tensor."""
    return _workspace('sort', dev, max(need, 1))


def _flat(t: Tensor, name: str) -> int:
    if t.dim() != 1:
        raise RuntimeError(f'{name}: expected a flat tensor, got shape {tuple(t.shape)}')
    if t.numel() > SORT_MAX_COUNT:
        raise RuntimeError(f'{name}: {t.numel()} elements exceed the 2^31 - 1 the sort kernels index')
    return t.numel()


def sort_values(x: Tensor) -> Tensor:
    """-> the flat float32 ``x`` sorted ascending (a stable radix sort in the HIP library): -0 before +0, every NaN last and returned
    as the canonical quiet NaN; without NaN and -0 equal to ``torch.sort(x).values`` bit for bit.  ``x`` is not written."""
    x = _typed(x, 'x', (torch.float32,))
    n = _flat(x, 'x')
    out = torch.empty_like(x)
    if n == 0:
        return out
    ws = _sort_workspace(x.device, int(_lib.load().snerf_sort_workspace_bytes(n, 32)))
    _enqueue('snerf_sort_f32', x.device, _ptr(x), n, _ptr(out), _ptr(ws))
    return out


def sort_keys_with_order(keys: Tensor, key_bits: Optional[int] = None):
    """-> (sorted_keys int32, order int64) of the flat non-negative int32 ``keys``: the STABLE ascending sort, order equal to
    ``numpy.argsort(keys, kind='stable')`` -- what ``torch.sort(keys, stable=True)`` returns.  ``key_bits``: every key is below
    2 ** key_bits (1..32; a caller that knows the bound of its keys saves passes, one per 8 bits); None = 32.  ``keys`` is not
    written."""
    keys = _typed(keys, 'keys', (torch.int32,))
    n = _flat(keys, 'keys')
    key_bits = 32 if key_bits is None else key_bits
    if isinstance(key_bits, bool) or int(key_bits) != key_bits or not 1 <= int(key_bits) <= 32:
        raise RuntimeError(f'key_bits: expected 1..32, got {key_bits}')
    sorted_keys = torch.empty_like(keys)
    order = torch.empty((n,), dtype=torch.int64, device=keys.device)
    if n == 0:
        return sorted_keys, order
    ws = _sort_workspace(keys.device, int(_lib.load().snerf_sort_workspace_bytes(n, int(key_bits))))
    _enqueue('snerf_sort_keys_with_order', keys.device, _ptr(keys), n, int(key_bits), _ptr(sorted_keys), _ptr(order), _ptr(ws))
    return sorted_keys, order


def compact_pair(a: Tensor, b: Tensor, mask: Tensor):
    """-> (a[mask != 0], b[mask != 0]) of the flat float32 ``a``, ``b`` under the flat bool / uint8 ``mask``, in input order (count,
    scan, scatter in the HIP library).  The kept count is read back from the device once, to size the results."""
    a = _typed(a, 'a', (torch.float32,))
    n = _flat(a, 'a')
    b = _typed(b, 'b', (torch.float32,), (n,))
    mask = _typed(mask, 'mask', (torch.bool, torch.uint8), (n,))
    a_kept, b_kept = torch.empty_like(a), torch.empty_like(b)
    kept = torch.empty((1,), dtype=torch.int64, device=a.device)
    ws = _sort_workspace(a.device, int(_lib.load().snerf_compact_workspace_bytes(n)))
    _enqueue('snerf_compact_f32_pair', a.device, _ptr(a), _ptr(b), _ptr(mask), n, _ptr(a_kept), _ptr(b_kept), _ptr(kept), _ptr(ws))
    count = int(kept.item())
    return a_kept[:count], b_kept[:count]


# ---------------------------------------------------------------------------------------------- Q5 the Warper
WARP_U8, WARP_F32, WARP_F64 = C.SNERF_WARP_U8, C.SNERF_WARP_F32, C.SNERF_WARP_F64
_WARP_TYPES = {torch.uint8: WARP_U8, torch.float32: WARP_F32, torch.float64: WARP_F64}
WARP_MAX_CHANNELS = 4


def _warp_frame(frame, name: str, is_image: bool, extent=None):
    """A frame of the Warper: (h, w, c), c in 1..4, uint8 with ``is_image`` and float32 / float64 without.  -> (frame, h, w, c)."""
    frame = _typed(frame, name, (torch.uint8, torch.float32, torch.float64))
    if is_image and frame.dtype != torch.uint8:
        raise RuntimeError(f'{name}: is_image expects a uint8 frame (the result is rounded to uint8), got {frame.dtype}')
    if not is_image and frame.dtype == torch.uint8:
        raise RuntimeError(f'{name}: expected float32 or float64 without is_image, got {frame.dtype}')
    if frame.dim() != 3 or frame.numel() < 1:
        raise RuntimeError(f'{name}: expected a non-empty shape (h, w, c), got {tuple(frame.shape)}')
    h, w, c = (int(s) for s in frame.shape)
    if not 1 <= c <= WARP_MAX_CHANNELS:
        raise RuntimeError(f'{name}: expected 1..{WARP_MAX_CHANNELS} channels (h, w, c), got {c} in {tuple(frame.shape)}')
    if extent is not None and (h, w) != tuple(extent):
        raise RuntimeError(f'{name}: expected shape ({extent[0]}, {extent[1]}, c), got {tuple(frame.shape)}')
    _visibility_extent(1, h, w, name)
    return frame, h, w, c


def _warp_mask(mask, name: str, h: int, w: int):
    return None if mask is None else _typed(mask, name, (torch.bool, torch.uint8), (h, w))


def _warp_together(dev: torch.device, **operands) -> None:
    """Every operand of one call lives on the device the call is enqueued on: a pointer of another device is refused by name."""
    for name, t in operands.items():
        if t is not None and t.device != dev:
            raise RuntimeError(f'{name}: expected a tensor on {dev}, the device of the call\'s first operand, got one on {t.device}')


def _warp_workspace(dev: torch.device, h: int, w: int) -> Tensor:
    """The projection's scratch (per-workgroup maxima): on purpose the masks' buffer, kind 'visibility'."""
    return _workspace('visibility', dev, int(_lib.load().snerf_warp_workspace_bytes(h, w)))


def warp_project(depth1: Tensor, camera: Tensor, mask1: Optional[Tensor] = None):
    """``visibility_mask_project`` for ONE (h,w) float32 depth (``camera``: float64 (30) on the device, one row of its table), which
    also returns the flow and sends the sources ``mask1`` drops to the discard list.  -> points float64 (1,3,h,w), keys int32 (1,h,w),
    stats float64 (1,2), flow12 float64 (h,w,2): what ``visibility_mask_list_starts`` / ``warp_splat_gather`` take with views = 1."""
    depth1 = _typed(depth1, 'depth1', (torch.float32,))
    if depth1.dim() != 2:
        raise RuntimeError(f'depth1: expected shape (h, w), got {tuple(depth1.shape)}')
    h, w = (int(s) for s in depth1.shape)
    _visibility_extent(1, h, w, 'depth1')
    camera = _typed(camera, 'camera', (torch.float64,), (VISIBILITY_CAMERA,))
    mask1 = _warp_mask(mask1, 'mask1', h, w)
    dev = depth1.device
    _warp_together(dev, camera=camera, mask1=mask1)
    points = torch.empty((1, 3, h, w), dtype=torch.float64, device=dev)
    keys = torch.empty((1, h, w), dtype=torch.int32, device=dev)
    stats = torch.empty((1, 2), dtype=torch.float64, device=dev)
    flow12 = torch.empty((h, w, 2), dtype=torch.float64, device=dev)
    _enqueue('snerf_warp_project', dev, _ptr(depth1), _ptr(camera), _ptr(mask1), h, w, _ptr(points), _ptr(keys), _ptr(stats),
             _ptr(flow12), _ptr(_warp_workspace(dev, h, w)))
    return points, keys, stats, flow12


def warp_positions_from_flow(flow12: Tensor, depth1: Tensor, mask1: Optional[Tensor] = None, flow12_mask: Optional[Tensor] = None):
    """Padded positions ((flow_x + x) + 1, (flow_y + y) + 1) and Z = ``depth1`` of every source of a float64 (h,w,2) flow; ``depth1``
    float32 or float64 (h,w); a source either mask drops goes to the discard list.  -> points (1,3,h,w), keys (1,h,w), stats (1,2)."""
    flow12 = _typed(flow12, 'flow12', (torch.float64,))
    if flow12.dim() != 3 or flow12.shape[2] != 2:
        raise RuntimeError(f'flow12: expected shape (h, w, 2), got {tuple(flow12.shape)}')
    h, w = int(flow12.shape[0]), int(flow12.shape[1])
    _visibility_extent(1, h, w, 'flow12')
    depth1 = _typed(depth1, 'depth1', (torch.float32, torch.float64), (h, w))
    mask1 = _warp_mask(mask1, 'mask1', h, w)
    flow12_mask = _warp_mask(flow12_mask, 'flow12_mask', h, w)
    dev = flow12.device
    _warp_together(dev, depth1=depth1, mask1=mask1, flow12_mask=flow12_mask)
    points = torch.empty((1, 3, h, w), dtype=torch.float64, device=dev)
    keys = torch.empty((1, h, w), dtype=torch.int32, device=dev)
    stats = torch.empty((1, 2), dtype=torch.float64, device=dev)
    _enqueue('snerf_warp_positions_from_flow', dev, _ptr(flow12), _ptr(depth1), _WARP_TYPES[depth1.dtype], _ptr(mask1),
             _ptr(flow12_mask), h, w, _ptr(points), _ptr(keys), _ptr(stats), _ptr(_warp_workspace(dev, h, w)))
    return points, keys, stats


def warp_splat_gather(points: Tensor, order: Tensor, starts: Tensor, stats: Tensor, values: Tensor, is_image: bool = False):
    """Splat the (h,w,c) ``values`` (uint8 with ``is_image``, float32 / float64 without) of the sources of ``points`` (1,3,h,w) through
    the inverted index (``order``: the int64 permutation of the STABLE sort of the keys, ``starts``: visibility_mask_list_starts with
    views = 1).  -> (warped (h,w,c) uint8 / float64, mask2 bool (h,w))."""
    points = _typed(points, 'points', (torch.float64,))
    if points.dim() != 4 or points.shape[0] != 1 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected shape (1, 3, h, w), got {tuple(points.shape)}')
    h, w = int(points.shape[2]), int(points.shape[3])
    per_view = _visibility_extent(1, h, w, 'points')
    order = _typed(order, 'order', (torch.int64,), (h * w,))
    starts = _typed(starts, 'starts', (torch.int32,), (per_view + 1,))
    stats = _typed(stats, 'stats', (torch.float64,), (1, 2))
    values, _, _, c = _warp_frame(values, 'values', is_image, (h, w))
    dev = points.device
    _warp_together(dev, order=order, starts=starts, stats=stats, values=values)
    warped = torch.empty((h, w, c), dtype=torch.uint8 if is_image else torch.float64, device=dev)
    mask2 = torch.empty((h, w), dtype=torch.bool, device=dev)
    _enqueue('snerf_warp_splat_gather', dev, _ptr(points), _ptr(order), _ptr(starts), _ptr(stats), _ptr(values),
             _WARP_TYPES[values.dtype], c, int(bool(is_image)), h, w, _ptr(warped), _ptr(mask2))
    return warped, mask2


def warp_interpolate(frame2: Tensor, flow12: Tensor, mask2: Optional[Tensor] = None, flow12_mask: Optional[Tensor] = None,
                     is_image: bool = False):
    """The backward warp of the (h,w,c) ``frame2`` along the float64 (h,w,2) ``flow12``.  -> (warped (h,w,c) uint8 / float64, mask1 bool)."""
    frame2, h, w, c = _warp_frame(frame2, 'frame2', is_image)
    flow12 = _typed(flow12, 'flow12', (torch.float64,), (h, w, 2))
    mask2 = _warp_mask(mask2, 'mask2', h, w)
    flow12_mask = _warp_mask(flow12_mask, 'flow12_mask', h, w)
    dev = frame2.device
    _warp_together(dev, flow12=flow12, mask2=mask2, flow12_mask=flow12_mask)
    warped = torch.empty((h, w, c), dtype=torch.uint8 if is_image else torch.float64, device=dev)
    mask1 = torch.empty((h, w), dtype=torch.bool, device=dev)
    _enqueue('snerf_warp_interpolate', dev, _ptr(frame2), _WARP_TYPES[frame2.dtype], c, _ptr(mask2), _ptr(flow12),
             _ptr(flow12_mask), int(bool(is_image)), h, w, _ptr(warped), _ptr(mask1))
    return warped, mask1


# ---------------------------------------------------------------------------------------------- Q6 the point-cloud export
FUSE_CAMERA = C.SNERF_FUSE_CAMERA_DOUBLES     # doubles per view: inv(K) 3x3 | rows 0..2 of inv(E) 3x4 | rows 0..2 of E 3x4 | K 3x3
FUSE_MAX_VIEWS = C.SNERF_FUSE_MAX_VIEWS


def _fuse_workspace(dev: torch.device, need: int) -> Tensor:
    """Scratch of the two calls below (state bytes, keys, counters, the sort's buffers); 256-byte aligned like every torch allocation."""
    return _workspace('fuse', dev, max(need, 1))


def fuse_depth_maps(depth: Tensor, image: Tensor, cameras: Tensor, depth_error_threshold: float = 0.02, min_views: int = 1,
                    mask: Optional[Tensor] = None):
    """-> (points float32 (N,3), colours uint8 (N,3), views uint8 (N)) on the device: the pixels of the (V,h,w) float32 ``depth`` maps
    (colours: the uint8 (V,h,w,3) ``image``) whose depth is finite and positive, whose ``mask`` byte (bool / uint8 (V,h,w), optional)
    is set and whose point at least ``min_views`` of the OTHER views agree on to ``depth_error_threshold`` x their own depth at the
    pixel it projects to, in ascending (view, row, column) order; ``views`` counts the agreeing views (csrc/simplenerf_fuse.h has the
    rule).  ``cameras``: float64 (V,42) on the device (``geometry.fuse_cameras``).  The outputs are allocated for V h w records; N is
    read back from the device once, to narrow them."""
    depth = _typed(depth, 'depth', (torch.float32,))
    if depth.dim() != 3:
        raise RuntimeError(f'depth: expected shape (views, h, w), got {tuple(depth.shape)}')
    views, h, w = (int(s) for s in depth.shape)
    total = views * h * w
    if views > FUSE_MAX_VIEWS or total > SORT_MAX_COUNT:
        raise RuntimeError(f'depth: {views} views of {h} x {w} exceed {FUSE_MAX_VIEWS} views or the 2^31 - 1 pixels the kernels index')
    image = _typed(image, 'image', (torch.uint8,), (views, h, w, 3))
    cameras = _typed(cameras, 'cameras', (torch.float64,), (views, FUSE_CAMERA))
    if mask is not None:
        mask = _typed(mask, 'mask', (torch.bool, torch.uint8), (views, h, w))
    if not float(depth_error_threshold) >= 0.0:
        raise RuntimeError(f'depth_error_threshold: expected a non-negative number, got {depth_error_threshold}')
    if isinstance(min_views, bool) or int(min_views) != min_views or not 0 <= int(min_views) <= max(views - 1, 0):
        raise RuntimeError(f'min_views: expected 0..{max(views - 1, 0)} (the number of other views), got {min_views}')
    dev = depth.device
    _warp_together(dev, image=image, cameras=cameras, mask=mask)
    points = torch.empty((total, 3), dtype=torch.float32, device=dev)
    colours = torch.empty((total, 3), dtype=torch.uint8, device=dev)
    agreeing = torch.empty((total,), dtype=torch.uint8, device=dev)
    if total == 0:
        return points, colours, agreeing
    kept = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = _fuse_workspace(dev, int(_lib.load().snerf_fuse_depth_maps_workspace_bytes(views, h, w)))
    _enqueue('snerf_fuse_depth_maps', dev, _ptr(depth), _ptr(image), _ptr(mask), _ptr(cameras), views, h, w, float(depth_error_threshold),
             int(min_views), _ptr(points), _ptr(colours), _ptr(agreeing), _ptr(kept), _ptr(ws))
    count = int(kept.item())
    return points[:count], colours[:count], agreeing[:count]


def voxel_grid(points: Tensor, voxel_size: float):
    """-> (lo, extents): the per-axis minimum (three floats) of the float32 (N,3) ``points``, N >= 1, and the grid's extents in voxels,
    n_a = floor((max_a - lo_a) / voxel_size) + 1 in float64 -- one small reduction on the device and a copy of six floats.  Raises,
    naming ``voxel_size`` and the extents, when a bound is not finite or the grid has more than 2^31 - 1 voxels."""
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
        raise RuntimeError(f'voxel_size: expected a finite number > 0, got {voxel_size}')
    low, high = torch.aminmax(points, dim=0)
    bounds = torch.cat([low, high]).cpu().numpy().astype(numpy.float64)
    if not numpy.isfinite(bounds).all():
        raise RuntimeError(f'points: the bounds {bounds[:3].tolist()} .. {bounds[3:].tolist()} are not finite: no grid of voxel_size '
                           f'{voxel_size} and finite extents holds them')
    extents = tuple(int(math.floor((bounds[3 + a] - bounds[a]) / voxel_size)) + 1 for a in range(3))
    if extents[0] * extents[1] * extents[2] > 2 ** 31 - 1:
        raise RuntimeError(f'voxel_size: {voxel_size} gives extents {extents[0]} x {extents[1]} x {extents[2]}, more than the 2^31 - 1 '
                           f'voxels an int32 key numbers; choose a larger voxel_size')
    return tuple(float(v) for v in bounds[:3]), extents


def voxel_thin(points: Tensor, colours: Tensor, voxel_size: float, lo=None, extents=None):
    """-> (points float32 (M,3), colours uint8 (M,3), counts int32 (M)) on the device: one record per occupied voxel of the grid of
    ``voxel_size`` with corner ``lo`` and ``extents`` voxels (both from ``voxel_grid`` when not given), in ascending voxel order (z,
    then y, then x): the mean position (a sequential float64 sum in source order), the rounded mean colour and the number of the
    float32 (N,3) ``points`` / uint8 (N,3) ``colours`` in it (csrc/simplenerf_fuse.h has the rule).  M is read back once."""
    points = _typed(points, 'points', (torch.float32,))
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected shape (N, 3), got {tuple(points.shape)}')
    n = int(points.shape[0])
    if n > SORT_MAX_COUNT:
        raise RuntimeError(f'points: {n} points exceed the 2^31 - 1 the sort kernels index')
    colours = _typed(colours, 'colours', (torch.uint8,), (n, 3))
    dev = points.device
    _warp_together(dev, colours=colours)
    thinned, thinned_colours = torch.empty_like(points), torch.empty_like(colours)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        if not (float(voxel_size) > 0.0 and math.isfinite(float(voxel_size))):
            raise RuntimeError(f'voxel_size: expected a finite number > 0, got {voxel_size}')
        return thinned, thinned_colours, counts
    if lo is None or extents is None:
        lo, extents = voxel_grid(points, voxel_size)
    lo, extents = tuple(float(v) for v in lo), tuple(int(v) for v in extents)
    if len(lo) != 3 or len(extents) != 3:
        raise RuntimeError(f'lo, extents: expected three values each, got {lo} and {extents}')
    runs = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = _fuse_workspace(dev, int(_lib.load().snerf_voxel_thin_workspace_bytes(n, *extents)))
    _enqueue('snerf_voxel_thin', dev, _ptr(points), _ptr(colours), n, float(voxel_size), *lo, *extents, _ptr(thinned),
             _ptr(thinned_colours), _ptr(counts), _ptr(runs), _ptr(ws))
    count = int(runs.item())
    return thinned[:count], thinned_colours[:count], counts[:count]


# ---------------------------------------------------------------------------------------------- Q7 the mesh export
MESH_KEYS_PER_NODE = C.SNERF_MESH_KEYS_PER_NODE     # a grid may have 7 nx ny nz <= 2^31 - 1


def mesh_grid(lo, voxel_size, extents):
    """-> (lo (three floats), voxel_size, extents (nx, ny, nz)) of a volume, checked: ``voxel_size`` and ``lo`` finite, ``voxel_size``
    > 0, extents >= 1 and 7 nx ny nz <= 2^31 - 1 (csrc/simplenerf_mesh.h); refused by name otherwise."""
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
        raise RuntimeError(f'voxel_size: expected a finite number > 0, got {voxel_size}')
    lo = tuple(float(v) for v in lo)
    if len(lo) != 3 or not all(math.isfinite(v) for v in lo):
        raise RuntimeError(f'lo: expected three finite numbers, got {lo}')
    extents = tuple(extents)
    if len(extents) != 3 or any(isinstance(n, bool) or int(n) != n or int(n) < 1 for n in extents):
        raise RuntimeError(f'extents: expected three integers >= 1 (nx, ny, nz), got {extents}')
    extents = tuple(int(n) for n in extents)
    if MESH_KEYS_PER_NODE * extents[0] * extents[1] * extents[2] > SORT_MAX_COUNT:
        raise RuntimeError(f'extents: {extents[0]} x {extents[1]} x {extents[2]} nodes exceed the limit 7 nx ny nz <= 2^31 - 1 of the '
                           f'mesh kernels; choose a larger voxel_size or smaller bounds')
    return lo, voxel_size, extents


def _mesh_views(depth, cameras, mask, image=None):
    """The (V,h,w) float32 depth maps of a mesh call with their camera table, mask and frames, checked as ``fuse_depth_maps`` checks."""
    depth = _typed(depth, 'depth', (torch.float32,))
    if depth.dim() != 3:
        raise RuntimeError(f'depth: expected shape (views, h, w), got {tuple(depth.shape)}')
    views, h, w = (int(s) for s in depth.shape)
    if views > FUSE_MAX_VIEWS or views * h * w > SORT_MAX_COUNT:
        raise RuntimeError(f'depth: {views} views of {h} x {w} exceed {FUSE_MAX_VIEWS} views or the 2^31 - 1 pixels the kernels index')
    cameras = _typed(cameras, 'cameras', (torch.float64,), (views, FUSE_CAMERA))
    if mask is not None:
        mask = _typed(mask, 'mask', (torch.bool, torch.uint8), (views, h, w))
    if image is not None:
        image = _typed(image, 'image', (torch.uint8,), (views, h, w, 3))
    _warp_together(depth.device, cameras=cameras, mask=mask, image=image)
    return depth, cameras, mask, image, views, h, w


def tsdf_integrate(depth: Tensor, cameras: Tensor, lo, voxel_size: float, extents, truncation: float, mask: Optional[Tensor] = None):
    """-> (tsdf float32 (nz,ny,nx), weight uint8 (nz,ny,nx)) on the device: per node of the grid (node (i,j,k) at ``lo`` +
    ``voxel_size`` (i,j,k), ``extents`` = (nx,ny,nz)) the mean over the views that see it of min(1, (d - z) / ``truncation``), d the
    valid depth of the pixel the node projects to and z the node's depth in the view, where d - z >= -``truncation``; ``weight``
    counts those views, and tsdf is 1 where it is 0 (csrc/simplenerf_mesh.h has the rule).  ``depth`` float32 (V,h,w), ``cameras``
    float64 (V,42) (``geometry.fuse_cameras``), ``mask`` bool / uint8 (V,h,w), optional."""
    depth, cameras, mask, _, views, h, w = _mesh_views(depth, cameras, mask)
    lo, voxel_size, extents = mesh_grid(lo, voxel_size, extents)
    truncation = float(truncation)
    if not (truncation > 0.0 and math.isfinite(truncation)):
        raise RuntimeError(f'truncation: expected a finite number > 0, got {truncation}')
    dev = depth.device
    nx, ny, nz = extents
    tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    weight = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
    _enqueue('snerf_tsdf_integrate', dev, _ptr(depth), _ptr(mask), _ptr(cameras), views, h, w, voxel_size, *lo, nx, ny, nz, truncation,
             _ptr(tsdf), _ptr(weight))
    return tsdf, weight


def mesh_extract(tsdf: Tensor, weight: Tensor, lo, voxel_size: float, min_weight: int = 1):
    """-> (vertices float32 (Nv,3), triangles int32 (Nt,3)) on the device: the marching-tetrahedra surface tsdf = 0 of a float32
    (nz,ny,nx) ``tsdf`` volume over the cells whose eight nodes all have uint8 ``weight`` >= ``min_weight`` (1..255); vertices in
    ascending (node, edge type) order, triangles in ascending (cell, tetrahedron) order (csrc/simplenerf_mesh.h has the rule).
    Count, read the two counts back (the one synchronisation), allocate, emit."""
    tsdf = _typed(tsdf, 'tsdf', (torch.float32,))
    if tsdf.dim() != 3 or 0 in tsdf.shape:
        raise RuntimeError(f'tsdf: expected shape (nz, ny, nx), every extent >= 1, got {tuple(tsdf.shape)}')
    nz, ny, nx = (int(s) for s in tsdf.shape)
    weight = _typed(weight, 'weight', (torch.uint8,), (nz, ny, nx))
    lo, voxel_size, extents = mesh_grid(lo, voxel_size, (nx, ny, nz))
    if isinstance(min_weight, bool) or int(min_weight) != min_weight or not 1 <= int(min_weight) <= 255:
        raise RuntimeError(f'min_weight: expected 1..255, got {min_weight}')
    dev = tsdf.device
    _warp_together(dev, weight=weight)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    ws = _workspace('mesh', dev, max(int(_lib.load().snerf_mesh_workspace_bytes(nx, ny, nz)), 1))
    grid = (_ptr(tsdf), _ptr(weight), voxel_size, *lo, nx, ny, nz, int(min_weight), _ptr(counts))
    _enqueue('snerf_mesh_count', dev, *grid, _ptr(ws))
    num_vertices, num_triangles = (int(v) for v in counts.tolist())
    vertices = torch.empty((num_vertices, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((num_triangles, 3), dtype=torch.int32, device=dev)
    if num_vertices > 0 and num_triangles > 0:
        _enqueue('snerf_mesh_emit', dev, *grid, _ptr(vertices), _ptr(triangles), _ptr(ws))
    return vertices, triangles


def colour_points(points: Tensor, depth: Tensor, image: Tensor, cameras: Tensor, colour_tolerance: float, mask: Optional[Tensor] = None):
    """-> (colours uint8 (N,3), views uint8 (N)) on the device: per float32 (N,3) point the rounded mean of the pixels it projects to
    in the views that agree with it -- the pixel is valid and its depth within ``colour_tolerance`` (scene units) of the point's depth
    in that view -- and the number of those views; (0,0,0) where none agrees (csrc/simplenerf_mesh.h has the rule).  ``depth``,
    ``image``, ``cameras``, ``mask`` as ``fuse_depth_maps`` takes them."""
    points = _typed(points, 'points', (torch.float32,))
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected shape (N, 3), got {tuple(points.shape)}')
    n = int(points.shape[0])
    if n > SORT_MAX_COUNT:
        raise RuntimeError(f'points: {n} points exceed the 2^31 - 1 the kernels index')
    depth, cameras, mask, image, views, h, w = _mesh_views(depth, cameras, mask, _typed(image, 'image', (torch.uint8,)))
    if not float(colour_tolerance) >= 0.0:
        raise RuntimeError(f'colour_tolerance: expected a non-negative number, got {colour_tolerance}')
    dev = points.device
    _warp_together(dev, depth=depth)
    colours = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    agreeing = torch.empty((n,), dtype=torch.uint8, device=dev)
    if n > 0:
        _enqueue('snerf_colour_points', dev, _ptr(points), n, _ptr(depth), _ptr(image), _ptr(mask), _ptr(cameras), views, h, w,
                 float(colour_tolerance), _ptr(colours), _ptr(agreeing))
    return colours, agreeing


# ---------------------------------------------------------------------------------------------- Q8 the field export
FIELD_NO_VIEW = C.SNERF_FIELD_NO_VIEW     # the view byte of a point that no view sees


def _field_views(cameras, resolution, ndc, least: int):
    """The camera table, frame size and input map of a field call, checked -> (cameras, views, h, w, (flag, cx, cy, near))."""
    cameras = _typed(cameras, 'cameras', (torch.float64,))
    if cameras.dim() != 2 or cameras.shape[1] != FUSE_CAMERA:
        raise RuntimeError(f'cameras: expected shape (views, {FUSE_CAMERA}), got {tuple(cameras.shape)}')
    views = int(cameras.shape[0])
    if not least <= views <= FUSE_MAX_VIEWS:
        raise RuntimeError(f'cameras: {views} views, expected {least}..{FUSE_MAX_VIEWS}')
    resolution = tuple(resolution)
    if len(resolution) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 0 for v in resolution):
        raise RuntimeError(f'resolution: expected two integers >= 0 (height, width), got {resolution}')
    if ndc is None:
        return cameras, views, int(resolution[0]), int(resolution[1]), (0, 0.0, 0.0, 0.0)
    ndc = tuple(float(v) for v in ndc)
    if len(ndc) != 3 or not all(math.isfinite(v) for v in ndc) or not ndc[2] > 0.0:
        raise RuntimeError(f'ndc: expected None or three finite numbers (cx, cy, near) with near > 0, got {ndc}')
    return cameras, views, int(resolution[0]), int(resolution[1]), (1,) + ndc


def field_grid_points(lo, voxel_size: float, extents, cameras: Tensor, resolution, ndc=None, first_node: int = 0,
                      count: Optional[int] = None):
    """-> (mlp_points float32 (count,3), weight uint8 (count)) on the device: for the nodes ``first_node`` .. ``first_node`` + ``count``
    - 1 of the grid (node (i,j,k), index (k ny + j) nx + i, at ``lo`` + ``voxel_size`` (i,j,k); ``extents`` = (nx,ny,nz); ``count``
    defaults to the rest of the grid) the point the model's MLP reads and the number of views that see the node: it lies in front
    of the view and projects (nearest pixel, ties to even) inside the (height, width) = ``resolution`` frame
    (csrc/simplenerf_field.h has the rules).  ``ndc``: None for a model of world-space rays (the point is the node), or (cx, cy,
    near) for a model of NDC rays (``geometry.ndc_parameters``): nodes nearer than the near plane get (0,0,0) and weight 0.
    ``cameras``: float64 (V,42) on the device (``geometry.fuse_cameras``), V >= 0."""
    lo, voxel_size, extents = mesh_grid(lo, voxel_size, extents)
    cameras, views, h, w, ndc = _field_views(cameras, resolution, ndc, 0)
    nodes = extents[0] * extents[1] * extents[2]
    if isinstance(first_node, bool) or int(first_node) != first_node or not 0 <= int(first_node) <= nodes:
        raise RuntimeError(f'first_node: expected 0..{nodes}, got {first_node}')
    first_node = int(first_node)
    if count is None:
        count = nodes - first_node
    if isinstance(count, bool) or int(count) != count or not 0 <= int(count) <= nodes - first_node:
        raise RuntimeError(f'count: expected 0..{nodes - first_node} (the nodes from first_node on), got {count}')
    count = int(count)
    dev = cameras.device
    points = torch.empty((count, 3), dtype=torch.float32, device=dev)
    weight = torch.empty((count,), dtype=torch.uint8, device=dev)
    if count > 0:
        _enqueue('snerf_field_grid_points', dev, voxel_size, *lo, *extents, first_node, count, _ptr(cameras if views else None), views, h, w,
                 *ndc, _ptr(points), _ptr(weight))
    return points, weight


def field_point_views(points: Tensor, cameras: Tensor, resolution, ndc=None):
    """-> (mlp_points float32 (N,3), view_dirs float32 (N,3), view uint8 (N)) on the device: per float32 (N,3) scene-frame point the
    point the model's MLP reads, the unit direction (scene frame) from the centre of the view that sees it from the smallest depth
    (the lowest index among equal ones) and that view's index; where no view sees the point, view 0's direction and
    ``FIELD_NO_VIEW`` (csrc/simplenerf_field.h has the rules).  ``cameras``, ``resolution``, ``ndc`` as ``field_grid_points`` takes
    them, V >= 1."""
    points = _typed(points, 'points', (torch.float32,))
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected shape (N, 3), got {tuple(points.shape)}')
    n = int(points.shape[0])
    if n > SORT_MAX_COUNT:
        raise RuntimeError(f'points: {n} points exceed the 2^31 - 1 the kernels index')
    cameras, views, h, w, ndc = _field_views(cameras, resolution, ndc, 1)
    dev = points.device
    _warp_together(dev, cameras=cameras)
    mlp_points, view_dirs = torch.empty_like(points), torch.empty_like(points)
    view = torch.empty((n,), dtype=torch.uint8, device=dev)
    if n > 0:
        _enqueue('snerf_field_point_views', dev, _ptr(points), n, _ptr(cameras), views, h, w, *ndc, _ptr(mlp_points), _ptr(view_dirs),
                 _ptr(view))
    return mlp_points, view_dirs, view


def field_values(sigma: Tensor, weight: Tensor, level: float) -> Tensor:
    """-> tsdf float32, shaped like ``sigma``, on the device: min(1, max(-1, (``level`` - sigma) / ``level``)) in float64 per element
    of the float32 ``sigma``, and 1 where the uint8 ``weight`` (same shape) is 0 or sigma is a NaN -- the signed volume
    ``mesh_extract`` takes, negative on the dense side (csrc/simplenerf_field.h has the rule).  ``level``: a finite number > 0."""
    sigma = _typed(sigma, 'sigma', (torch.float32,))
    weight = _typed(weight, 'weight', (torch.uint8,), tuple(sigma.shape))
    level = float(level)
    if not (level > 0.0 and math.isfinite(level)):
        raise RuntimeError(f'level: expected a finite number > 0, got {level}')
    n = int(sigma.numel())
    if n > SORT_MAX_COUNT:
        raise RuntimeError(f'sigma: {n} elements exceed the 2^31 - 1 the kernels index')
    dev = sigma.device
    _warp_together(dev, weight=weight)
    tsdf = torch.empty_like(sigma)
    if n > 0:
        _enqueue('snerf_field_values', dev, _ptr(sigma), _ptr(weight), n, level, _ptr(tsdf))
    return tsdf


def field_normals(points: Tensor, grad: Tensor, ndc=None) -> Tensor:
    """-> float32 (N,3) on the device: the unit outward normal of the density field at every float32 (N,3) scene-frame point, from
    the float32 (N,3) gradient ``grad`` of the density in the space the model's MLP reads (``PackedMlp.input_gradient``,
    ``model.query_gradient``): the gradient is pulled back through the input map (``ndc`` = None: the identity; (cx, cy, near): the
    transposed Jacobian of the NDC warp), negated -- the density's low side is outside -- and normalised, in float64
    (csrc/simplenerf_gradient.h has the rule).  (0, 0, 0) where the gradient is zero or not finite, or the point is nearer than
    the near plane."""
    points = _typed(points, 'points', (torch.float32,))
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points: expected shape (N, 3), got {tuple(points.shape)}')
    n = int(points.shape[0])
    grad = _typed(grad, 'grad', (torch.float32,), (n, 3))
    if n > SORT_MAX_COUNT:
        raise RuntimeError(f'points: {n} points exceed the 2^31 - 1 the kernels index')
    flag = (0, 0.0, 0.0, 0.0)
    if ndc is not None:
        ndc = tuple(float(v) for v in ndc)
        if len(ndc) != 3 or not all(math.isfinite(v) for v in ndc) or not ndc[2] > 0.0:
            raise RuntimeError(f'ndc: expected None or three finite numbers (cx, cy, near) with near > 0, got {ndc}')
        flag = (1,) + ndc
    dev = points.device
    _warp_together(dev, grad=grad)
    normals = torch.empty_like(points)
    if n > 0:
        _enqueue('snerf_field_normals', dev, _ptr(points), _ptr(grad), n, *flag, _ptr(normals))
    return normals


# ---------------------------------------------------------------------------------------------- Q10 normal maps
def _ndc_flag(ndc) -> tuple:
    """(0, 0, 0, 0) or (1, cx, cy, near): THE INPUT MAP's arguments of a C call, checked as ``field_normals`` checks them."""
    if ndc is None:
        return (0, 0.0, 0.0, 0.0)
    ndc = tuple(float(v) for v in ndc)
    if len(ndc) != 3 or not all(math.isfinite(v) for v in ndc) or not ndc[2] > 0.0:
        raise RuntimeError(f'ndc: expected None or three finite numbers (cx, cy, near) with near > 0, got {ndc}')
    return (1,) + ndc


def _ray_samples(weights, min_weight):
    weights = _typed(weights, 'weights', (torch.float32,))
    if weights.dim() != 2:
        raise RuntimeError(f'weights: expected shape (rays, samples), got {tuple(weights.shape)}')
    rays, samples = (int(s) for s in weights.shape)
    if rays * samples > SORT_MAX_COUNT:
        raise RuntimeError(f'weights: {rays} rays of {samples} samples exceed the 2^31 - 1 samples the kernels index')
    min_weight = float(min_weight)
    if math.isnan(min_weight):
        raise RuntimeError('min_weight: expected a number, got nan')
    return weights, rays, samples, min_weight


def select_ray_samples(rays_o: Tensor, rays_d: Tensor, z_vals: Tensor, weights: Tensor, min_weight: float = 0.0):
    """-> (offsets int32 (R+1), sample int32 (M), points float32 (M,3)) on the device: the samples of a render whose float32 (R,S)
    ``weights`` exceed ``min_weight`` (a NaN weight is not selected), in ascending flat index r S + i (``sample``), with the points
    ``rays_o`` + ``rays_d`` x ``z_vals`` evaluated in float32 exactly as the render kernels evaluate them -- the points the MLP saw;
    ``offsets`` is the exclusive prefix of the per-ray counts, ``offsets[R]`` = M (csrc/simplenerf_normals.h has the rule).
    ``rays_o``, ``rays_d`` float32 (R,3), ``z_vals`` float32 (R,S): the rays the render marched, the NDC rays and depths of an NDC
    render.  Count, read M back (the one synchronisation), allocate, emit."""
    weights, rays, samples, min_weight = _ray_samples(weights, min_weight)
    rays_o = _typed(rays_o, 'rays_o', (torch.float32,), (rays, 3))
    rays_d = _typed(rays_d, 'rays_d', (torch.float32,), (rays, 3))
    z_vals = _typed(z_vals, 'z_vals', (torch.float32,), (rays, samples))
    dev = weights.device
    _warp_together(dev, rays_o=rays_o, rays_d=rays_d, z_vals=z_vals)
    offsets = torch.empty((rays + 1,), dtype=torch.int32, device=dev)
    _enqueue('snerf_ray_samples_count', dev, _ptr(weights), rays, samples, min_weight, _ptr(offsets))
    count = int(offsets[rays].item())
    sample = torch.empty((count,), dtype=torch.int32, device=dev)
    points = torch.empty((count, 3), dtype=torch.float32, device=dev)
    if count > 0:
        _enqueue('snerf_ray_samples_emit', dev, _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), _ptr(weights), rays, samples, min_weight,
                 _ptr(offsets), count, _ptr(sample), _ptr(points))
    return offsets, sample, points


def composite_normals(points: Tensor, grad: Tensor, offsets: Tensor, sample: Tensor, weights: Tensor, ndc=None):
    """-> (normal float32 (R,3), strength float32 (R)) on the device: per ray the weighted sum, over its selected samples
    (``offsets``, ``sample``, ``points`` of ``select_ray_samples``), of the field's unit normals -G / |G| there, G the float32 (M,3)
    gradient ``grad`` of the density at the points (``model.query_gradient``) pulled back through the input map (``ndc`` = None: the
    identity; (cx, cy, near): the NDC warp, inverted to find the scene point); ``strength`` is the sum's length, ``normal`` the sum
    over it, and both are 0 where it is 0 or not finite.  Sequential float64 sums in sample order (csrc/simplenerf_normals.h has the
    rule).  ``weights`` float32 (R,S): the render's."""
    weights, rays, samples, _ = _ray_samples(weights, 0.0)
    offsets = _typed(offsets, 'offsets', (torch.int32,), (rays + 1,))
    sample = _typed(sample, 'sample', (torch.int32,))
    if sample.dim() != 1:
        raise RuntimeError(f'sample: expected shape (M,), got {tuple(sample.shape)}')
    count = int(sample.shape[0])
    points = _typed(points, 'points', (torch.float32,), (count, 3))
    grad = _typed(grad, 'grad', (torch.float32,), (count, 3))
    flag = _ndc_flag(ndc)
    dev = weights.device
    _warp_together(dev, points=points, grad=grad, offsets=offsets, sample=sample)
    normal = torch.empty((rays, 3), dtype=torch.float32, device=dev)
    strength = torch.empty((rays,), dtype=torch.float32, device=dev)
    if rays > 0:
        _enqueue('snerf_composite_normals', dev, _ptr(points), _ptr(grad), count, _ptr(offsets), _ptr(sample), _ptr(weights), rays, samples,
                 *flag, _ptr(normal), _ptr(strength))
    return normal, strength


def depth_normals(depth: Tensor, cameras: Tensor, mask: Optional[Tensor] = None, edge_threshold: Optional[float] = None) -> Tensor:
    """-> float32 (V,h,w,3) on the device: the unit normals of the float32 (V,h,w) ``depth`` maps in the scene frame, facing their
    cameras: the cross product of a pixel's horizontal and vertical tangents, each the difference of the neighbouring pixels' points
    (``fuse_depth_maps``' own points; central where both neighbours are usable, one-sided with one).  A pixel is valid as in the fuse
    (finite positive depth, ``mask`` set); a neighbour is usable when it is valid and, with ``edge_threshold``, its depth differs
    from the pixel's by at most ``edge_threshold`` x the pixel's.  (0, 0, 0) for an invalid pixel, a missing tangent or a degenerate
    cross product (csrc/simplenerf_normals.h has the rule).  ``cameras``: float64 (V,42) (``geometry.fuse_cameras``)."""
    depth, cameras, mask, _, views, h, w = _mesh_views(depth, cameras, mask)
    edge = -1.0 if edge_threshold is None else float(edge_threshold)
    if edge_threshold is not None and not edge >= 0.0:
        raise RuntimeError(f'edge_threshold: expected None or a non-negative number, got {edge_threshold}')
    dev = depth.device
    normals = torch.empty((views, h, w, 3), dtype=torch.float32, device=dev)
    if views * h * w > 0:
        _enqueue('snerf_depth_normals', dev, _ptr(depth), _ptr(mask), _ptr(cameras), views, h, w, edge, _ptr(normals))
    return normals


def normals_to_u8(normals: Tensor, rotation=None) -> Tensor:
    """-> uint8, the shape of ``normals``: float32 (...,3) unit normals as a picture, min(255, max(0, floor(127.5 (c + 1) + 0.5)))
    of c = R^T n for the 3x3 ``rotation`` R (a camera-to-world rotation: the picture is in the camera's frame; None: the identity).
    A zero normal is (128, 128, 128), a NaN 0 (csrc/simplenerf_normals.h has the rule)."""
    normals = _typed(normals, 'normals', (torch.float32,))
    if normals.dim() < 1 or normals.shape[-1] != 3:
        raise RuntimeError(f'normals: expected shape (..., 3), got {tuple(normals.shape)}')
    count = normals.numel() // 3
    if count > SORT_MAX_COUNT:
        raise RuntimeError(f'normals: {count} normals exceed the 2^31 - 1 the kernels index')
    table = None
    if rotation is not None:
        matrix = numpy.asarray(rotation.detach().cpu().numpy() if isinstance(rotation, torch.Tensor) else rotation, dtype=numpy.float64)
        if matrix.shape != (3, 3) or not numpy.isfinite(matrix).all():
            raise RuntimeError(f'rotation: expected None or a finite 3x3 matrix, got shape {matrix.shape}')
        table = (ctypes.c_double * 9)(*matrix.reshape(-1).tolist())
    image = torch.empty(normals.shape, dtype=torch.uint8, device=normals.device)
    if count > 0:
        _enqueue('snerf_normals_to_u8', normals.device, _ptr(normals), count, table, _ptr(image))
    return image


# ---------------------------------------------------------------------------------------------- f1 losses
class LossTermSpec:
    """One masked mean-squared-error term of the fused loss evaluation (struct snerf_loss_term).  ``two_sided``: the
    backward may also be asked for the gradient of ``target`` (the exact negation of ``pred``'s); the value is that of
    the one-sided term."""
    __slots__ = ('pred', 'target', 'numerator_mask', 'denominator_mask', 'group', 'weight', 'two_sided')

    def __init__(self, pred: Tensor, target: Tensor, numerator_mask: Optional[Tensor], denominator_mask: Optional[Tensor],
                 group: int, weight: float, two_sided: bool = False):
        self.two_sided = bool(two_sided)
        n = pred.shape[0]
        self.pred = _dev(pred, 'loss pred')
        self.target = _dev(target, 'loss target', tuple(pred.shape))
        self.numerator_mask = _mask(numerator_mask, 'numerator_mask', n)
        self.denominator_mask = _mask(denominator_mask, 'denominator_mask', n)
        self.group, self.weight = int(group), float(weight)
        if self.pred.dim() not in (1, 2) or (self.pred.dim() == 2 and self.pred.shape[1] > 4):
            raise RuntimeError(f'loss pred: expected (n,) or (n,c<=4), got {tuple(pred.shape)}')


def _mask(t: Optional[Tensor], name: str, n: int) -> Optional[Tensor]:
    if t is None:
        return None
    if not t.is_cuda or t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != (n,):
        raise RuntimeError(f'{name}: expected a bool/uint8 GPU tensor of shape ({n},), got {t.dtype} {tuple(t.shape)} on {t.device}')
    return t.contiguous()


def _loss_table(terms: List[LossTermSpec], grads: Optional[List[Optional[Tensor]]],
                target_grads: Optional[List[Optional[Tensor]]] = None):
    if not 1 <= len(terms) <= _lib.LOSS_MAX_TERMS:
        raise RuntimeError(f'fused loss: {len(terms)} terms, the kernel table holds 1..{_lib.LOSS_MAX_TERMS}')
    table = (_lib.LossTerm * len(terms))()
    seen = set()
    for i, t in enumerate(terms):
        e = table[i]
        e.pred, e.target = t.pred.data_ptr(), t.target.data_ptr()
        e.numerator_mask = 0 if t.numerator_mask is None else t.numerator_mask.data_ptr()
        e.denominator_mask = 0 if t.denominator_mask is None else t.denominator_mask.data_ptr()
        e.channels = 1 if t.pred.dim() == 1 else t.pred.shape[1]
        e.group, e.weight = t.group, t.weight
        e.d_pred, e.accumulate, e.d_target, e.accumulate_target = 0, 0, 0, 0
        if grads is not None and grads[i] is not None:
            e.d_pred = grads[i].data_ptr()
            e.accumulate = int(e.d_pred in seen)
            seen.add(e.d_pred)
        if target_grads is not None and target_grads[i] is not None:
            e.d_target = target_grads[i].data_ptr()
            e.accumulate_target = int(e.d_target in seen)
            seen.add(e.d_target)
    return table


def loss_forward(terms: List[LossTermSpec], num_groups: int):
    """-> values (T+G+1: term values, per-loss sums, weighted total), scales (T) for loss_backward.  One launch."""
    lib = _lib.load()
    dev = terms[0].pred.device
    n, count = terms[0].pred.shape[0], len(terms)
    if any(t.pred.shape[0] != n for t in terms):
        raise RuntimeError('fused loss: every term must cover the same rays')
    values = torch.empty((count + num_groups + 1,), dtype=torch.float32, device=dev)
    scales = torch.empty((count,), dtype=torch.float32, device=dev)
    # block partials + a completion counter that must be zero on first use (the kernel leaves it zero again); callers that
    # evaluate losses on several streams of one device at once need one buffer each
    ws = _workspace('loss', dev, int(lib.snerf_loss_workspace_bytes()), zeroed=True)
    with torch.cuda.device(dev):
        st = lib.snerf_loss_forward(_loss_table(terms, None), count, int(num_groups), n, _ptr(values), _ptr(scales),
                                    ctypes.c_void_p(ws.data_ptr()), _stream())
    _lib.check(st, 'snerf_loss_forward')
    return values, scales


def loss_backward(terms: List[LossTermSpec], num_groups: int, scales: Tensor, upstream: Tensor,
                  wanted: List[bool], wanted_target: Optional[List[bool]] = None):
    """Gradient of every term's pred (None where ``wanted[i]`` is false).  Terms that share a tensor share one buffer
    holding the sum.  One launch.  ``wanted_target`` (two-sided terms only): also the gradient of those terms' targets;
    the result is then the pair (pred gradients, target gradients), and a tensor that is pred of one term and target of
    another has ONE buffer, in both lists, holding the sum over both roles."""
    lib = _lib.load()
    n = terms[0].pred.shape[0]
    buffers: Dict[int, Tensor] = {}

    def buffer_of(t: Tensor) -> Tensor:
        key = t.data_ptr()
        if key not in buffers:
            buffers[key] = torch.empty_like(t)
        return buffers[key]

    grads: List[Optional[Tensor]] = [buffer_of(t.pred) if want else None for t, want in zip(terms, wanted)]
    target_grads: Optional[List[Optional[Tensor]]] = None
    if wanted_target is not None:
        for t, want in zip(terms, wanted_target):
            if want and not t.two_sided:
                raise RuntimeError('fused loss: the gradient of a target was asked of a term that is not two_sided')
        target_grads = [buffer_of(t.target) if want else None for t, want in zip(terms, wanted_target)]
    upstream = _dev(upstream, 'upstream', (len(terms) + num_groups + 1,))
    if n > 0 and buffers:
        with torch.cuda.device(scales.device):
            st = lib.snerf_loss_backward(_loss_table(terms, grads, target_grads), len(terms), int(num_groups), n,
                                         _ptr(scales), _ptr(upstream), _stream())
        _lib.check(st, 'snerf_loss_backward')
    return grads if wanted_target is None else (grads, target_grads)


def patch_consistency_masks(rays_o: Tensor, rays_d: Tensor, depth1: Tensor, depth2: Tensor, ray_mask: Optional[Tensor],
                            pixel_id: Tensor, poses: Tensor, intrinsic: Tensor, images: Tensor, patch_size,
                            rmse_threshold: float, with_rmse: bool = False):
    """Decision masks of the patch-reprojection consistency losses: (mask1, mask2[, rmse1, rmse2]) per ray."""
    n = rays_o.shape[0]
    v, h, w, c = images.shape
    if c != 3:
        raise RuntimeError(f'images: expected (views,h,w,3), got {tuple(images.shape)}')
    rays_o, rays_d = _dev(rays_o, 'rays_o', (n, 3)), _dev(rays_d, 'rays_d', (n, 3))
    depth1, depth2 = _dev(depth1, 'depth1', (n,)), _dev(depth2, 'depth2', (n,))
    ray_mask = _mask(ray_mask, 'ray_mask', n)
    if not pixel_id.is_cuda or pixel_id.dtype != torch.int32 or tuple(pixel_id.shape) != (n, 3):
        raise RuntimeError(f'pixel_id: expected int32 GPU tensor ({n},3), got {pixel_id.dtype} {tuple(pixel_id.shape)}')
    pixel_id = pixel_id.contiguous()
    poses, images = _dev(poses, 'poses', (v, 4, 4)), _dev(images, 'images')
    intrinsic = _dev(intrinsic, 'intrinsic', (3, 3))
    dev = rays_o.device
    mask1 = torch.empty((n,), dtype=torch.bool, device=dev)
    mask2 = torch.empty((n,), dtype=torch.bool, device=dev)
    rmse1 = torch.empty((n,), dtype=torch.float32, device=dev) if with_rmse else None
    rmse2 = torch.empty((n,), dtype=torch.float32, device=dev) if with_rmse else None
    if n > 0:
        lib = _lib.load()
        with torch.cuda.device(dev):      # (inline, not _enqueue: three times per training iteration)
            st = lib.snerf_patch_consistency_masks(
                _ptr(rays_o), _ptr(rays_d), _ptr(depth1), _ptr(depth2), _ptr(ray_mask), _ptr(pixel_id), n, _ptr(poses),
                _ptr(intrinsic), _ptr(images), v, h, w, int(patch_size[0]), int(patch_size[1]), float(rmse_threshold),
                _ptr(mask1), _ptr(mask2), _ptr(rmse1), _ptr(rmse2), _stream())
        _lib.check(st, 'snerf_patch_consistency_masks')
    return (mask1, mask2, rmse1, rmse2) if with_rmse else (mask1, mask2)


# ---------------------------------------------------------------------------------------------- f4 optimiser
def adam_step(params: List[Tensor], grads: List[Optional[Tensor]], exp_avg: List[Tensor], exp_avg_sq: List[Tensor],
              step: int, lr: float, beta1: float, beta2: float, eps: float, at: Optional[Tensor] = None) -> None:
    """In-place Adam update of every tensor with a gradient (one launch per 64 tensors).  ``at``: the device-resident
    iteration record (``IterationRing.current``) to take the step-dependent factors from instead of ``step`` / ``lr``."""
    lib = _lib.load()
    n = len(params)
    if n == 0:
        return
    f32 = torch.float32
    for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
        for name, t in (('param', p), ('exp_avg', m), ('exp_avg_sq', v)):
            if not t.is_cuda or t.dtype != f32 or not t.is_contiguous():
                raise RuntimeError(f'adam_step: {name} must be a contiguous float32 GPU tensor, got {t.dtype} on {t.device}')
        if g is not None and (not g.is_cuda or g.dtype != f32 or g.shape != p.shape):
            raise RuntimeError(f'adam_step: grad must be a float32 GPU tensor shaped like its parameter, got {g.dtype} '
                               f'{tuple(g.shape)} on {g.device}')
    grads = [None if g is None else (g if g.is_contiguous() else g.contiguous()) for g in grads]
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    sizes = (ctypes.c_longlong * n)(*[p.numel() for p in params])
    with torch.cuda.device(params[0].device):
        if at is not None:
            st = lib.snerf_adam_step_at(ptrs(params), ptrs(grads), ptrs(exp_avg), ptrs(exp_avg_sq), sizes, n,
                                        ctypes.c_void_p(at.data_ptr()), float(beta1), float(beta2), float(eps), _stream())
        else:
            st = lib.snerf_adam_step(ptrs(params), ptrs(grads), ptrs(exp_avg), ptrs(exp_avg_sq), sizes, n, int(step),
                                     float(lr), float(beta1), float(beta2), float(eps), _stream())
    _lib.check(st, 'snerf_adam_step')


# ---------------------------------------------------------------------------------------------- f2 batch assembly
def camera_table(intrinsics: Tensor, poses: Tensor, resolution) -> Tensor:
    """(V, 24) per-view camera constants (inverse intrinsic, rotation, origin, NDC factors) on the device."""
    v = poses.shape[0]
    intrinsics, poses = _dev(intrinsics, 'intrinsics', (v, 3, 3)), _dev(poses, 'poses', (v, 4, 4))
    table = torch.empty((v, _lib.CAMERA_FLOATS), dtype=torch.float32, device=poses.device)
    _enqueue('snerf_camera_table', poses.device, _ptr(intrinsics), _ptr(poses), v, int(resolution[0]), int(resolution[1]),
             _ptr(table))
    return table


def assemble_batch(indices: Tensor, num_pixel_rays: int, table: Tensor, resolution, images: Tensor, ndc: bool, near: float,
                   far: float, near_ndc: float = 0.0, far_ndc: float = 1.0, sparse_depths: Optional[Tensor] = None,
                   sparse_errors: Optional[Tensor] = None, sparse_depths_ndc: Optional[Tensor] = None,
                   with_sparse_mask: bool = False, first_pixel_row: int = 0, first_sparse_row: Optional[int] = None
                   ) -> Dict[str, Tensor]:
    """One launch: rays (+NDC), view_dirs, pixel_id, target_rgb, near/far columns, sparse-depth columns and the row
    masks for the global pixel ``indices`` (int64 GPU tensor); the first ``num_pixel_rays`` rows are pixel rays.
    ``global_rows`` (int64, (n,)) numbers the rows as the single-process batch would: ``first_pixel_row + i`` for pixel
    rows, ``first_sparse_row + j`` for sparse rows (default: right behind this call's pixel rows)."""
    lib = _lib.load()
    if not indices.is_cuda or indices.dtype != torch.int64 or indices.dim() != 1:
        raise RuntimeError(f'indices: expected a 1-D int64 GPU tensor, got {indices.dtype} {tuple(indices.shape)} on {indices.device}')
    indices = indices.contiguous()
    n, dev = indices.shape[0], indices.device
    h, w = int(resolution[0]), int(resolution[1])
    v = table.shape[0]
    table = _dev(table, 'camera table', (v, _lib.CAMERA_FLOATS))
    images = _dev(images, 'images', (v, h, w, 3))
    tables = [None if t is None else _dev(t.reshape(-1), name, (v * h * w,)) for t, name in
              ((sparse_depths, 'sparse_depths'), (sparse_errors, 'sparse_errors'), (sparse_depths_ndc, 'sparse_depths_ndc'))]
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {'rays_o': f(n, 3), 'rays_d': f(n, 3), 'view_dirs': f(n, 3),
           'pixel_id': torch.empty((n, 3), dtype=torch.int32, device=dev), 'target_rgb': f(n, 3), 'near': f(n, 1), 'far': f(n, 1),
           'indices_mask_nerf': torch.empty((n,), dtype=torch.bool, device=dev),
           'global_rows': torch.empty((n,), dtype=torch.int64, device=dev)}
    if ndc:
        out.update(rays_o_ndc=f(n, 3), rays_d_ndc=f(n, 3), near_ndc=f(n, 1), far_ndc=f(n, 1))
    for key, t in zip(('sparse_depth_values', 'sparse_depth_errors', 'sparse_depth_values_ndc'), tables):
        if t is not None:
            out[key] = f(n, 1)
    if with_sparse_mask:
        out['indices_mask_sparse_depth'] = torch.empty((n,), dtype=torch.bool, device=dev)
    if n == 0:
        return out
    b = _lib.Batch()
    for field, key in (('rays_o', 'rays_o'), ('rays_d', 'rays_d'), ('view_dirs', 'view_dirs'), ('rays_o_ndc', 'rays_o_ndc'),
                       ('rays_d_ndc', 'rays_d_ndc'), ('pixel_id', 'pixel_id'), ('target_rgb', 'target_rgb'), ('near', 'near'),
                       ('far', 'far'), ('near_ndc', 'near_ndc'), ('far_ndc', 'far_ndc'),
                       ('sparse_depth_values', 'sparse_depth_values'), ('sparse_depth_errors', 'sparse_depth_errors'),
                       ('sparse_depth_values_ndc', 'sparse_depth_values_ndc'), ('mask_pixel_rays', 'indices_mask_nerf'),
                       ('mask_sparse_rays', 'indices_mask_sparse_depth'), ('global_rows', 'global_rows')):
        setattr(b, field, out[key].data_ptr() if key in out else None)
    with torch.cuda.device(dev):
        st = lib.snerf_assemble_batch(ctypes.c_void_p(indices.data_ptr()), n, int(num_pixel_rays), _ptr(table), v, h, w,
                                      _ptr(images), _ptr(tables[0]), _ptr(tables[1]), _ptr(tables[2]), int(ndc), float(near),
                                      float(far), float(near_ndc), float(far_ndc), int(first_pixel_row),
                                      int(first_pixel_row + num_pixel_rays if first_sparse_row is None else first_sparse_row),
                                      ctypes.byref(b), _stream())
    _lib.check(st, 'snerf_assemble_batch')
    return out


def gather_dense_depth(indices: Tensor, num_pixel_rays: int, depths: Tensor, weights: Tensor,
                       depths_ndc: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """One launch: the dense-depth columns of a batch, ``dense_depth_values``, ``dense_depth_weights`` [,
    ``dense_depth_values_ndc``], each (n, 1) -- the first ``num_pixel_rays`` rows gather the per-pixel tables (flat,
    num_views*height*width) at ``indices`` (the int64 GPU tensor ``assemble_batch`` reads), every other row holds -1."""
    lib = _lib.load()
    if not indices.is_cuda or indices.dtype != torch.int64 or indices.dim() != 1:
        raise RuntimeError(f'indices: expected a 1-D int64 GPU tensor, got {indices.dtype} {tuple(indices.shape)} on {indices.device}')
    indices = indices.contiguous()
    n, dev = indices.shape[0], indices.device
    depths = _dev(depths, 'dense_depths')
    if depths.dim() != 1:
        raise RuntimeError(f'dense_depths: expected a flat per-pixel table, got {tuple(depths.shape)}')
    pixels = depths.shape[0]
    weights = _dev(weights, 'dense_depth_weights', (pixels,))
    depths_ndc = _dev(depths_ndc, 'dense_depths_ndc', (pixels,))
    if not 0 <= int(num_pixel_rays) <= n:
        raise RuntimeError(f'gather_dense_depth: {num_pixel_rays} pixel rays of {n} rows')
    out = {'dense_depth_values': torch.empty((n, 1), dtype=torch.float32, device=dev),
           'dense_depth_weights': torch.empty((n, 1), dtype=torch.float32, device=dev)}
    if depths_ndc is not None:
        out['dense_depth_values_ndc'] = torch.empty((n, 1), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        st = lib.snerf_gather_dense_depth(ctypes.c_void_p(indices.data_ptr()), n, int(num_pixel_rays), pixels, _ptr(depths),
                                          _ptr(weights), _ptr(depths_ndc), _ptr(out['dense_depth_values']),
                                          _ptr(out['dense_depth_weights']), _ptr(out.get('dense_depth_values_ndc')), _stream())
    _lib.check(st, 'snerf_gather_dense_depth')
    return out


# ---------------------------------------------------------------------------------------------- f2 scene tables (S1-S3)
def scene_images(images: Tensor, white_bkgd: bool = False) -> Tensor:
    """One launch: (..., C) uint8 images on the device, C = 3 or 4 -> (..., 3) float32, ``u8 / 255`` and, with ``white_bkgd``,
    ``rgb * a + (1 - a)`` over the last channel (the reference's preprocess_images)."""
    images = _typed(images, 'images', (torch.uint8,))
    if images.dim() < 2 or images.shape[-1] not in (3, 4):
        raise RuntimeError(f'images: expected (..., 3) or (..., 4), got {tuple(images.shape)}')
    channels = int(images.shape[-1])
    out = torch.empty(tuple(images.shape[:-1]) + (3,), dtype=torch.float32, device=images.device)
    pixels = images.numel() // channels
    if pixels == 0:
        return out
    _enqueue('snerf_scene_images', images.device, _ptr(images), pixels, channels, int(bool(white_bkgd)), _ptr(out))
    return out


MAX_SPARSE_POINTS = 2 ** 31 - 1      # the winner table of the rasteriser holds int32 point indices


def _points(device, x, y, depth, error, view, num_views: int):
    """The five point arrays of the rasteriser as device tensors.  Host arrays (numpy / CPU tensors: what a loader hands over)
    are checked here -- finite coordinates, views inside [0, num_views) -- and uploaded; device tensors are taken as they are
    (reading them back would be a host round trip: the kernel drops a point without a pixel)."""
    fields = {'x': x, 'y': y, 'depth': depth, 'reprojection_error': error}
    on_device = [isinstance(a, torch.Tensor) and a.is_cuda for a in (*fields.values(), view)]
    if all(on_device):
        out = [_typed(a, name, (torch.float64,)).reshape(-1) for name, a in fields.items()]
        out.append(_typed(view, 'view', (torch.int32,)).reshape(-1))
    elif any(on_device):
        raise RuntimeError('rasterise_sparse_depth: pass the point arrays either all on the host or all on the GPU')
    else:
        host = {name: numpy.ascontiguousarray(numpy.asarray(a, dtype=numpy.float64)).reshape(-1) for name, a in fields.items()}
        views = numpy.asarray(view).reshape(-1)
        for name in ('x', 'y'):
            if not numpy.isfinite(host[name]).all():
                raise ValueError(f'rasterise_sparse_depth: {name} has non-finite coordinates (the reference casts them to an '
                                 f'undefined integer)')
        if views.size and (views.min() < 0 or views.max() >= num_views):
            raise RuntimeError(f'rasterise_sparse_depth: view numbers span [{views.min()}, {views.max()}], outside [0, {num_views})')
        out = [torch.from_numpy(a).to(device) for a in host.values()]
        out.append(torch.from_numpy(numpy.ascontiguousarray(views.astype(numpy.int32))).to(device))
    count = out[0].shape[0]
    if any(t.shape[0] != count for t in out):
        raise RuntimeError(f'rasterise_sparse_depth: point arrays of different lengths {[t.shape[0] for t in out]}')
    if count > MAX_SPARSE_POINTS:
        raise RuntimeError(f'rasterise_sparse_depth: {count} points, at most {MAX_SPARSE_POINTS}')
    return out, count


def rasterise_sparse_depth(x, y, depth, reprojection_error, view, num_views: int, resolution, scale: float = 1.0,
                           divisor: float = 1.0, table: Optional[Tensor] = None, near: float = 1.0, device=None) -> Dict[str, Tensor]:
    """The reference's sparse-depth tables, flat (num_views*h*w,) float32 on the device: ``depths`` = depth * scale and ``errors``
    at the pixel ``(clip(rint(y / divisor)), clip(rint(x / divisor)))`` of each point's view, the last point in input order where
    several share a pixel, -1 where there is none; with a camera ``table`` also ``depths_ndc`` (near plane ``near``).  Point arrays:
    float64 ``x``, ``y``, ``depth``, ``reprojection_error`` and int32 ``view``, all views concatenated, on the host (checked and
    uploaded) or on the GPU.  Two launches and one fill; deterministic."""
    lib = _lib.load()
    h, w, v = int(resolution[0]), int(resolution[1]), int(num_views)
    if v < 1 or h < 1 or w < 1:
        raise RuntimeError(f'rasterise_sparse_depth: bad sizes ({v} views, {h}x{w})')
    if table is not None:
        table = _dev(table, 'camera table', (v, _lib.CAMERA_FLOATS))
        device = table.device
    elif isinstance(x, torch.Tensor) and x.is_cuda:
        device = x.device
    if device is None:
        raise RuntimeError('rasterise_sparse_depth: no device (pass device= with host arrays and no camera table)')
    dev = torch.device(device)
    (px, py, pd, pe, pv), count = _points(dev, x, y, depth, reprojection_error, view, v)
    f = lambda: torch.empty((v * h * w,), dtype=torch.float32, device=dev)
    out = {'depths': f(), 'errors': f()}
    if table is not None:
        out['depths_ndc'] = f()
    workspace = torch.empty((int(lib.snerf_rasterise_sparse_depth_workspace_bytes(v, h, w)),), dtype=torch.uint8, device=dev)
    _enqueue('snerf_rasterise_sparse_depth', dev, _ptr(px), _ptr(py), _ptr(pd), _ptr(pe), _ptr(pv), count, float(scale),
             float(divisor), _ptr(table), float(near), v, h, w, _ptr(out['depths']), _ptr(out['errors']),
             _ptr(out.get('depths_ndc')), _ptr(workspace))
    return out


def depth_table_to_ndc(depths: Tensor, table: Tensor, resolution, near: float) -> Tensor:
    """One launch: the reference's convert_depth_to_ndc over a per-pixel depth table (num_views*h*w entries, any shape) with the
    rays recomputed from the camera ``table``; -1 stays -1.  Returns a tensor of the input's shape."""
    h, w = int(resolution[0]), int(resolution[1])
    v = table.shape[0]
    table = _dev(table, 'camera table', (v, _lib.CAMERA_FLOATS))
    depths = _dev(depths, 'depths')
    if depths.numel() != v * h * w:
        raise RuntimeError(f'depths: {depths.numel()} entries, expected {v}*{h}*{w} (one per pixel)')
    out = torch.empty_like(depths)
    _enqueue('snerf_depth_table_to_ndc', depths.device, _ptr(depths), _ptr(table), v, h, w, float(near), _ptr(out))
    return out


def shuffled_indices(seed: int, epoch: int, first: int, count: int, domain: int, device, candidates: Optional[Tensor] = None,
                     num_views: int = 0, resolution=(0, 0), crop=None, at: Optional[Tensor] = None, sparse: bool = False) -> Tensor:
    """Positions [first, first+count) of epoch ``epoch``'s permutation of the candidate pixels, as global pixel indices.
    ``at`` (``IterationRing.current``): epoch and position come from the device-resident iteration record (its pixel or
    ``sparse`` pair), ``first`` is then the offset added to that position (a rank's shard of the slice)."""
    lib = _lib.load()
    h, w = int(resolution[0]), int(resolution[1])
    y0, y1, x0, x1 = crop if crop is not None else (0, h, 0, w)
    if candidates is not None:
        if not candidates.is_cuda or candidates.dtype != torch.int64 or tuple(candidates.shape) != (domain,):
            raise RuntimeError(f'candidates: expected int64 GPU tensor ({domain},), got {candidates.dtype} {tuple(candidates.shape)}')
        candidates = candidates.contiguous()
        device = candidates.device
    out = torch.empty((count,), dtype=torch.int64, device=device)
    if count == 0:
        return out
    with torch.cuda.device(out.device):
        if at is not None:
            st = lib.snerf_shuffled_indices_at(int(seed) & (2 ** 64 - 1), ctypes.c_void_p(at.data_ptr()), int(bool(sparse)), int(first),
                                               int(count), int(domain), ctypes.c_void_p(0 if candidates is None else candidates.data_ptr()),
                                               int(num_views), h, w, int(y0), int(y1), int(x0), int(x1),
                                               ctypes.c_void_p(out.data_ptr()), _stream())
        else:
            st = lib.snerf_shuffled_indices(int(seed) & (2 ** 64 - 1), int(epoch), int(first), int(count), int(domain),
                                            ctypes.c_void_p(0 if candidates is None else candidates.data_ptr()), int(num_views), h, w,
                                            int(y0), int(y1), int(x0), int(x1), ctypes.c_void_p(out.data_ptr()), _stream())
    _lib.check(st, 'snerf_shuffled_indices')
    return out


def _draw_target(shape, device, out: Optional[Tensor]) -> Tensor:
    if out is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise RuntimeError(f'draw target: expected a contiguous float32 GPU tensor of shape {tuple(shape)}')
    return out


def _row_ids(rows: Optional[Tensor], count: int) -> Optional[Tensor]:
    if rows is None:
        return None
    if not rows.is_cuda or rows.dtype != torch.int64 or tuple(rows.shape) != (count,):
        raise RuntimeError(f'global rows: expected an int64 GPU tensor of shape ({count},), got {rows.dtype} {tuple(rows.shape)} on {rows.device}')
    return rows.contiguous()


def random_uniform(seed: int, stream_id: int, first_row: int, shape, device, out: Optional[Tensor] = None,
                   rows: Optional[Tensor] = None, at=None) -> Tensor:
    """[0,1) Philox draws of shape (rows, width...); element (r, c) depends only on (seed, stream_id, global row of r, c),
    where the global row is ``rows[r]`` (int64 GPU tensor, e.g. a batch's ``global_rows``) or ``first_row + r``.
    ``out`` (optional) receives the draws in place (static buffers of a captured graph)."""
    lib = _lib.load()
    out = _draw_target(shape, device, out)
    count = int(shape[0])
    width = out.numel() // count if count else 1
    if out.numel() == 0:
        return out
    rows = _row_ids(rows, count)
    with torch.cuda.device(out.device):
        if at is not None:      # (record, kind, number of kinds): the stream is record.iter_num * kinds + kind, read on the device
            st = lib.snerf_random_uniform_at(int(seed) & (2 ** 64 - 1), ctypes.c_void_p(at[0].data_ptr()), int(at[1]), int(at[2]),
                                             int(first_row), ctypes.c_void_p(0 if rows is None else rows.data_ptr()), count,
                                             max(width, 1), _ptr(out), _stream())
        else:
            st = lib.snerf_random_uniform(int(seed) & (2 ** 64 - 1), int(stream_id) & 0xFFFFFFFF, int(first_row),
                                          ctypes.c_void_p(0 if rows is None else rows.data_ptr()), count, max(width, 1), _ptr(out),
                                          _stream())
    _lib.check(st, 'snerf_random_uniform')
    return out


def random_normal(seed: int, stream_id: int, first_row: int, shape, device, scale: float = 1.0,
                  out: Optional[Tensor] = None, rows: Optional[Tensor] = None, at=None) -> Tensor:
    lib = _lib.load()
    out = _draw_target(shape, device, out)
    count = int(shape[0])
    width = out.numel() // count if count else 1
    if out.numel() == 0:
        return out
    rows = _row_ids(rows, count)
    with torch.cuda.device(out.device):
        if at is not None:
            st = lib.snerf_random_normal_at(int(seed) & (2 ** 64 - 1), ctypes.c_void_p(at[0].data_ptr()), int(at[1]), int(at[2]),
                                            int(first_row), ctypes.c_void_p(0 if rows is None else rows.data_ptr()), count,
                                            max(width, 1), float(scale), _ptr(out), _stream())
        else:
            st = lib.snerf_random_normal(int(seed) & (2 ** 64 - 1), int(stream_id) & 0xFFFFFFFF, int(first_row),
                                         ctypes.c_void_p(0 if rows is None else rows.data_ptr()), count, max(width, 1), float(scale),
                                         _ptr(out), _stream())
    _lib.check(st, 'snerf_random_normal')
    return out


# ---------------------------------------------------------------------------------------------- whole-iteration graphs
class IterationRing:
    """The per-iteration scalars of a replayed training graph (struct snerf_iteration, include/simplenerf_train.h): a ring of
    records in PINNED host memory that the host fills ahead of time, a device-resident counter and the device-resident
    ``current`` record.  ``advance()`` (captured as the graph's first node) makes record ``counter mod slots`` current."""

    def __init__(self, device, slots: int = 8):
        self.slots = int(slots)
        self.device = torch.device(device)
        self.ring = torch.zeros((self.slots, _lib.ITERATION_WORDS), dtype=torch.int64).pin_memory()
        self.view = self.ring.numpy()
        self.counter = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.current = torch.zeros((_lib.ITERATION_WORDS,), dtype=torch.int64, device=self.device)
        self.filled = 0                       # records written so far = index of the next replay

    def fill(self, iter_num: int, pixel: tuple, sparse: tuple, adam_neg_step_size: float, adam_bias2_sqrt: float) -> int:
        """Write the record of the NEXT replay; ``pixel`` / ``sparse`` = (epoch, first).  -> its slot."""
        slot = self.filled % self.slots
        row = self.view[slot]
        row[0], row[1], row[2], row[3], row[4] = int(iter_num), int(pixel[0]), int(pixel[1]), int(sparse[0]), int(sparse[1])
        row[5] = int(numpy.array([adam_neg_step_size, adam_bias2_sqrt], dtype=numpy.float32).view(numpy.int64)[0])
        self.filled += 1
        return slot

    def advance(self) -> None:
        _enqueue('snerf_iteration_advance', self.device, ctypes.c_void_p(self.ring.data_ptr()), self.slots,
                 ctypes.c_void_p(self.counter.data_ptr()), ctypes.c_void_p(self.current.data_ptr()))


# ---------------------------------------------------------------------------------------------- Q3 LPIPS
LPIPS_MIN_EXTENT = 31      # the smallest side AlexNet's features accept: relu1 7 -> pool 3 -> pool 1
# (c_out, c_in, kernel) of the five convolutions whose post-ReLU outputs are the taps
LPIPS_CONVS = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
LPIPS_VGG_MIN_EXTENT = 16  # the smallest side VGG-16's features accept down to relu5_3: 16 -> 8 -> 4 -> 2 -> 1
# (c_out, c_in, kernel) of VGG-16's thirteen convolutions, and which of them the five taps follow (relu1_2 .. relu5_3)
LPIPS_VGG_CONVS = ((64, 3, 3), (64, 64, 3), (128, 64, 3), (128, 128, 3), (256, 128, 3), (256, 256, 3), (256, 256, 3), (512, 256, 3),
                   (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3))
LPIPS_VGG_TAP_CONVS = (1, 3, 6, 9, 12)
# net -> (the C ABI's selector, the name in messages, minimum extent, convolutions, the convolution each tap follows)
_LPIPS_NETS = {'alex': (C.SNERF_LPIPS_ALEX, 'AlexNet', LPIPS_MIN_EXTENT, LPIPS_CONVS, (0, 1, 2, 3, 4)),
               'vgg': (C.SNERF_LPIPS_VGG16, 'VGG-16', LPIPS_VGG_MIN_EXTENT, LPIPS_VGG_CONVS, LPIPS_VGG_TAP_CONVS)}


def _lpips_net(net):
    if net not in _LPIPS_NETS:
        raise RuntimeError(f"net: expected 'alex' or 'vgg', got {net!r}")
    return _LPIPS_NETS[net]


def _pointer_array(tensors) -> ctypes.Array:
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def lpips_pack(conv_weights, conv_biases, lin_weights, shift=None, scale=None, net: str = 'alex') -> Tensor:
    """The tensors of LPIPS-alex (15) or LPIPS-vgg (13 + 13 + 5) -> the packed fp32 device buffer ``lpips_sums`` reads
    (snerf_lpips_net_pack): every convolution re-ordered to [k = (tap row, tap column, channel)][c_out].  ``conv_weights[l]``
    float32 (c_out, c_in, k, k), ``conv_biases[l]`` (c_out), ``lin_weights[t]`` (c_out of tap t) (or (1, c_out, 1, 1)), all on one
    GPU; ``shift`` / ``scale``: three numbers each, the scaling layer's buffers (default: the package's constants)."""
    selector, _, _, convs, tap_convs = _lpips_net(net)
    if not (len(conv_weights) == len(conv_biases) == len(convs) and len(lin_weights) == len(tap_convs)):
        if net == 'alex':
            raise RuntimeError(f'lpips_pack: expected {len(LPIPS_CONVS)} convolution weights, biases and lin weights')
        raise RuntimeError(f'lpips_pack: expected {len(convs)} convolution weights and biases and {len(tap_convs)} lin weights')
    weights, biases, lins = [], [], []
    for l, (c_out, c_in, k) in enumerate(convs):
        weights.append(_typed(conv_weights[l], f'conv_weights[{l}]', (torch.float32,), (c_out, c_in, k, k)))
        biases.append(_typed(conv_biases[l], f'conv_biases[{l}]', (torch.float32,), (c_out,)))
        if l in tap_convs:
            t = tap_convs.index(l)
            lin = _typed(lin_weights[t], f'lin_weights[{t}]', (torch.float32,))
            if tuple(lin.shape) not in ((c_out,), (1, c_out, 1, 1)):
                raise RuntimeError(f'lin_weights[{t}]: expected shape {(1, c_out, 1, 1)} or {(c_out,)}, got {tuple(lin.shape)}')
            lins.append(lin)
    dev = weights[0].device
    for name, group in (('conv_weights', weights), ('conv_biases', biases), ('lin_weights', lins)):
        for l, t in enumerate(group):
            if t.device != dev:
                raise RuntimeError(f'{name}[{l}]: expected a tensor on {dev}, got one on {t.device}')
    scaling = None
    if (shift is None) != (scale is None):
        raise RuntimeError('lpips_pack: shift and scale come together')
    if shift is not None:
        values = [float(v) for v in torch.as_tensor(shift).reshape(-1).tolist()] + [float(v) for v in torch.as_tensor(scale).reshape(-1).tolist()]
        if len(values) != 6:
            raise RuntimeError('lpips_pack: shift and scale hold three values each')
        scaling = (ctypes.c_float * 6)(*values)
    lib = _lib.load()
    packed = torch.empty((int(lib.snerf_lpips_net_packed_floats(selector)),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = lib.snerf_lpips_net_pack(selector, _pointer_array(weights), _pointer_array(biases), _pointer_array(lins), scaling, _ptr(packed),
                                      _stream())
    _lib.check(st, 'snerf_lpips_pack')      # (inline, not _enqueue: the message keeps the name it had before the selector)
    return packed


def lpips_tap_shapes(height: int, width: int, net: str = 'alex'):
    """[(tap_h, tap_w, channels)] of the five taps for a height x width frame."""
    selector = _lpips_net(net)[0]
    lib = _lib.load()
    shapes = []
    for l in range(5):
        th, tw, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(lib.snerf_lpips_net_tap_shape(selector, int(height), int(width), l, ctypes.byref(th), ctypes.byref(tw), ctypes.byref(c)),
                   'snerf_lpips_tap_shape')
        shapes.append((th.value, tw.value, c.value))
    return shapes


def lpips_sums(gt: Tensor, image: Tensor, packed: Tensor, mask: Optional[Tensor] = None, return_taps: bool = False, net: str = 'alex'):
    """-> float64 (5) on the device: per tap of the network the sum over its pixels of sum_c lin_c (n_gt - n_eval)^2 (LPIPS is the
    sum of sums[l] / (tap_h_l tap_w_l)); with a mask, eval is where(mask, eval, gt).  ``packed``: what ``lpips_pack`` returned for
    the same ``net``.  ``return_taps``: also the five post-ReLU activations, float32 (2, tap_h, tap_w, channels), gt first,
    channels last."""
    selector, name, min_extent, _, _ = _lpips_net(net)
    gt, image, mask, h, w = _image_pair(gt, image, mask)
    if min(h, w) < min_extent:
        raise RuntimeError(f'gt_image: {name} needs {min_extent} pixels on every side, the image extent is {h} x {w}')
    lib = _lib.load()
    packed = _typed(packed, 'packed', (torch.float32,), (int(lib.snerf_lpips_net_packed_floats(selector)),))
    if packed.device != gt.device:
        raise RuntimeError(f'packed: expected a tensor on {gt.device}, got one on {packed.device}')
    need = int(lib.snerf_lpips_net_workspace_bytes(selector, h, w))
    if need <= 0:
        raise RuntimeError(f'gt_image: the image extent {h} x {w} exceeds what the LPIPS kernels index')
    sums = torch.empty((5,), dtype=torch.float64, device=gt.device)
    taps = [torch.empty((2, th, tw, c), dtype=torch.float32, device=gt.device) for th, tw, c in lpips_tap_shapes(h, w, net)] if return_taps else None
    with torch.cuda.device(gt.device):
        ws = _workspace(('lpips', net), gt.device, need)      # one per (device, network)
        st = lib.snerf_lpips_net_sums(selector, _ptr(gt), _ptr(image), _ptr(mask), h, w, _ptr(packed), _ptr(sums),
                                      None if taps is None else _pointer_array(taps), _ptr(ws), _stream())
    _lib.check(st, 'snerf_lpips_sums')      # (as in lpips_pack)
    return (sums, taps) if return_taps else sums
