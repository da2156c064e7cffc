"""The restated weight-gradient planner (tests/wgrad_plan.py) and its probe set, without a GPU: invariants every chunk plan must
keep, and the sensitivity of the boundary probe as an instrument.  That the restatement IS the library's planner is asserted on the
device machine (tests/test_gpu_wgrad_plans.py: its workspace total against snerf_mlp_backward_workspace_floats)."""
import functools

import numpy
import pytest

from simplenerf_amd import synth
from tests import wgrad_plan
from tests.wgrad_plan import KINDS, SIZES, SWEEP

LAYOUTS = {'main': {}, 'ptsaug': dict(sigma_pe_degree=3), 'viewsaug': dict(use_view_dirs=False, view_dependent_rgb=False)}
MLPS = [(8, 256, 128), (4, 128, 64)]
TOTALS = sorted(set(SWEEP) | {n * s for n, s in SIZES})


def config(layout, size):
    depth, width, vwidth = size
    return synth.mlp_config(64, depth=depth, width=width, views_width=vwidth, **LAYOUTS[layout])


def test_layouts_are_the_gpu_suites():
    """(restated here so that this module imports no GPU test)"""
    from tests import test_gpu_kernels
    assert LAYOUTS == test_gpu_kernels.LAYOUTS


@functools.lru_cache(maxsize=None)
def counted_empty(chunks, blocks):
    per = -(-blocks // chunks)
    return sum(1 for c in range(chunks) if c * per >= blocks)


@pytest.mark.parametrize('size', MLPS)
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_every_plan_keeps_the_invariants(layout, size):
    cfg = config(layout, size)
    for total in TOTALS:
        for kind in KINDS:
            pl = wgrad_plan.plan(cfg, total, kind)
            B = pl.blocks
            assert B % 4 == 0 and B * 32 >= total > (B - (8 if kind != 'fp32' else 4)) * 32, (total, kind, B)
            assert 64 <= pl.large_budget <= 256
            assert len(pl.jobs) <= 16                                      # kMaxJobs (mlp_backward.hip:259)
            for j in pl.jobs:
                tag = (total, kind, j.name)
                assert 1 <= j.chunks <= max(1, B // 8), tag
                assert j.per == -(-B // j.chunks) and j.blocks == B, tag
                live = j.chunks - j.empty_chunks
                # chunk c holds [c per, min((c + 1) per, B)): the non-empty ones tile [0, B) exactly once
                assert live >= 1 and (live - 1) * j.per < B <= live * j.per, tag
                assert j.chunk_range(0)[0] == 0 and j.chunk_range(live - 1)[1] == B, tag
                assert j.empty_chunks == counted_empty(j.chunks, B), tag
                if not j.launched:                                         # a rider: a view of its host's partial sums
                    host = wgrad_plan.host_of(pl, j)
                    assert host is not None and kind != 'fp32', tag
                    assert (j.chunks, j.partial_off, j.bias_off) == (host.chunks, host.partial_off, host.bias_off), tag
                    assert j.partial_ld == host.in_tiles * 32 and j.partial_col0 == (host.in_tiles - host.x2_tiles) * 32, tag
            large = pl.of_class('large')
            assert sum(j.chunks for j in large) <= pl.large_budget, (total, kind)
            assert (size[1] == 256) == bool(large)                         # the narrow MLP has no large class at all
            assert pl.total_floats == pl.grads_floats + pl.partial_floats
            # the partial sums of the launched jobs lie one behind the other, after the zero pages and the region table
            off = 448 + 64 * 128
            for j in pl.launched():
                assert j.partial_off == off and j.bias_off == off + j.chunks * j.out_tiles * 32 * j.in_tiles * 32
                off = j.bias_off + j.chunks * j.out_tiles * 32
            assert off == pl.partial_floats


@pytest.mark.parametrize('n,s', SIZES)
def test_chunks_of_the_table_sizes_cover_every_block_once(n, s):
    """the tiling once more by counting, at the sizes the device tests run"""
    for layout, size in [('main', MLPS[0]), ('main', MLPS[1]), ('ptsaug', MLPS[0]), ('viewsaug', MLPS[0])]:
        for kind in KINDS:
            pl = wgrad_plan.plan(config(layout, size), n * s, kind)
            for j in pl.jobs:
                seen = numpy.zeros(pl.blocks, dtype=numpy.int64)
                empty = 0
                for c in range(j.chunks):
                    b0, b1 = j.chunk_range(c)
                    empty += b0 >= b1
                    if b0 < b1:
                        seen[b0:b1] += 1
                assert (seen == 1).all() and empty == j.empty_chunks, (layout, size, kind, j.name)


@pytest.mark.parametrize('size', MLPS)
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_probe_blocks_hold_every_chunk_boundary(layout, size):
    cfg = config(layout, size)
    for total in TOTALS:
        for kind in KINDS:
            pl = wgrad_plan.plan(cfg, total, kind)
            probe = wgrad_plan.probe_blocks(pl)
            real = -(-total // 32)
            assert probe == sorted(set(probe)) and 1 <= len(probe) <= wgrad_plan.PROBE_MAX_BLOCKS, (total, kind, len(probe))
            assert 0 <= probe[0] and probe[-1] == real - 1, (total, kind)
            have = set(probe)
            for j in pl.launched():
                last = j.chunks - j.empty_chunks - 1
                for c in (0, last):
                    b0, b1 = j.chunk_range(c)
                    for b in (b0, b1 - 1, b1):
                        assert b in have or b >= real, (total, kind, j.name, c, b)


# ------------------------------------------------------------------------------------- the fp32 saved tensor's decoder
@pytest.mark.parametrize('layout,size', [('main', MLPS[1]), ('viewsaug', MLPS[1])])
def test_decode_fused32_reads_back_a_tensor_laid_out_by_hand(layout, size):
    """A saved tensor written element by element from csrc/mlp_plan.h:61-75 (row = feature, column = sample of the wave block;
    mask dword (t >> 1, sample + 32 half), bit 16 (t & 1) + r <-> feature (r & 3) + 8 (r >> 2) + 4 half of tile t), decoded whole
    and through blocks=: the listed blocks' real samples, in order."""
    import torch
    from tests.fused_saved_reference import decode_fused32
    cfg = config(layout, size)
    p = wgrad_plan.rows_of(cfg)
    total = 3 * 128 + 41                                            # four workgroups, the last wave block holds 9 samples
    blocks_all = (total + 127) // 128 * 4
    rng = numpy.random.RandomState(3)
    rows = p.act_rows()
    saved = rng.standard_normal((blocks_all, rows, 32)).astype(numpy.float32)
    by_sample = saved.transpose(0, 2, 1).reshape(blocks_all * 32, rows).astype(numpy.float64)    # [sample][row]
    words = numpy.zeros((blocks_all, (p.mask_tiles() + 1) // 2, 64), dtype=numpy.uint32)
    bits = rng.randint(0, 2, (blocks_all * 32, p.mask_tiles() * 32)).astype(bool)       # [sample][32 t + feature of tile t]
    for t in range(p.mask_tiles()):
        for r in range(16):
            for half in range(2):
                f = (r & 3) + 8 * (r >> 2) + 4 * half
                col = bits[:, 32 * t + f].reshape(blocks_all, 32).astype(numpy.uint32)
                words[:, t >> 1, 32 * half:32 * half + 32] |= col << numpy.uint32(16 * (t & 1) + r)
    saved[:, p.act_mask():p.act_mask() + 2 * words.shape[1]] = words.view(numpy.float32).reshape(blocks_all, -1, 32)
    flat = torch.from_numpy(saved.reshape(-1))
    for pick in (None, [0, 5, 12, 13], [13], [2, 1]):
        dec = decode_fused32(flat, cfg, total, pick)
        want = numpy.arange(total) if pick is None else numpy.concatenate([numpy.arange(32 * b, min(32 * b + 32, total)) for b in pick])
        assert dec['samples'].tolist() == want.tolist()
        assert numpy.array_equal(dec['pe'].numpy(), by_sample[want, :p.full_pe])
        W = p.width
        for l in range(p.depth):
            assert numpy.array_equal(dec['h'][l].numpy(), by_sample[want, p.act_h(l + 1):p.act_h(l + 1) + W])
            assert numpy.array_equal(dec['mask'][l].numpy(), bits[want, l * W:(l + 1) * W])
        assert ('hv' in dec) == p.view_dependent
        if p.view_dependent:
            assert numpy.array_equal(dec['pev'].numpy(), by_sample[want, 64:64 + p.views_pe])
            assert numpy.array_equal(dec['feature'].numpy(), by_sample[want, p.act_feature():p.act_feature() + W])
            assert numpy.array_equal(dec['hv'].numpy(), by_sample[want, p.act_hv():p.act_hv() + p.views_width])
            assert numpy.array_equal(dec['vmask'].numpy(), bits[want, p.depth * W:p.depth * W + p.views_width])


# ------------------------------------------------------------------------------------------- the probe as an instrument
GATE_16BIT = 4.8e-3          # GRAD_REL_MAX of tests/test_gpu_rounding.py: the widest gate a probe case is held to
# (out, in) of the weight tensors of the two MLPs in the three layouts
WEIGHT_SHAPES = [(256, 63), (256, 256), (256, 319), (256, 21), (256, 277), (1, 256), (4, 256), (128, 283), (128, 325), (3, 128),
                 (128, 63), (128, 128), (64, 155), (3, 64), (4, 128)]


@pytest.mark.parametrize('k', [3, 17, 40, 64])
def test_a_lost_block_moves_every_weight_gradient_far_beyond_the_gate(k):
    """With the upstream gradient confined to k <= 64 probe blocks, each block carries about 1 / sqrt(k) of a weight gradient's
    scale: a chunk that lost (or doubled) ANY one of them moves EVERY weight-gradient tensor by more than 10x the widest gate.
    The operands have the statistics the device test gives them: zero-mean layer gradients of comparable size in every block
    (the random upstream of tests/test_gpu_wgrad_plans.py), X a ReLU output or an encoding in [-1, 1].  (A bias gradient with a
    single entry, the density head's, is one zero-mean sum: a block's share of it has no lower bound, so the condition is stated
    for the weights.  The device test asserts the biases all the same.)"""
    rng = numpy.random.RandomState(k)
    for out, in_ in WEIGHT_SHAPES:
        dz = rng.standard_normal((k, 32, out))
        x = numpy.maximum(rng.standard_normal((k, 32, in_)), 0.0) if in_ % 32 == 0 else rng.uniform(-1, 1, (k, 32, in_))
        per_block = numpy.einsum('kso,ksi->koi', dz, x)
        whole = per_block.sum(0)
        moved = numpy.abs(per_block).max(axis=(1, 2)) / numpy.abs(whole).max()
        assert moved.min() > 10 * GATE_16BIT, (out, in_, k, float(moved.min()))
