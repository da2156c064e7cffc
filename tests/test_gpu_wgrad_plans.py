"""The fused MLP backward's weight gradients against float64 in every chunk plan (wgrad_kernel / wgrad16_kernel / reduce_kernel and
plan_workspace of csrc/mlp_backward.hip).

The planner splits each product dW = dY . X^T over workgroups ("chunks") by the number of samples alone; a chunk that loses, doubles
or misplaces a wave block, an empty chunk whose partial is not zero, or a padded lane that contributes, is a wrong gradient that the
ReLU-flip-wide end-to-end gates do not see.  Here:

  a. the Python restatement of the planner (tests/wgrad_plan.py) is the library's: the largest of its three totals equals
     PackedMlp.backward_workspace_floats at every swept sample count; every later test asserts through it the regime its size is in
     (REGIMES: the large class's budget, and the distinct (chunks, blocks per chunk, empty chunks) of each job class), so that a size
     that a later planner change moves out of its regime fails instead of testing less;
  c. boundary probe: upstream gradients random on the samples of wgrad_plan.probe_blocks (<= 64 wave blocks: the first and last
     block of every job's first, middle and last non-empty chunk, the block after each, the call's last real block) and exactly
     zero elsewhere, every parameter gradient against float64 from the kernel's OWN saved activations and ReLU masks of those
     blocks (fp32 / f16x3: tests/fused_saved_reference.py with rounding_ref.EXACT; f16 / bf16: decode_fused with the mode's
     rounding).  Zero upstream contributes exactly nothing, so the reference costs the same at 315 and at 262 272 samples;
  d. dense random upstream against the same reference over all samples, up to 8256 samples;
  e. the s8 modes at 8256 and 49 408 samples, where the spare redistribution gives the trunk jobs unequal chunk counts, against the
     16-bit mode's records with rounding_ref's e4m3 X operand (their forward is held bit-equal to the 16-bit one elsewhere);
  f. backward(into=...) at 3400 samples (empty chunks present).

Sizes (SIZES of tests/wgrad_plan.py) and what the restatement says of them -- every regime sits at the size the planner's reading
gave, none had to move:
     315  one chunk (fp32), two of 8 (16-bit)            1000  cap-bound: 4 chunks of 8
    3400  fp32 small and views jobs 13 chunks of 9, the last one empty; large jobs 8 ragged chunks of 14 (the last holds 10)
    8256  fp32 small / views 32 chunks of 9, 3 empty; s8: trunk jobs on 7 / 8 / 9 chunks
  20 000  fp32 small 78 chunks of 9, 8 empty; the views job on its 64-chunk floor (fp32: one of them empty)
  33 000  views job 64 chunks of 17, 3 empty, in every mode
  49 408  budget 96; 16-bit small jobs 192 chunks of 9, 20 empty; s8: trunk jobs on 11 / 12 / 14 chunks
  65 664  budget 128; fp32 small jobs 256 chunks of 9, 28 empty; 16-bit small jobs 192 of 11, 5 empty
 262 272  budget 256, 32 chunks per trunk job, fp32 small / views 256 chunks of 33, 7 empty; five samples past a workgroup
          boundary: the last workgroup ends in wholly padded wave blocks
The 4 x 128 MLP has no large class: all of its jobs are small ones.

Gates.  f16 / bf16: GRAD_REL_MAX, GRAD_REL_L2 of tests/test_gpu_rounding.py, unchanged.  fp32 / f16x3 (identical masks: what
remains is fp32 summation and the f16x3 split) and the s8 modes: the smaller of a ceiling -- 1e-4 of the tensor's largest entry and
1e-4 relative L2, the gate of test_f16x3_chain_arithmetic_with_identical_masks; GRAD_REL_MAX + S8_DELTA_L2 for s8 -- and 4x the
worst value observed on the MI355X over all cases of this module (the rule of tests/test_gpu_rounding.py).  Observed (printed in
pytest's summary, tag `wgrad_plans/...`):
  fp32    1.8e-6 of max (dense, 8 x 256, 8256 samples), 1.0e-6 rel L2 (probe, 262 272)   -> gates 7.2e-6, 4.0e-6
  f16x3   2.5e-6 of max (probe, 8 x 256, 3400), 1.7e-6 rel L2 (probe, 65 664)              -> gates 1.0e-5, 6.8e-6
  f16     2.2e-3 of max (probe, 65 664), 7.2e-4 rel L2;  bf16  1.4e-3, 5.6e-4               (gates 4.8e-3, 2e-3 as they were)
  f16s8   2.2e-3 of max, 4.2e-4 rel L2 (8256)                                               -> gates 7.8e-3 (the ceiling), 1.7e-3
  bf16s8  1.6e-3 of max, 8.6e-4 rel L2 (49 408)                                             -> gates 6.4e-3, 3.4e-3
  into=   1.00 fp32 ulp of max(|prior|, |fresh|) [INTO_ULPS = 2]
No case with empty or ragged chunks, padded tail blocks or unequal chunk counts was further from float64 than the others: the
kernels needed no fix.  test_boundary_probe_sees_a_lost_block is the negative control of the probe.
"""
import numpy
import pytest
import torch

from simplenerf_amd import ops, synth
from tests import rounding_ref as rr
from tests import util, wgrad_plan
from tests.fused_saved_reference import decode_fused32
from tests.test_gpu_grads import rel_l2, rel_to_max
from tests.test_gpu_rounding import (FUSED_MODES, GRAD_REL_L2, GRAD_REL_MAX, S8_DELTA_L2, accumulate_check, decode_fused, fused_case,
                                     fused_records, packed, reference_grads)
from tests.wgrad_plan import KIND_OF, SIZES, SWEEP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = ops.PRECISIONS

WIDE, NARROW = (8, 256, 128), (4, 128, 64)
AUG_SIZES = [(50, 68), (165, 200)]
CASES = [('main', size, n, s) for size in (WIDE, NARROW) for n, s in SIZES] + \
        [(layout, WIDE, n, s) for layout in ('ptsaug', 'viewsaug') for n, s in AUG_SIZES]
DENSE_CASES = [c for c in CASES if c[2] * c[3] <= 8256]
S8_CASES = [(64, 129), (193, 256)]
PRECISIONS = ['fp32', 'f16x3', 'f16', 'bf16']

CEILING_32 = 1e-4
CEILING_S8 = (GRAD_REL_MAX + S8_DELTA_L2, GRAD_REL_L2 + S8_DELTA_L2)
# worst (of the tensor's largest entry, relative L2) observed on the MI355X over all cases of this module (module docstring)
OBSERVED = {'fp32': (1.8e-6, 1.0e-6), 'f16x3': (2.5e-6, 1.7e-6), 'f16s8': (2.2e-3, 4.2e-4), 'bf16s8': (1.6e-3, 8.6e-4)}
CEILINGS = {'fp32': (CEILING_32, CEILING_32), 'f16x3': (CEILING_32, CEILING_32), 'f16s8': CEILING_S8, 'bf16s8': CEILING_S8}
# the smaller of the ceiling and 4x the worst observed; the 16-bit modes keep the gates of tests/test_gpu_rounding.py
GATES = {q: tuple(min(c, 4 * o) for c, o in zip(CEILINGS[q], OBSERVED[q])) for q in OBSERVED}
GATES.update({'f16': (GRAD_REL_MAX, GRAD_REL_L2), 'bf16': (GRAD_REL_MAX, GRAD_REL_L2)})

# (layout, trunk width, samples) -> plan -> (budget of the large class, then the sorted distinct (chunks, blocks per chunk, empty
# chunks) of the launched jobs of the classes 'large' (8 x 8 tiles), 'views' (the lone 4 x 8 / 4 x 9 job) and 'small')
REGIMES = {
    ('main', 256, 315): {'fp32': (64, [(1, 12, 0)], [(1, 12, 0)], [(1, 12, 0)]),
                         'f16': (64, [(2, 8, 0)], [(2, 8, 0)], [(2, 8, 0)])},
    ('main', 256, 1000): {'fp32': (64, [(4, 8, 0)], [(4, 8, 0)], [(4, 8, 0)]),
                          'f16': (64, [(4, 8, 0)], [(4, 8, 0)], [(4, 8, 0)])},
    ('main', 256, 3400): {'fp32': (64, [(8, 14, 0)], [(13, 9, 1)], [(13, 9, 1)]),
                          'f16': (64, [(8, 14, 0)], [(14, 8, 0)], [(14, 8, 0)])},
    ('main', 256, 8256): {'fp32': (64, [(8, 33, 0)], [(32, 9, 3)], [(32, 9, 3)]),
                          'f16': (64, [(8, 33, 0)], [(33, 8, 0)], [(33, 8, 0)]),
                          'f16s8': (64, [(7, 38, 0), (8, 33, 0), (9, 30, 0)], [(33, 8, 0)], [(33, 8, 0)])},
    ('main', 256, 20000): {'fp32': (64, [(8, 79, 0)], [(64, 10, 1)], [(78, 9, 8)]),
                           'f16': (64, [(8, 79, 0)], [(64, 10, 0)], [(79, 8, 0)])},
    ('main', 256, 33000): {'fp32': (64, [(8, 129, 0)], [(64, 17, 3)], [(129, 8, 0)]),
                           'f16': (64, [(8, 129, 0)], [(64, 17, 3)], [(129, 8, 0)])},
    ('main', 256, 49408): {'fp32': (96, [(12, 129, 0)], [(64, 25, 2)], [(193, 8, 0)]),
                           'f16': (96, [(12, 129, 0)], [(64, 25, 2)], [(192, 9, 20)]),
                           'f16s8': (96, [(11, 141, 0), (12, 129, 0), (14, 111, 0)], [(64, 25, 2)], [(192, 9, 20)])},
    ('main', 256, 65664): {'fp32': (128, [(16, 129, 0)], [(64, 33, 1)], [(256, 9, 28)]),
                           'f16': (128, [(16, 129, 0)], [(64, 33, 1)], [(192, 11, 5)])},
    ('main', 256, 262272): {'fp32': (256, [(32, 257, 0)], [(256, 33, 7)], [(256, 33, 7)]),
                            'f16': (256, [(32, 257, 0)], [(256, 33, 7)], [(192, 43, 1)])},
    ('main', 128, 315): {'fp32': (64, [], [], [(1, 12, 0)]), 'f16': (64, [], [], [(2, 8, 0)])},
    ('main', 128, 1000): {'fp32': (64, [], [], [(4, 8, 0)]), 'f16': (64, [], [], [(4, 8, 0)])},
    ('main', 128, 3400): {'fp32': (64, [], [], [(13, 9, 1)]), 'f16': (64, [], [], [(14, 8, 0)])},
    ('main', 128, 8256): {'fp32': (64, [], [], [(32, 9, 3)]), 'f16': (64, [], [], [(33, 8, 0)])},
    ('main', 128, 20000): {'fp32': (64, [], [], [(78, 9, 8)]), 'f16': (64, [], [], [(79, 8, 0)])},
    ('main', 128, 33000): {'fp32': (64, [], [], [(129, 8, 0)]), 'f16': (64, [], [], [(129, 8, 0)])},
    ('main', 128, 49408): {'fp32': (96, [], [], [(193, 8, 0)]), 'f16': (96, [], [], [(192, 9, 20)])},
    ('main', 128, 65664): {'fp32': (128, [], [], [(256, 9, 28)]), 'f16': (128, [], [], [(192, 11, 5)])},
    ('main', 128, 262272): {'fp32': (256, [], [], [(256, 33, 7)]), 'f16': (256, [], [], [(192, 43, 1)])},
    ('ptsaug', 256, 3400): {'fp32': (64, [(8, 14, 0)], [(13, 9, 1)], [(13, 9, 1)]),
                            'f16': (64, [(8, 14, 0)], [(14, 8, 0)], [(14, 8, 0)])},
    ('ptsaug', 256, 33000): {'fp32': (64, [(8, 129, 0)], [(64, 17, 3)], [(129, 8, 0)]),
                             'f16': (64, [(8, 129, 0)], [(64, 17, 3)], [(129, 8, 0)])},
    # (no views layer: seven trunk products share the budget, 64 = 6 x 9 + 10)
    ('viewsaug', 256, 3400): {'fp32': (64, [(9, 12, 0), (10, 11, 0)], [], [(13, 9, 1)]),
                              'f16': (64, [(9, 13, 0), (10, 12, 0)], [], [(14, 8, 0)])},
    ('viewsaug', 256, 33000): {'fp32': (64, [(9, 115, 0), (10, 104, 0)], [], [(129, 8, 0)]),
                               'f16': (64, [(9, 115, 0), (10, 104, 0)], [], [(129, 8, 0)])},
}


# -------------------------------------------------------------------------------------------------------------------- helpers
_MODELS = {}
WORST = {}


def model(layout, size):
    """(cfg, state dict, packed MLP, parameter shapes, parameter names), one per MLP for the whole module: fused_case's weights
    depend on the layout and the size alone"""
    key = (layout, size)
    if key not in _MODELS:
        cfg, sd, _, _ = fused_case(layout, size, 1, 1)
        mlp, shapes = packed(cfg, sd)
        _MODELS[key] = (cfg, sd, mlp, shapes, synth.abi_param_list({k: k for k in sd}))
    return _MODELS[key]


def plan_in_its_regime(layout, size, n, s, precision):
    """The restated plan of the call, asserted to be in the regime REGIMES records and to size the library's workspace."""
    cfg, _, mlp, _, _ = model(layout, size)
    kind = KIND_OF[precision]
    pl = wgrad_plan.plan(cfg, n * s, kind)
    got = (pl.large_budget, pl.regime('large'), pl.regime('views'), pl.regime('small'))
    assert got == REGIMES[(layout, size[1], n * s)][kind], (layout, size, n * s, kind, got)
    assert mlp.backward_workspace_floats(n, s) == wgrad_plan.workspace_floats(cfg, n * s)
    return pl


def upstream(n, s, blocks, seed):
    """random d_sigma / d_rgb on the real samples of the wave blocks `blocks` (None: everywhere), exactly zero elsewhere"""
    total = n * s
    if blocks is None:
        index = torch.arange(total)
    else:
        index = (torch.as_tensor(blocks, dtype=torch.int64)[:, None] * 32 + torch.arange(32)).reshape(-1)
        index = index[index < total]
    rng = numpy.random.RandomState(seed)
    g_sigma, g_rgb = torch.zeros(total, 1), torch.zeros(total, 3)
    g_sigma[index] = torch.from_numpy(rng.standard_normal((index.numel(), 1)).astype(numpy.float32))
    g_rgb[index] = torch.from_numpy(rng.standard_normal((index.numel(), 3)).astype(numpy.float32))
    return g_sigma.reshape(n, s, 1), g_rgb.reshape(n, s, 3), index


def compare(got, want, names, precision, tag):
    gate_m, gate_2 = GATES[precision]
    worst_m, worst_2, bad = 0.0, 0.0, {}
    for name, g in zip(names, got):
        w = want[name]
        assert bool(torch.isfinite(g).all()), (tag, name)
        if float(w.abs().max()) == 0:
            assert float(g.abs().max()) == 0, (tag, name)
            continue
        m, l2 = rel_to_max(g, w), rel_l2(g, w)
        worst_m, worst_2 = max(worst_m, m), max(worst_2, l2)
        if not (m <= gate_m and l2 <= gate_2):
            bad[name] = (m, l2)
    seen = WORST.setdefault(precision, [0.0, 0.0])
    seen[0], seen[1] = max(seen[0], worst_m), max(seen[1], worst_2)
    util.observe(f'wgrad_plans/{tag}', f'gradients {worst_m:.1e} of max [{gate_m:.1e}], rel L2 {worst_2:.1e} [{gate_2:.1e}]; '
                 f'worst of {precision} so far {seen[0]:.1e}, {seen[1]:.1e}')
    assert not bad, (tag, bad)


def run_case(layout, size, n, s, precision, probe, seed=5):
    """One forward_train and one backward in `precision` with the upstream confined to the plan's probe blocks (or dense), every
    parameter gradient against float64 from the kernel's own saved activations and masks of the blocks that carry upstream."""
    cfg, sd, mlp, shapes, names = model(layout, size)
    total = n * s
    pl = plan_in_its_regime(layout, size, n, s, precision)
    blocks = wgrad_plan.probe_blocks(pl) if probe else None
    if probe:
        assert len(blocks) <= wgrad_plan.PROBE_MAX_BLOCKS and blocks[-1] == -(-total // 32) - 1
    _, _, inputs, _ = fused_case(layout, size, n, s)
    dev = [t.to(DEV) for t in inputs]
    g_sigma, g_rgb, index = upstream(n, s, blocks, seed)
    s8 = precision.endswith('s8')
    base = precision[:-2] if s8 else precision
    sigma, rgb, saved = mlp.forward_train(*dev, P[base])
    if KIND_OF[precision] == 'fp32':
        dec, mode = decode_fused32(saved, cfg, total, blocks), rr.EXACT
    else:
        mode = rr.MODES[FUSED_MODES[precision]]
        dec = decode_fused(saved, cfg, total, mode.fmt == 'bf16', blocks)
    assert torch.equal(dec['samples'], index)
    if s8:        # the s8 forward saves h_1 .. h_D-1 as e4m3, which the decoder does not read: the 16-bit records with mode.x8
        del saved
        sigma, rgb, saved = mlp.forward_train(*dev, P[precision])
    got = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes, P[precision])
    got = [g.cpu() for g in got]
    pick = index.to(DEV)
    sigma_p, rgb_p = sigma.reshape(-1, 1)[pick].cpu(), rgb.reshape(-1, 3)[pick].cpu()
    del saved, sigma, rgb, dev
    if total > 100000:                       # (about 3 GB of saved activations and as much workspace)
        torch.cuda.empty_cache()
    def reference(rows):
        """float64 gradients from the decoded rows `rows` (a bool mask over dec['samples'])"""
        part = {k: ([t[rows] for t in v] if isinstance(v, list) else v[rows]) for k, v in dec.items()}
        return reference_grads(sd, cfg, fused_records(sd, cfg, part, mode), sigma_p[rows], rgb_p[rows],
                               g_sigma.reshape(-1, 1)[index][rows], g_rgb.reshape(-1, 3)[index][rows], mode)

    kind = 'probe' if probe else 'dense'
    tag = f'{kind}/{layout}/{size[0]}x{size[1]}/{n}x{s}/{precision}'
    compare(got, reference(torch.ones(index.numel(), dtype=torch.bool)), names, precision, tag)
    return {'plan': pl, 'blocks': blocks, 'got': got, 'names': names, 'samples': index, 'reference': reference, 'tag': tag}


# ------------------------------------------------------------------------------------------- a: the restatement is the library's
@pytest.mark.parametrize('size', [WIDE, NARROW])
@pytest.mark.parametrize('layout', ['main', 'ptsaug', 'viewsaug'])
def test_restated_workspace_equals_the_librarys(layout, size):
    cfg, _, mlp, _, _ = model(layout, size)
    for total in sorted(set(SWEEP) | {n * s for n, s in SIZES}):
        assert mlp.backward_workspace_floats(total, 1) == wgrad_plan.workspace_floats(cfg, total), total
    for n, s in SIZES:
        assert mlp.backward_workspace_floats(n, s) == wgrad_plan.workspace_floats(cfg, n * s), (n, s)


def test_the_cases_reach_every_regime():
    """at least one empty chunk in the fp32 small class, in the 16-bit small class and in the 64-chunk views job; the budgets 64,
    an intermediate value and 256; unequal chunk counts in the s8 plans"""
    seen = {(kind, cls): set() for kind in wgrad_plan.KINDS for cls in ('large', 'views', 'small')}
    budgets = set()
    for (layout, width, total), kinds in REGIMES.items():
        for kind, (budget, large, views, small) in kinds.items():
            if width == 256:
                budgets.add(budget)
            for cls, regimes in (('large', large), ('views', views), ('small', small)):
                seen[(kind, cls)].update(regimes)
    assert any(e > 0 for _, _, e in seen[('fp32', 'small')]) and any(e > 0 for _, _, e in seen[('f16', 'small')])
    assert any(c == 64 and e > 0 for c, _, e in seen[('fp32', 'views')]) and any(c == 64 and e > 0 for c, _, e in seen[('f16', 'views')])
    assert 64 in budgets and 256 in budgets and any(64 < b < 256 for b in budgets)
    assert {(layout, width, n * s) for layout, (_, width, _), n, s in CASES} == set(REGIMES)
    for n, s in S8_CASES:
        assert len({c for c, _, _ in REGIMES[('main', 256, n * s)]['f16s8'][1]}) > 1


# ----------------------------------------------------------------------------------------------------------- c: boundary probe
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('layout,size,n,s', CASES)
def test_boundary_probe_against_float64(layout, size, n, s, precision):
    run_case(layout, size, n, s, precision, probe=True)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('layout,size,n,s', [('main', WIDE, 50, 68), ('main', WIDE, 165, 200), ('main', NARROW, 342, 192)])
def test_boundary_probe_sees_a_lost_block(layout, size, n, s, precision):
    """The instrument on the device's own operands: a reference that LACKS one probe block -- what a chunk that lost it would have
    summed -- is further from the kernel's gradients than the case's gate, in every weight-gradient tensor and for every probe
    block.  (tests/test_wgrad_plan_host.py shows more than 10x the widest gate for operands of ideal statistics; the real ones,
    with ReLU-gated samples and density gradients only where sigma > 0, are asked for the gate itself.)"""
    case = run_case(layout, size, n, s, precision, probe=True)
    gate = GATES[precision][0]
    least = (float('inf'), None, None)
    for b in case['blocks']:
        want = case['reference'](case['samples'] // 32 != b)
        for name, g in zip(case['names'], case['got']):
            if name.endswith('.weight'):
                least = min(least, (rel_to_max(g, want[name]), name, b))
    util.observe(f'wgrad_plans/lost_block/{case["tag"]}', f'least movement {least[0]:.1e} of max ({least[1]}, block {least[2]}) [> {gate:.1e}]')
    assert least[0] > gate, least


# ------------------------------------------------------------------------------------------------------------ d: dense upstream
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('layout,size,n,s', DENSE_CASES)
def test_dense_upstream_against_float64(layout, size, n, s, precision):
    run_case(layout, size, n, s, precision, probe=False)


# ----------------------------------------------------------------------------------------------------------------- e: s8 modes
@pytest.mark.parametrize('precision', ['f16s8', 'bf16s8'])
@pytest.mark.parametrize('n,s', S8_CASES)
def test_s8_boundary_probe_with_unequal_chunk_counts(n, s, precision):
    pl = run_case('main', WIDE, n, s, precision, probe=True)['plan']
    trunk ={j.chunks for j in pl.of_class('large')}
    assert len(trunk) > 1, trunk                       # the spare redistribution (mlp_backward.hip:1152-1172)
    assert sum(j.x8 for j in pl.jobs) == 7             # h_1 .. h_7 as e4m3


# ---------------------------------------------------------------------------------------------------- f: accumulating backward
@pytest.mark.parametrize('precision,n,s', [('fp32', 50, 68), ('f16', 50, 68), ('f16', 193, 256)])
def test_accumulating_backward_with_empty_chunks(precision, n, s):
    """backward(into=...) through the reduction's read-modify-write: 3400 samples (fp32: the small and views jobs end in an empty
    chunk; the 16-bit plan has none there) and, for the 16-bit plan, 49 408 (20 empty small chunks)."""
    pl = plan_in_its_regime('main', WIDE, n, s, precision)
    assert any(j.empty_chunks for j in pl.of_class('small')) or (precision, n * s) == ('f16', 3400)
    cfg, sd, inputs, (g_sigma, g_rgb) = fused_case('main', WIDE, n, s)
    accumulate_check(cfg, sd, inputs, g_sigma, g_rgb, P[precision], f'wgrad_plans/into/{n}x{s}/{precision}')
