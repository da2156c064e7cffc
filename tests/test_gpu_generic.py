"""MLP shapes outside the fused kernels' set (VERDICT r3 "next" #9): any points_net_width / views_net_width, views_net_depth
> 1, any depth -- everything the reference's MLP.__init__ builds (src/models/SimpleNeRF01.py:567-609) except
predict_visibility -- run on the layered fp32 path (csrc/mlp_generic.hip: one strided fp32-MFMA GEMM per Linear layer,
activations in memory) behind the same C ABI and the same model class.  Forward against the oracle at the fp32 parity
tolerances, gradients against the oracle's autograd."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import util
from tests.test_gpu_grads import GRAD_TOL, rel_l2, rel_to_max

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (layout kwargs, depth, width, views width, views depth)
SHAPES = [
    ({}, 8, 512, 256, 1),                                                   # the 512-wide trunk no register tile holds
    ({}, 4, 64, 32, 2),                                                     # narrow, two views layers
    ({}, 6, 96, 48, 3),                                                     # widths off the 32-tile grid, skip layer present
    ({'use_view_dirs': False, 'view_dependent_rgb': False}, 3, 160, 0, 1),  # views-augmentation layout (no views head)
    ({'sigma_pe_degree': 3}, 8, 64, 64, 2),                                 # points-augmentation layout
    ({}, 8, 256, 128, 2),                                                   # a fused WIDTH with views_net_depth 2
]


def case(index, n=5, s=37):
    kwargs, depth, width, vwidth, vdepth = SHAPES[index]
    cfg = synth.mlp_config(64, depth=depth, width=width, views_width=vwidth, views_depth=vdepth, **kwargs)
    sd = synth.synth_state_dict(util.mlp_param_shapes(cfg), 40 + index, 30.0, 0.5)
    rng = numpy.random.RandomState(index)
    o = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    d = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(numpy.float32))
    v = d / d.norm(dim=1, keepdim=True)
    z = torch.from_numpy(numpy.sort(rng.uniform(0, 1, (n, s)).astype(numpy.float32), axis=1))
    noise = torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32))
    g_sigma = torch.from_numpy(rng.standard_normal((n, s, 1)).astype(numpy.float32))
    g_rgb = torch.from_numpy(rng.standard_normal((n, s, 3)).astype(numpy.float32))
    return cfg, sd, (o, d, v, z, noise), (g_sigma, g_rgb)


def samples_on_a_relu_threshold(sd, cfg, pts, view_dirs, noise, margin=2e-6):
    """bool (N,S): samples with a ReLU pre-activation (any hidden unit of any layer, or the density) within `margin` of zero,
    evaluated in float64 with the oracle's building blocks.  Two fp32 evaluations may gate such a unit differently; the
    gradient comparison leaves these samples out ON BOTH SIDES (their upstream gradients are zeroed) instead of widening its
    tolerance for everything else."""
    import torch.nn.functional as F
    p = {k: torch.from_numpy(a).double() for k, a in sd.items()}
    flat = pts.reshape(-1, 3).double()
    enc = oracle.pos_encode(flat, cfg['points_positional_encoding_degree'])
    lay = oracle.mlp_layout(p, '')
    trunk_in = enc[:, :lay['pts_in']]
    h, closest = trunk_in, torch.full((flat.shape[0],), float('inf'), dtype=torch.float64)
    for i in range(lay['depth']):
        pre = F.linear(h, p[f'pts_linears.{i}.weight'], p[f'pts_linears.{i}.bias'])
        closest = torch.minimum(closest, pre.abs().min(1)[0])
        h = F.relu(pre)
        if i == oracle.SKIP_AFTER_LAYER:
            h = torch.cat([trunk_in, h], -1)
    head = F.linear(h, p['pts_output_linear.weight'], p['pts_output_linear.bias'])
    closest = torch.minimum(closest, (head[:, 0] + noise.reshape(-1).double()).abs())
    if lay['view_dependent']:
        feature = torch.cat([F.linear(h, p['feature_linear.weight'], p['feature_linear.bias']), enc[:, lay['pts_in']:]], 1)
        views = view_dirs[:, None].expand(pts.shape).reshape(-1, 3).double()
        hv = torch.cat([feature, oracle.pos_encode(views, cfg['views_positional_encoding_degree'])], -1)
        for i in range(lay['views_depth']):
            pre = F.linear(hv, p[f'views_linears.{i}.weight'], p[f'views_linears.{i}.bias'])
            closest = torch.minimum(closest, pre.abs().min(1)[0])
            hv = F.relu(pre)
    return (closest < margin).reshape(pts.shape[:2])


@pytest.mark.parametrize('index', range(len(SHAPES)))
@pytest.mark.parametrize('n,s', [(5, 37), (1, 1), (9, 64)])
def test_layered_mlp_matches_the_oracle(index, n, s):
    cfg, sd, inputs, (g_sigma, g_rgb) = case(index, n, s)
    o, d, v, z, noise = inputs
    risky = samples_on_a_relu_threshold(sd, cfg, oracle.ray_points(o, d, z), v, noise)
    assert float(risky.float().mean()) < 0.25      # (observed: up to 3 % of the samples of the 512 x 8 MLP, 4096 gated units each)
    g_sigma, g_rgb = g_sigma * (~risky)[..., None], g_rgb * (~risky)[..., None]
    params = {k: torch.from_numpy(a).clone().requires_grad_(True) for k, a in sd.items()}
    ref = oracle.run_mlp(params, '', cfg, oracle.ray_points(o, d, z), v if cfg['use_view_dirs'] else None, None, noise)
    ((ref['sigma'] * g_sigma).sum() + (ref['rgb'] * g_rgb).sum()).backward()
    plist = synth.abi_param_list({k: torch.from_numpy(a).to(DEV) for k, a in sd.items()})
    mlp = ops.PackedMlp(cfg, DEV)
    assert mlp.num_params == len(plist)
    mlp.pack(plist)
    dev = [t.to(DEV) for t in inputs]
    sigma_eval, rgb_eval = mlp.forward(*dev)
    sigma, rgb, saved = mlp.forward_train(*dev)
    assert torch.equal(sigma, sigma_eval) and torch.equal(rgb, rgb_eval)          # the same kernels, with and without keeping
    assert util.rel_linf(sigma, ref['sigma']) < 1e-5 and util.linf(rgb, ref['rgb']) < 1e-5
    shapes = [tuple(p.shape) for p in plist]
    grads = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes)
    again = mlp.backward(saved, sigma, rgb, g_sigma.to(DEV), g_rgb.to(DEV), shapes)
    names = synth.abi_param_list({k: k for k in sd})
    worst, worst_l2 = 0.0, 0.0
    for name, got, twice in zip(names, grads, again):
        assert torch.equal(got, twice), name                                       # fixed-order reductions
        want = params[name].grad
        assert got.shape == want.shape
        if float(want.abs().max()) > 0:
            worst, worst_l2 = max(worst, rel_to_max(got, want)), max(worst_l2, rel_l2(got, want))
    # the same gate as the fused fp32 kernels (tests/test_gpu_grads.py): relative to each tensor's largest entry -- a sample
    # whose pre-activation sits within an ulp of zero flips its ReLU gate between two fp32 evaluations
    util.observe(f'layered/{index}/{n}x{s}', f'sigma rel {util.rel_linf(sigma, ref["sigma"]):.1e} [1e-5], rgb {util.linf(rgb, ref["rgb"]):.1e} [1e-5], '
                 f'worst gradient error / largest entry {worst:.1e} [{GRAD_TOL}], rel L2 {worst_l2:.1e}')
    assert worst < GRAD_TOL


@pytest.mark.parametrize('index', range(len(SHAPES)))
def test_layered_gradients_of_a_large_call_equal_the_sum_over_its_parts(index):
    """13 440 samples (70 rays x 192): the forward against the oracle, and the parameter gradients against the SUM of the same
    path's gradients over ten 7-ray parts -- what changes with the size (tile grid, the split of the weight-gradient products
    over the samples, bias column sums) is exercised, while every sample keeps the ReLU gates of its own forward.  (Against the
    oracle's autograd a call of this size cannot be gated tightly: among its 7-55 M pre-activations a few sit within an ulp of
    zero, their gates flip between two fp32 evaluations, and one flipped sample moves entries of a gradient tensor by ~1/sqrt(N)
    of its largest -- 2e-3 to 6e-3 observed here, with the arithmetic exact to 1e-6 at 185 samples above.)"""
    cfg, sd, inputs, (g_sigma, g_rgb) = case(index, 70, 192)
    o, d, v, z, noise = inputs
    ref = oracle.run_mlp({k: torch.from_numpy(a) for k, a in sd.items()}, '', cfg, oracle.ray_points(o, d, z),
                         v if cfg['use_view_dirs'] else None, None, noise)
    plist = synth.abi_param_list({k: torch.from_numpy(a).to(DEV) for k, a in sd.items()})
    mlp = ops.PackedMlp(cfg, DEV)
    mlp.pack(plist)
    shapes = [tuple(p.shape) for p in plist]
    dev = [t.to(DEV) for t in inputs]
    gs, gc = g_sigma.to(DEV), g_rgb.to(DEV)
    sigma, rgb, saved = mlp.forward_train(*dev)
    assert util.rel_linf(sigma, ref['sigma']) < 1e-5 and util.linf(rgb, ref['rgb']) < 1e-5
    whole = mlp.backward(saved, sigma, rgb, gs, gc, shapes)
    parts = [torch.zeros_like(g) for g in whole]
    for lo in range(0, 70, 7):
        cut = slice(lo, lo + 7)
        sg, cl, sv = mlp.forward_train(*[t[cut].contiguous() for t in dev])
        assert torch.equal(sg, sigma[cut]) and torch.equal(cl, rgb[cut])
        for acc, g in zip(parts, mlp.backward(sv, sg, cl, gs[cut].contiguous(), gc[cut].contiguous(), shapes)):
            acc += g
    worst = max(rel_to_max(a, b) for a, b in zip(whole, parts) if float(b.abs().max()) > 0)
    util.observe(f'layered/{index}/70x192', f'gradients of the whole call vs the sum over ten parts: {worst:.1e} of the largest entry [1e-5]')
    assert worst < 1e-5


def test_two_threads_on_two_streams_each_grow_their_own_scratch():
    """The inference forward's scratch belongs to the (device, stream) it runs on: two threads, each on a non-default stream of its
    own, each with its own layered MLP, run a 5-ray x 37-sample call and then a 9-ray x 64-sample one (the stream's block grows once),
    five times over; every result is bit-equal to the same call made alone on the default stream."""
    import threading
    mlps, calls = [], []
    for index in (1, 2):
        cfg, sd, _, _ = case(index)
        mlp = ops.PackedMlp(cfg, DEV)
        mlp.pack(synth.abi_param_list({k: torch.from_numpy(a).to(DEV) for k, a in sd.items()}))
        mlps.append(mlp)
        calls.append([[t.to(DEV) for t in case(index, n, s)[2]] for n, s in ((5, 37), (9, 64))])
    alone = [[mlp.forward(*inputs) for inputs in mine] for mlp, mine in zip(mlps, calls)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    results, errors = [[], []], []
    start = threading.Barrier(2)

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                assert torch.cuda.current_stream(0) == streams[i] != torch.cuda.default_stream(0)
                start.wait()
                for _ in range(5):
                    results[i].append([mlps[i].forward(*inputs) for inputs in calls[i]])
        except BaseException as error:       # (reported below, in the test's thread)
            errors.append(error)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        assert len(results[i]) == 5
        for rep, got in enumerate(results[i]):
            for call, ((sigma, rgb), (want_sigma, want_rgb)) in enumerate(zip(got, alone[i])):
                assert torch.equal(sigma, want_sigma) and torch.equal(rgb, want_rgb), (i, rep, call)


def test_the_fp16_modes_are_refused_for_layered_shapes_not_silently_run_in_fp32():
    cfg, sd, inputs, _ = case(1)
    mlp = ops.PackedMlp(cfg, DEV)
    mlp.pack(synth.abi_param_list({k: torch.from_numpy(a).to(DEV) for k, a in sd.items()}))
    with pytest.raises(Exception, match='fp32'):
        mlp.forward(*[t.to(DEV) for t in inputs], ops.PRECISION_F16)


@pytest.mark.parametrize('width,views_width,views_depth', [(512, 256, 1), (64, 64, 2)])
def test_model_with_a_layered_shape_renders_and_trains_like_the_oracle(width, views_width, views_depth):
    """config 2 with other MLP shapes through the drop-in model: eval render against the oracle at north_star's tolerances,
    then a training-mode forward + backward against the oracle's autograd."""
    cfg = synth.make_configs('config2')
    for key in ('coarse_mlp', 'fine_mlp'):
        cfg['model'][key].update(points_net_width=width, views_net_width=views_width, views_net_depth=views_depth)
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 11, 150.0, 4.0).items()}
    for k in list(sd):                                  # consistent geometry: fine = coarse (see tests/test_gpu_model.py)
        if k.startswith('coarse_model.'):
            sd['fine_model.' + k[len('coarse_model.'):]] = sd[k].clone()
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 190000, 96)
    cpu_batch = {k: v.cpu() for k, v in batch.items()}
    with torch.no_grad():
        out = model(batch, retraw=True)
        ref = oracle.render(sd, cfg, cpu_batch, training=False, retraw=True)
    assert float(ref['acc_fine'].mean()) > 0.05
    for k in ('rgb_coarse', 'acc_coarse', 'weights_coarse', 'raw_rgb_coarse'):
        assert util.linf(out[k], ref[k]) <= 1e-4, k
    assert util.linf(out['depth_ndc_coarse'], ref['depth_ndc_coarse']) <= 1e-3
    moved = (out['z_vals_fine'].cpu() - ref['z_vals_fine']).abs().max(1)[0] > 1e-5
    over = (out['rgb_fine'].cpu() - ref['rgb_fine']).abs().max(1)[0] > 1e-4
    assert not (over & ~moved).any() and float(over.float().mean()) <= 0.05
    # training-mode forward + backward (no jitter, no noise) against the oracle's autograd.  The fine depths are resampled from
    # each side's own coarse weights (0.1 % of them sit on sample_pdf's rounding-decided threshold), hence 1e-2 here; the
    # kernels themselves are held to 1e-4 by the MLP-level test above.
    model.train()
    model.set_random_draws({})
    got = model(batch)
    (got['rgb_fine'].sum() + got['rgb_coarse'].sum() + got['depth_ndc_coarse'].sum()).backward()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    want = oracle.render(params, cfg, cpu_batch, training=True, rand_per_chunk=[{}])
    (want['rgb_fine'].sum() + want['rgb_coarse'].sum() + want['depth_ndc_coarse'].sum()).backward()
    worst = 0.0
    for name, p in model.named_parameters():
        g = params[name].grad
        if g is not None and float(g.abs().max()) > 0:
            worst = max(worst, rel_l2(p.grad, g))
    util.observe(f'layered/model/{width}x{views_width}x{views_depth}', f'worst parameter-gradient rel L2 {worst:.1e} [1e-2]')
    assert worst < 1e-2, worst
