"""The weight-gradient planner of the fused MLP backward, restated in plain Python -- test infrastructure, never imported by the
package.

`plan_workspace` (simplenerf_amd/csrc/mlp_backward.hip:1022-1190) splits every product dW = dY . X^T of a backward call over
workgroups ("chunks") by a plan that depends on the MLP's shape and the number of samples only.  This module restates it, line
for line, for the three plans the library builds -- 'fp32' (fp32 and f16x3), 'f16' (f16 and bf16) and 'f16s8' (the 16-bit modes with
an fp8 saved trunk) -- so that a test can say which regime a size is in (chunks, blocks per chunk, empty chunks of every job) and
assert it.  tests/test_gpu_wgrad_plans.py pins the restatement to the library: the largest of the three totals must equal
`snerf_mlp_backward_workspace_floats` (mlp_backward.hip:1239-1252) at every swept size.

A chunk `c` of a job contracts the wave blocks [c per, min((c + 1) per, B)), per = ceil(B / chunks) (wgrad_kernel,
mlp_backward.hip:288-289; wgrad16_kernel, :574-575); chunks with c per >= B are EMPTY and still write a zero partial, which
reduce_kernel (:933-995) folds.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Tuple

KINDS = ('fp32', 'f16', 'f16s8')
# precision name (ops.PRECISIONS) -> the plan snerf_mlp_backward builds for it (mlp_backward.hip:1279-1293)
KIND_OF = {'fp32': 'fp32', 'f16x3': 'fp32', 'f16': 'f16', 'bf16': 'f16', 'f16s8': 'f16s8', 'bf16s8': 'f16s8'}

SEG_ACC, SEG_POINTS_PE, SEG_VIEWS_PE = 'acc', 'points_pe', 'views_pe'
REGION_TABLE_FLOAT0, REGION_SLOTS, REGION_WORDS = 448, 64, 128        # mlp_backward.hip:193-194
SMALL_JOB_CHUNKS, SMALL_JOB_CHUNKS_FP32 = 192, 256                     # :1004, :1144
MID_BLOCKS = 32                                                        # :1005
LARGE_MIN_BLOCKS = 16                                                  # :1114
PROBE_MAX_BLOCKS = 64

# (rays, samples per ray) at which the device tests hold the plans (tests/test_gpu_wgrad_plans.py names each one's regime), and the
# sample counts at which the restatement is compared with the library's workspace size
SIZES = [(7, 45), (25, 40), (50, 68), (64, 129), (125, 160), (165, 200), (193, 256), (342, 192), (2049, 128)]
SWEEP = range(1, 70001, 37)


# ------------------------------------------------------------------------------------------------------------ MlpPlan's rows
@dataclasses.dataclass(frozen=True)
class Rows:
    """The sizes and tile rows of snerf::MlpPlan that the planner reads (csrc/mlp_plan.h:12-20, :61-85, :99-143)."""
    depth: int
    width: int
    views_width: int
    view_dependent: bool
    sigma_pe: bool
    full_pe: int
    pts_in: int
    extra: int
    views_pe: int

    @property
    def wt(self): return self.width // 32
    @property
    def vt(self): return self.views_width // 32
    def act_pe(self): return 0
    def act_pev(self): return 64
    def act_h(self, l): return 96 + (l - 1) * self.width
    def act_feature(self): return 96 + self.depth * self.width
    def act_hv(self): return 96 + (self.depth + 1) * self.width
    def mask_tiles(self): return self.depth * (self.width // 32) + (self.views_width // 32 if self.view_dependent else 0)
    def act_mask(self): return 96 + (self.depth + 1) * self.width + (self.views_width if self.view_dependent else 0)
    def act_rows(self): return self.act_mask() + 2 * ((self.mask_tiles() + 1) // 2)
    def act16_rows(self): return self.act_mask() + 4 * ((self.mask_tiles() + 1) // 2)
    def grad_y(self, l): return l * self.width
    def grad_feature(self): return self.depth * self.width
    def grad_yv(self): return (self.depth + 1) * self.width
    def grad_head(self): return (self.depth + 1) * self.width + (self.views_width if self.view_dependent else 0)
    def grad_rows(self): return self.grad_head() + 32
    def grad16_rows(self): return self.grad_rows()


def rows_of(cfg: dict) -> Rows:
    """build_plan (csrc/mlp_plan.h:96-144) from an MLP config dict (simplenerf_amd.synth.mlp_config)."""
    view_dep = bool(cfg['view_dependent_rgb'])
    full_pe = 3 + 6 * cfg['points_positional_encoding_degree']
    sigma_pe = 'points_sigma_positional_encoding_degree' in cfg
    pts_in = (2 * cfg['points_sigma_positional_encoding_degree'] + 1) * 3 if sigma_pe else full_pe
    return Rows(depth=cfg['points_net_depth'], width=cfg['points_net_width'], views_width=cfg['views_net_width'] if view_dep else 0,
                view_dependent=view_dep, sigma_pe=sigma_pe, full_pe=full_pe, pts_in=pts_in, extra=full_pe - pts_in if sigma_pe else 0,
                views_pe=3 + 6 * cfg['views_positional_encoding_degree'] if view_dep else 0)


# --------------------------------------------------------------------------------------------------------------------- jobs
@dataclasses.dataclass
class Job:
    """WgradJob (mlp_backward.hip:157-181), the fields the planner sets."""
    name: str
    dy_row0: int
    out_rows: int
    x_row0: int
    in_rows: int
    w_param: int
    w_ld: int
    w_col: int
    b_param: int
    dy_skip: int = 0
    x_kind: str = SEG_ACC
    feat_lo: int = 0
    feat_hi: int = 0
    out_tiles: int = 0
    in_tiles: int = 0
    grad_rows: int = 0
    act_rows: int = 0
    x8: int = 0
    x2_row0: int = 0
    x2_tiles: int = 0
    launched: int = 1
    partial_ld: int = 0
    partial_col0: int = 0
    chunks: int = 1
    blocks: int = 0
    partial_off: int = 0
    bias_off: int = 0

    @property
    def tiles(self) -> int:
        return self.out_tiles * self.in_tiles

    @property
    def per(self) -> int:
        """wave blocks a chunk contracts (mlp_backward.hip:288, :574)"""
        return -(-self.blocks // self.chunks)

    @property
    def empty_chunks(self) -> int:
        """chunks c with c per >= B: ceil(B / per) chunks hold blocks"""
        return self.chunks - -(-self.blocks // self.per)

    @property
    def job_class(self) -> str:
        """'large': the 8 x 8-tile products that share the budget; 'views': the lone 4 x 8 / 4 x 9 job; 'small': heads, encodings
        and every product of a narrow MLP (fewer than 32 tile products)"""
        return 'small' if self.tiles < 32 else 'views' if self.tiles < 64 else 'large'

    def chunk_range(self, c: int) -> Tuple[int, int]:
        """[b0, b1) of chunk c; b0 >= b1: empty"""
        b0 = c * self.per
        return b0, min(b0 + self.per, self.blocks)

    def summary(self) -> Tuple[int, int, int, int, int, int]:
        return self.out_tiles, self.in_tiles, self.chunks, self.per, self.empty_chunks, self.launched


@dataclasses.dataclass
class Plan:
    kind: str
    total_samples: int
    blocks: int                 # wave blocks (32 samples) the chain writes and every job contracts over
    large_budget: int
    jobs: List[Job]
    grads_floats: int
    partial_floats: int
    total_floats: int

    @property
    def real_blocks(self) -> int:
        """wave blocks that hold at least one real sample"""
        return -(-self.total_samples // 32)

    def launched(self) -> List[Job]:
        return [j for j in self.jobs if j.launched]

    def of_class(self, job_class: str) -> List[Job]:
        return [j for j in self.jobs if j.launched and j.job_class == job_class]

    def regime(self, job_class: str) -> List[Tuple[int, int, int]]:
        """sorted distinct (chunks, per, empty chunks) of the launched jobs of a class"""
        return sorted({(j.chunks, j.per, j.empty_chunks) for j in self.of_class(job_class)})


def wave_tile(j: Job) -> Tuple[int, int]:
    """wave_tile (mlp_backward.hip:1008-1013)"""
    ot, it = j.out_tiles, j.in_tiles
    if ot >= 4:
        return ot // 4, it
    if ot == 2:
        return 1, (it // 2 if it >= 2 else 1)
    return 1, (it // 4 if it >= 4 else 1)


def plan(cfg: dict, total_samples: int, kind: str = 'fp32') -> Plan:
    """plan_workspace (mlp_backward.hip:1022-1190)."""
    assert kind in KINDS, kind
    f16, s8 = kind != 'fp32', kind == 'f16s8'
    p = rows_of(cfg)
    blocks = (total_samples + 255) // 256 * 8 if f16 else (total_samples + 127) // 128 * 4               # :1026
    grads_floats = blocks * p.grad_rows() * 32                                                           # :1027
    off = REGION_TABLE_FLOAT0 + REGION_SLOTS * REGION_WORDS                                              # :1028
    jobs: List[Job] = []

    def add(name, dy_row0, out_rows, x_row0, in_rows, w_param, w_ld, w_col, b_param, x_kind=SEG_ACC):   # :1030-1057
        j = Job(name, dy_row0, out_rows, x_row0, in_rows, w_param, w_ld, w_col, b_param)
        if f16:
            j.dy_skip = dy_row0 % 32
            j.dy_row0 = dy_row0 - j.dy_skip
            if x_kind != SEG_ACC:
                tile_row0 = p.act_pe() if x_kind == SEG_POINTS_PE else p.act_pev()
                j.x_kind = x_kind
                j.feat_lo = x_row0 - tile_row0
                j.feat_hi = j.feat_lo + in_rows
                j.x_row0 = tile_row0
                j.in_rows = 64 if x_kind == SEG_POINTS_PE else 32
        j.out_tiles = (j.dy_skip + out_rows + 31) // 32
        j.in_tiles = (j.in_rows + 31) // 32
        j.grad_rows = p.grad16_rows() if f16 else p.grad_rows()
        j.act_rows = p.act16_rows() if f16 else p.act_rows()
        j.blocks = blocks
        j.x8 = 1 if (s8 and p.wt == 8 and x_kind == SEG_ACC and p.act_h(1) <= x_row0 < p.act_h(p.depth)) else 0   # :1052
        if j.x8:
            j.x_row0 = p.act_h(1) + (x_row0 - p.act_h(1)) // 2                                          # :1054
        jobs.append(j)

    d, wd = p.depth, p.width
    add('pts_linears.0', p.grad_y(0), wd, p.act_pe(), p.pts_in, 0, p.pts_in, 0, 1, SEG_POINTS_PE)     # :1060
    for l in range(1, d):                                                                                # :1061-1066
        skip_in = l == 5
        ld = wd + (p.pts_in if skip_in else 0)
        add(f'pts_linears.{l}', p.grad_y(l), wd, p.act_h(l), wd, 2 * l, ld, p.pts_in if skip_in else 0, 2 * l + 1)
        if skip_in:
            add(f'pts_linears.{l}|encoding', p.grad_y(l), wd, p.act_pe(), p.pts_in, 2 * l, ld, 0, -1, SEG_POINTS_PE)
    if p.view_dependent:                                                                                 # :1068-1076
        add('pts_output_linear', p.grad_head(), 1, p.act_h(d), wd, 2 * d, wd, 0, 2 * d + 1)
        add('feature_linear', p.grad_feature(), wd, p.act_h(d), wd, 2 * d + 2, wd, 0, 2 * d + 3)
        ldv = wd + p.extra + p.views_pe
        add('views_linears.0|feature', p.grad_yv(), p.views_width, p.act_feature(), wd, 2 * d + 4, ldv, 0, 2 * d + 5)
        if p.sigma_pe:
            add('views_linears.0|sigma_pe', p.grad_yv(), p.views_width, p.act_pe() + p.pts_in, p.extra, 2 * d + 4, ldv, wd, -1,
                SEG_POINTS_PE)
        add('views_linears.0|views_pe', p.grad_yv(), p.views_width, p.act_pev(), p.views_pe, 2 * d + 4, ldv, wd + p.extra, -1,
            SEG_VIEWS_PE)
        add('views_output_linear', p.grad_head() + 1, 3, p.act_hv(), p.views_width, 2 * d + 6, p.views_width, 0, 2 * d + 7)
    else:                                                                                                # :1078
        add('pts_output_linear', p.grad_head(), 4, p.act_h(d), wd, 2 * d, wd, 0, 2 * d + 1)
    if f16:                                                                                              # the rider merge, :1084-1097
        for host in jobs:
            if host.x_kind != SEG_ACC or host.out_tiles != 4 or host.in_tiles != 8 or host.dy_skip != 0:
                continue
            for rider in jobs:
                if (rider.x_kind != SEG_VIEWS_PE or rider.dy_row0 != host.dy_row0 or rider.out_rows != host.out_rows or
                        rider.dy_skip != 0 or rider.in_tiles != 1 or rider.launched == 0 or host.x2_tiles != 0):
                    continue
                host.x2_row0, host.x2_tiles = rider.x_row0, rider.in_tiles
                rider.launched, rider.partial_col0 = 0, host.in_tiles * 32
                host.in_tiles += rider.in_tiles
                rider.partial_ld = host.in_tiles * 32
    jobs.sort(key=lambda j: -j.tiles)                                                                    # stable, :1099-1101
    large_budget = min(256, max(64, blocks // LARGE_MIN_BLOCKS))                                        # :1115

    def weight(k):                                                                                       # :1127
        return 20 * k.out_tiles + (12 if k.x8 else 20) * k.in_tiles

    tile_of = [wave_tile(j) for j in jobs]
    for j, (no, ni) in zip(jobs, tile_of):                                                               # :1116-1151
        if j.tiles >= 32:
            peers_weight = sum(weight(k) for k, t in zip(jobs, tile_of) if t == (no, ni) and k.tiles >= 32 and k.launched)
            chunks = large_budget * weight(j) // peers_weight                                           # :1133
            if j.tiles < 64 and chunks > blocks // MID_BLOCKS:                                           # :1140-1141
                chunks = min(chunks, max(blocks // MID_BLOCKS, min(64, blocks // 4), 1))
            cap = blocks // 8
        else:
            chunks = SMALL_JOB_CHUNKS if f16 else SMALL_JOB_CHUNKS_FP32                                  # :1145
            cap = blocks // 8
        j.chunks = max(min(chunks, cap), 1)                                                              # :1148-1150

    def member(j, t):                                                                                    # :1159, :1167
        return t == (2, 8) and j.launched and j.tiles >= 32

    members = [j for j, t in zip(jobs, tile_of) if member(j, t)]                                         # the spare, :1154-1172
    spare = large_budget - sum(j.chunks for j in members)
    while len(members) > 1 and spare > 0:
        given = False
        for light in (1, 0):
            for j in members:
                if (j.x8 != 0) != (light != 0):
                    continue
                if spare > 0 and j.chunks < blocks // 8:
                    j.chunks += 1
                    spare -= 1
                    given = True
        if not given:
            break
    for j in jobs:                                                                                       # :1173-1179
        if not j.launched:
            continue
        j.partial_off = off
        off += j.chunks * j.out_tiles * 32 * j.in_tiles * 32
        j.bias_off = off
        off += j.chunks * j.out_tiles * 32
    for rider in jobs:                                                                                   # :1180-1186
        if rider.launched:
            continue
        for host in jobs:
            if host.launched and host.x2_tiles > 0 and host.dy_row0 == rider.dy_row0 and host.x2_row0 == rider.x_row0:
                rider.chunks, rider.partial_off, rider.bias_off = host.chunks, host.partial_off, host.bias_off
    return Plan(kind, total_samples, blocks, large_budget, jobs, grads_floats, off, grads_floats + off)


def host_of(pl: Plan, rider: Job) -> Optional[Job]:
    """the launched job whose partial sums a rider (launched = 0) is a view of"""
    for host in pl.jobs:
        if host.launched and host.x2_tiles > 0 and host.dy_row0 == rider.dy_row0 and host.x2_row0 == rider.x_row0:
            return host
    return None


def workspace_floats(cfg: dict, total_samples: int) -> int:
    """snerf_mlp_backward_workspace_floats (mlp_backward.hip:1249-1251): the largest of the three plans"""
    return max(plan(cfg, total_samples, kind).total_floats for kind in KINDS)


# ------------------------------------------------------------------------------------------------------------- probe blocks
def chunk_boundaries(j: Job, c: int) -> List[int]:
    """first and last block of chunk c and the first block after its end (which may be B: the caller drops what is out of range)"""
    b0, b1 = j.chunk_range(c)
    assert b0 < b1, (j.name, c)
    return [b0, b1 - 1, b1]


def job_probe_chunks(j: Job) -> Tuple[List[int], List[int]]:
    """(boundary chunks: the first and the last non-empty one, middle chunks: one in between)"""
    last = j.chunks - j.empty_chunks - 1
    edge = sorted({0, last})
    middle = [last // 2] if last // 2 not in edge else []
    return edge, middle


def probe_blocks(pl: Plan) -> List[int]:
    """Sorted wave-block indices at which a chunk plan can go wrong: per launched job the first and last block of its first chunk,
    of one middle chunk and of its last non-empty chunk, the first block after each of those chunks, and the call's last block with a
    real sample.  Only blocks that hold a real sample count.  At most PROBE_MAX_BLOCKS: the boundary chunks are always in, the
    middle chunks are added job by job (most chunks first) while they fit."""
    real = pl.real_blocks
    keep = {real - 1}
    middles = []
    for j in pl.launched():
        edge, middle = job_probe_chunks(j)
        for c in edge:
            keep.update(chunk_boundaries(j, c))
        for c in middle:
            middles.append((j.chunks, set(chunk_boundaries(j, c))))
    keep = {b for b in keep if 0 <= b < real}
    assert len(keep) <= PROBE_MAX_BLOCKS, len(keep)
    for _, blocks_ in sorted(middles, key=lambda m: -m[0]):
        more = keep | {b for b in blocks_ if 0 <= b < real}
        if len(more) <= PROBE_MAX_BLOCKS:
            keep = more
    return sorted(keep)
