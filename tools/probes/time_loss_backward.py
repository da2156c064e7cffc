"""Time snerf_loss_backward for the table of the nine shipped losses (11 terms, the shapes of tests/golden/losses_full.npz
scaled to 4096 rows) through the C ABI of a given library build: HIP events around 100 back-to-back launches, warm, median of
40.  Run it alternately on the parent commit's library and this one's (profiles/r08_time_loss_backward.jsonl).

    python tools/probes/time_loss_backward.py LIB {old|new} TAG OUT.jsonl

``old`` = struct snerf_loss_term of ABI 9 (no d_target tail), ``new`` = ABI 10.  A TAG ending in ``+01`` (new only) times the
table of all thirteen losses instead: 16 terms, three of them two-sided."""
import ctypes, json, os, statistics, sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from simplenerf_amd import _lib  # noqa: E402

lib_path, layout, tag, out_path = sys.argv[1:5]
c_void_p, c_int = ctypes.c_void_p, ctypes.c_int
fields = list(_lib.LossTerm._fields_)      # struct snerf_loss_term as the header in the tree has it
if layout == 'old':
    fields = fields[:[name for name, _ in fields].index('d_target')]      # ABI 9: before the d_target tail was appended


class Term(ctypes.Structure):
    _fields_ = fields


lib = ctypes.CDLL(lib_path)
lib.snerf_loss_workspace_bytes.restype = ctypes.c_longlong
lib.snerf_loss_forward.argtypes = [ctypes.POINTER(Term), c_int, c_int, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]
lib.snerf_loss_backward.argtypes = [ctypes.POINTER(Term), c_int, c_int, ctypes.c_longlong, c_void_p, c_void_p, c_void_p]
assert lib.snerf_abi_version() == (10 if layout == 'new' else 9), lib.snerf_abi_version()
dev = 'cuda:0'
n, n_px = 4096, 3584
gen = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.rand(s, device=dev, generator=gen)
T = {k: rnd(n, 3) for k in ('rgb_c', 'rgb_f', 'pa_rgb', 'va_rgb', 'target')}
T.update({k: 4 + rnd(n) for k in ('d_c', 'd_f', 'pa_d', 'va_d', 'sparse')})
m_px = (torch.arange(n, device=dev) < n_px)
m_sd = ~m_px
better = [m_px & (rnd(n) < 0.4) for _ in range(3)]
u8 = lambda m: m.to(torch.uint8).contiguous()
m_px8, m_sd8, better8 = u8(m_px), u8(m_sd), [u8(b) for b in better]
spec = [('rgb_c', 'target', m_px8, m_px8, 0, 1.0), ('rgb_f', 'target', m_px8, m_px8, 0, 1.0), ('d_f', 'sparse', m_sd8, m_sd8, 1, 0.1),
        ('pa_rgb', 'target', m_px8, m_px8, 2, 1.0), ('pa_d', 'sparse', m_sd8, m_sd8, 3, 0.1),
        ('va_rgb', 'target', m_px8, m_px8, 4, 1.0), ('va_d', 'sparse', m_sd8, m_sd8, 5, 0.1),
        ('d_c', 'pa_d', better8[0], m_px8, 6, 0.1), ('d_c', 'va_d', better8[1], m_px8, 7, 0.1),
        ('d_c', 'd_f', better8[2], m_px8, 8, 0.1), ('d_c', 'd_f', m_sd8, m_sd8, 8, 0.1)]
if layout == 'new' and tag.endswith('+01'):      # the thirteen losses: 16 terms, three of them two-sided
    spec += [('d_c', 'pa_d', None, None, 9, 0.1, True), ('d_c', 'va_d', None, None, 10, 0.1, True), ('d_c', 'd_f', None, None, 11, 0.1, True),
             ('d_c', 'sparse', m_px8, m_px8, 12, 0.1), ('d_f', 'sparse', m_px8, m_px8, 12, 0.1)]
groups = max(s[4] for s in spec) + 1
grads = {}
table = (Term * len(spec))()
seen = set()
for i, s in enumerate(spec):
    pred, target, num, den, group, weight = s[:6]
    e = table[i]
    e.pred, e.target = T[pred].data_ptr(), T[target].data_ptr()
    e.numerator_mask = 0 if num is None else num.data_ptr()
    e.denominator_mask = 0 if den is None else den.data_ptr()
    e.channels, e.group, e.weight = (3 if T[pred].dim() == 2 else 1), group, weight
    buf = grads.setdefault(pred, torch.empty_like(T[pred]))
    e.d_pred, e.accumulate = buf.data_ptr(), int(buf.data_ptr() in seen)
    seen.add(buf.data_ptr())
    if len(s) == 7:
        buf = grads.setdefault(target, torch.empty_like(T[target]))
        e.d_target, e.accumulate_target = buf.data_ptr(), int(buf.data_ptr() in seen)
        seen.add(buf.data_ptr())
count = len(spec)
values = torch.empty(count + groups + 1, device=dev)
scales = torch.empty(count, device=dev)
ws = torch.zeros(int(lib.snerf_loss_workspace_bytes()), dtype=torch.uint8, device=dev)
up = torch.zeros(count + groups + 1, device=dev)
up[-1] = 1.0
stream = c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: c_void_p(t.data_ptr())
assert lib.snerf_loss_forward(table, count, groups, n, p(values), p(scales), p(ws), stream) == 0
backward = lambda: lib.snerf_loss_backward(table, count, groups, n, p(scales), p(up), stream)
for _ in range(200):
    assert backward() == 0
torch.cuda.synchronize()
INNER = 100
samples = []
for _ in range(40):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        backward()
    b.record()
    b.synchronize()
    samples.append(a.elapsed_time(b) * 1000.0 / INNER)
rec = {'tag': tag, 'terms': count, 'rows': n, 'us_per_launch_median': statistics.median(samples), 'min': min(samples), 'max': max(samples),
       'inner': INNER, 'samples': len(samples), 'total': float(values[-1]), 'grad_checksum': float(sum(g.double().abs().sum() for g in grads.values()))}
print(json.dumps(rec))
with open(out_path, 'a') as f:
    f.write(json.dumps(rec) + '\n')
