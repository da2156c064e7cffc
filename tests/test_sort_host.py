"""The library's sorts and mask compaction (csrc/sort.hip, block Q4 of include/simplenerf_hip.h) as far as a machine without a GPU
can hold them: the symbols and their table, the refusals that are decided before anything is enqueued, the workspace queries, the
``sorter`` argument, and csrc/sort_plan.h walked on the host under sanitizers (tests/native/sort_plan_test.cpp)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from simplenerf_amd import _lib, harness, qa

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snerf_sort_workspace_bytes', 'snerf_sort_f32', 'snerf_sort_keys_with_order', 'snerf_compact_workspace_bytes',
         'snerf_compact_f32_pair')
COUNTS = (1, 2, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17, 16384, 16385, 70001, 762048, 1200003, 2292000, 2 ** 25 + 1, 2 ** 31 - 1)


def test_the_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, 'include', 'simplenerf_hip.h')).read()
    declared = set(re.findall(r'\b(snerf_[a-z_0-9]+)\s*\(', header))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r'#define\s+SNERF_ABI_VERSION\s+10\b', header)


def test_refusals_are_decided_without_a_device():
    """Null pointers, a negative count, 2^31, key_bits 0 and 33: SNERF_E_INVALID with the argument's name, before any launch (the test
    runs where there is no GPU to launch on).  The fake non-null pointers are never dereferenced by a refused call."""
    lib = _lib.load()
    buffer = (ctypes.c_char * 64)()
    p = ctypes.addressof(buffer)

    def refused(status, *words):
        message = lib.snerf_last_error().decode()
        assert status == -1 and all(word in message for word in words), (status, message)

    refused(lib.snerf_sort_f32(None, 8, p, p, None), 'sort_f32', 'values')
    refused(lib.snerf_sort_f32(p, 8, None, p, None), 'sort_f32', 'sorted')
    refused(lib.snerf_sort_f32(p, 8, p + 32, None, None), 'sort_f32', 'workspace')
    refused(lib.snerf_sort_f32(p, -1, p + 32, p, None), 'sort_f32', 'count')
    refused(lib.snerf_sort_f32(p, 2 ** 31, p + 32, p, None), 'sort_f32', 'count')
    refused(lib.snerf_sort_f32(p, 8, p, p, None), 'sort_f32', 'sorted must not be values')
    for k, name in enumerate(('keys', 'sorted_keys', 'order', 'workspace')):
        args = [p, p + 32, p + 16, p + 48]
        args[k] = None
        refused(lib.snerf_sort_keys_with_order(args[0], 8, 22, args[1], args[2], args[3], None), 'sort_keys_with_order', name)
    refused(lib.snerf_sort_keys_with_order(p, 8, 0, p + 32, p, p, None), 'sort_keys_with_order', 'key_bits 0')
    refused(lib.snerf_sort_keys_with_order(p, 8, 33, p + 32, p, p, None), 'sort_keys_with_order', 'key_bits 33')
    refused(lib.snerf_sort_keys_with_order(p, -1, 22, p + 32, p, p, None), 'sort_keys_with_order', 'count')
    refused(lib.snerf_sort_keys_with_order(p, 2 ** 31, 22, p + 32, p, p, None), 'sort_keys_with_order', 'count')
    for k, name in enumerate(('a or b', 'a or b', 'mask', 'a_kept', 'a_kept', 'kept is NULL', 'workspace')):
        args = [p, p, p, p + 32, p + 48, p + 16, p]
        args[k] = None
        refused(lib.snerf_compact_f32_pair(args[0], args[1], args[2], 8, args[3], args[4], args[5], args[6], None), 'compact_f32_pair', name)
    refused(lib.snerf_compact_f32_pair(p, p, p, -1, p, p, p, p, None), 'compact_f32_pair', 'count')
    refused(lib.snerf_compact_f32_pair(p, p, p, 2 ** 31, p, p, p, p, None), 'compact_f32_pair', 'count')
    # an empty sort is done before it looks at a pointer
    assert lib.snerf_sort_f32(None, 0, None, None, None) == 0
    assert lib.snerf_sort_keys_with_order(None, 0, 22, None, None, None, None) == 0


def test_workspace_queries():
    lib = _lib.load()
    for bits in (1, 8, 9, 22, 32):
        sizes = [lib.snerf_sort_workspace_bytes(n, bits) for n in COUNTS]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (bits, sizes)
        assert all(size >= 8 * n + 4 * 256 * ((n + 2047) // 2048) for size, n in zip(sizes, COUNTS))    # two buffers and the counters
    sizes = [lib.snerf_compact_workspace_bytes(n) for n in COUNTS]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, sizes
    # fewer bits never need more scratch; what the sorts refuse needs none
    assert lib.snerf_sort_workspace_bytes(2292000, 22) <= lib.snerf_sort_workspace_bytes(2292000, 32)
    for n, bits in ((0, 32), (-1, 32), (2 ** 31, 32), (100, 0), (100, 33)):
        assert lib.snerf_sort_workspace_bytes(n, bits) == 0
    for n in (0, -1, 2 ** 31):
        assert lib.snerf_compact_workspace_bytes(n) == 0


def test_an_unknown_sorter_is_refused_by_name():
    depth = torch.zeros((16, 16), dtype=torch.float32)
    for call in (lambda: qa.depth_metrics(depth, depth, sorter='nonsense'),
                 lambda: qa.visibility_mask(depth[None], depth, None, None, None, sorter='nonsense'),
                 lambda: harness.evaluate_frames(None, {}, [], 'cpu', sorter='nonsense')):
        with pytest.raises(RuntimeError, match="sorter: expected 'torch' or 'library', got 'nonsense'"):
            call()
    # both names reach the checks that follow
    for sorter in qa.SORTERS:
        with pytest.raises(RuntimeError, match='gt_depth: expected a tensor on the GPU'):
            qa.depth_metrics(depth, depth, sorter=sorter)


def test_ops_refuse_what_they_cannot_sort():
    from simplenerf_amd import ops

    class Stub(torch.Tensor):
        """A host tensor that claims to live on the GPU: reaches the checks that follow the device check."""
        is_cuda = True

    def stub(shape, dtype):
        return torch.zeros(shape, dtype=dtype).as_subclass(Stub)

    with pytest.raises(RuntimeError, match='x: expected a tensor on the GPU'):
        ops.sort_values(torch.zeros(4))
    with pytest.raises(RuntimeError, match='x: expected float32, got torch.float64'):
        ops.sort_values(stub((4,), torch.float64))
    with pytest.raises(RuntimeError, match=r'x: expected a flat tensor, got shape \(2, 2\)'):
        ops.sort_values(stub((2, 2), torch.float32))
    with pytest.raises(RuntimeError, match='keys: expected int32, got torch.int64'):
        ops.sort_keys_with_order(stub((4,), torch.int64))
    for bits in (0, 33, 2.5, True):
        with pytest.raises(RuntimeError, match='key_bits: expected 1..32'):
            ops.sort_keys_with_order(stub((4,), torch.int32), bits)
    with pytest.raises(RuntimeError, match=r'b: expected shape \(4,\), got \(5,\)'):
        ops.compact_pair(stub((4,), torch.float32), stub((5,), torch.float32), stub((4,), torch.bool))
    with pytest.raises(RuntimeError, match='mask: expected bool or uint8, got torch.float32'):
        ops.compact_pair(stub((4,), torch.float32), stub((4,), torch.float32), stub((4,), torch.float32))


def test_plan_on_the_host_under_sanitizers(tmp_path):
    """tests/native/sort_plan_test.cpp: the key map is strictly monotone and inverts, NaNs are last and canonical; for every count the
    tiles cover [0, count) once, the counter index is a bijection, the workspace regions are aligned, disjoint and inside the reported
    size, and for 1..4 passes the last write goes to the caller's output.  AddressSanitizer + UBSan, no GPU."""
    exe = str(tmp_path / 'sort_plan_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(REPO, 'tests', 'native', 'sort_plan_test.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 0 and 'sort_plan_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
