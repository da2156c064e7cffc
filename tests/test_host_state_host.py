"""The library's per-stream and per-device host state (csrc/host_state.h: the (device, stream) table, its cap, the per-device cached
value) driven on the host with fake stream handles under sanitizers: tests/native/host_state_test.cpp."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'simplenerf_amd', 'csrc')


@pytest.mark.parametrize('sanitizers, options', [
    (['-fsanitize=thread'], {'TSAN_OPTIONS': 'halt_on_error=1'}),
    (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], {'ASAN_OPTIONS': 'detect_leaks=0'}),
], ids=['thread', 'address_undefined'])
def test_tables_on_the_host_under_sanitizers(tmp_path, sanitizers, options):
    """8 threads x 64 keys x 4 000 find-or-create calls mixed with inserts of fresh keys get one pointer per key, and it still
    addresses the same object after 1 000 further inserts; the key's mutex is recursive; two threads incrementing a plain int of one
    State 100 000 times each under that State's lock alone sum exactly and the thread sanitizer has nothing to say (what lets the
    side streams and the scratch blocks do without mutexes of their own); the first 64 keys that ask are granted, the 65th refused,
    a granted key is granted again, a failed set-up gives its slot back; the per-device value is computed until one success is
    published, again after a failure, and every time for ordinals beyond the table.  (States are never freed: no leak check.)"""
    exe = str(tmp_path / 'host_state_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-pthread', *sanitizers,
                        os.path.join(REPO, 'tests', 'native', 'host_state_test.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **options))
    assert r.returncode == 0 and 'host_state_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_each_piece_of_host_state_has_one_owner():
    """The three keyed tables and two mutexes that used to sit in api.hip, render.hip and mlp_generic.hip are gone, the lock carries
    a typed state, and api.hip has its includes at the top."""
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(('.hip', '.h')):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for gone in ('g_side', 'g_arena', 'g_stream_locks', 'void* mutex'):
            assert gone not in text, (name, gone)
        if name not in ('host_state.hip', 'host_state.h'):
            assert 'hipDeviceGetAttribute' not in text and not re.search(r'std::(recursive_)?mutex g_(?!profile)', text), name
    api = open(os.path.join(CSRC, 'api.hip')).read().splitlines()
    includes = [i for i, line in enumerate(api) if line.startswith('#include')]
    first_code = next(i for i, line in enumerate(api) if line.startswith(('namespace', 'extern')))
    assert includes and max(includes) < first_code
