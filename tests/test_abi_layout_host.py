"""The struct layouts the binding derives from the headers (simplenerf_amd/_cdecl.py) held to the host compiler's:
tests/native/abi_layout_dump.cpp prints sizeof and every field's offsetof.  No device."""
import ctypes
import os
import subprocess

from simplenerf_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_derived_struct_layouts_equal_the_compilers(tmp_path):
    exe = str(tmp_path / 'abi_layout_dump')
    r = subprocess.run(['g++', '-O0', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'),
                        os.path.join(REPO, 'tests', 'native', 'abi_layout_dump.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    sizes, fields = {}, {}
    for line in r.stdout.splitlines():
        words = line.split()
        if words[0] == 'struct':
            sizes[words[1]] = int(words[2])
            fields[words[1]] = []
        else:
            struct, field = words[0].split('.')
            fields[struct].append((field, int(words[1]), int(words[2])))
    assert len(sizes) == 12 and set(sizes) == set(_lib.STRUCTS), set(sizes) ^ set(_lib.STRUCTS)
    for name, cls in _lib.STRUCTS.items():
        assert ctypes.sizeof(cls) == sizes[name], (name, ctypes.sizeof(cls), sizes[name])
        derived = [(field, getattr(cls, field).offset, getattr(cls, field).size) for field, _ in cls._fields_]
        assert derived == fields[name], (name, derived, fields[name])
