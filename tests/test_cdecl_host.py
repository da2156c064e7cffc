"""The reader of the project's headers (simplenerf_amd/_cdecl.py): every form it accepts on a few lines of synthetic header text,
every refusal, and what it finds in the two real headers.  No device, no library."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_ubyte, c_void_p

import pytest

from simplenerf_amd import _cdecl, _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYNTHETIC = '''
/* a block comment with a prototype in it: int snerf_hidden(int x);
   over two lines */
#ifndef GUARD_H
#define GUARD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* snerf_stream_t; // a line comment; int snerf_hidden2(void);
#define SNERF_ROWS 3
#define SNERF_COLS 0x4
enum snerf_kind { SNERF_A = 2, SNERF_B, SNERF_C = -7, SNERF_D, SNERF_E = SNERF_ROWS };
enum { SNERF_FIRST, SNERF_SECOND };
typedef struct snerf_inner {
    long long offset;       /* a comment; with a semicolon */
    int dims[3];
} snerf_inner;
typedef struct snerf_outer {
    const float *a, *b;
    float* const* list;
    const snerf_inner* inner;
    unsigned char flag;
    double scale;
    const float* per_row[SNERF_ROWS];
    snerf_inner grid[SNERF_ROWS][SNERF_COLS];
    snerf_inner one, two;
} snerf_outer;
int snerf_none(void);
const char* snerf_text(void);
size_t snerf_count(const snerf_outer* outer, long long n,
                   int k);
long long snerf_call(const snerf_outer* outer, const float* const* params, unsigned long long seed, unsigned int id, float x,
                     double y, const unsigned char* mask, void* scratch, int* out, snerf_inner* record, snerf_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_every_form_of_the_subset():
    h = _cdecl.Header(by_address=()).read(SYNTHETIC, 'synthetic.h')
    # defines; explicit and implicit enum values, implicit after explicit, a value given by a defined name; the anonymous enum
    assert h.constants == {'SNERF_ROWS': 3, 'SNERF_COLS': 4, 'SNERF_A': 2, 'SNERF_B': 3, 'SNERF_C': -7, 'SNERF_D': -6, 'SNERF_E': 3,
                           'SNERF_FIRST': 0, 'SNERF_SECOND': 1}
    inner, outer = h.structs['snerf_inner'], h.structs['snerf_outer']
    assert list(h.structs) == ['snerf_inner', 'snerf_outer']
    assert [(name, t) for name, t in inner._fields_] == [('offset', c_longlong), ('dims', c_int * 3)]
    assert ctypes.sizeof(inner) == 24
    names = [name for name, _ in outer._fields_]
    assert names == ['a', 'b', 'list', 'inner', 'flag', 'scale', 'per_row', 'grid', 'one', 'two']      # T *a, *b and T one, two
    types = dict(outer._fields_)
    assert types['a'] is c_void_p and types['b'] is c_void_p and types['list'] is POINTER(c_void_p)
    assert types['inner'] is POINTER(inner) and types['flag'] is c_ubyte and types['scale'] is c_double
    assert types['per_row'] is c_void_p * 3
    assert types['grid'] is (inner * 4) * 3 and types['one'] is inner          # [ROWS][COLS] by defined names: ROWS arrays of COLS
    assert (outer.flag.offset, outer.scale.offset, outer.per_row.offset, outer.grid.offset) == (32, 40, 48, 72)
    assert ctypes.sizeof(outer) == 72 + 12 * 24 + 2 * 24
    # prototypes: the ones inside comments are not there
    assert set(h.functions) == {'snerf_none', 'snerf_text', 'snerf_count', 'snerf_call'}
    assert h.functions['snerf_none'] == (c_int, [])
    assert h.functions['snerf_text'] == (c_char_p, [])
    assert h.functions['snerf_count'] == (c_size_t, [POINTER(outer), c_longlong, c_int])
    assert h.functions['snerf_call'] == (c_longlong, [POINTER(outer), POINTER(c_void_p), ctypes.c_ulonglong, ctypes.c_uint, c_float,
                                                      c_double, c_void_p, c_void_p, c_void_p, POINTER(inner), c_void_p])
    # a struct whose records the caller passes by address binds as void*
    h = _cdecl.Header(by_address=('snerf_inner',)).read(SYNTHETIC, 'synthetic.h')
    assert h.functions['snerf_call'][1][-2] is c_void_p and dict(h.structs['snerf_outer']._fields_)['inner'] is c_void_p


@pytest.mark.parametrize('text, line, words', [
    ('int snerf_a(int x);\nint snerf_b(uint32_t x);\n', 2, 'unknown type'),                    # an unknown type token
    ('typedef struct s {\n    int a;\n    wchar_t b;\n} snerf_s;\n', 3, 'unknown type'),
    ('int snerf_a(int x);\n\nint snerf_b(int (*callback)(int));\n', 3, 'cannot read'),         # a prototype it cannot read:
    ('int snerf_a(int x)\nint snerf_b(int y);\n', 1, 'cannot read'),                           # ... the counts would differ
    ('typedef struct s {\n    int a[SNERF_MISSING];\n} snerf_s;\n', 2, 'cannot resolve'),      # an undefined extent
    ('typedef struct s {\n    int a[2][SNERF_MISSING];\n} snerf_s;\n', 2, 'cannot resolve'),
    ('enum { SNERF_A = SNERF_MISSING };\n', 1, 'cannot resolve'),
    ('typedef struct s {\n    int a : 3;\n} snerf_s;\n', 2, 'cannot split'),                   # a declarator it cannot split
    ('typedef struct s {\n    int (*f)(int);\n} snerf_s;\n', 2, 'cannot split'),
    ('#define SNERF_N (2 + 1)\n', 1, 'cannot resolve'),
    ('\n#if SNERF_N > 1\nint snerf_a(void);\n#endif\n', 2, 'directive'),
    ('int snerf_global;\n', 1, 'cannot read'),
    ('void snerf_a(void x);\n', 1, 'void value'),
])
def test_refusals_name_the_header_line(text, line, words):
    with pytest.raises(RuntimeError, match=rf'^bad\.h:{line}: .*{words}'):
        _cdecl.Header().read(text, 'bad.h')


def test_the_prototypes_read_are_counted_against_the_names_in_the_text():
    """The prototypes a header adds are held to the distinct names its stripped text carries: here the second header declares
    again what the first one did, which would replace a signature in silence."""
    h = _cdecl.Header().read('int snerf_a(int x);\n', 'first.h')
    with pytest.raises(RuntimeError, match=r"^second\.h: read 1 prototypes, the text names 2: \['snerf_a'\]"):
        h.read('int snerf_a(long long x);\nint snerf_b(void);\n', 'second.h')


def test_the_real_headers():
    assert len(_lib.SIGNATURES) == 81 and len(_lib.STRUCTS) == 12
    assert ctypes.sizeof(_lib.STRUCTS['snerf_iteration']) == 64 == 8 * _lib.ITERATION_WORDS
    assert len(_lib.LEVEL_OUT_FIELDS) == _lib.C.SNERF_RENDER_FIELDS == 16
    assert _lib.LEVEL_OUT_FIELDS[_lib.C.SNERF_FIELD_SAVED_ACTS] == 'saved_acts' and _lib.LEVEL_OUT_FIELDS[-1] == 'view_dirs2'
    assert _lib.C.SNERF_E_RANGE == -4 and _lib.C.SNERF_OK == 0
    assert _lib.ABI_VERSION == _lib.C.SNERF_ABI_VERSION == 10
    assert (_lib.C.SNERF_PRECISION_F16S8, _lib.C.SNERF_PRECISION_BF16S8, _lib.C.SNERF_PRECISION_BF16) == (4, 5, 3)
    assert _lib.SIGNATURES['snerf_last_error'] == (c_char_p, [])
    assert _lib.SIGNATURES['snerf_mlp_packed_floats'] == (c_size_t, [POINTER(_lib.MlpDesc)])
    # records that live in device memory are passed by address
    assert _lib.SIGNATURES['snerf_iteration_advance'] == (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p])
    assert _lib.SIGNATURES['snerf_depth_error_sums'][1][2:4] == [c_double, c_double]
    assert _lib.RenderLayout.level.size == 6 * 16 * ctypes.sizeof(_lib.RenderSlot)
