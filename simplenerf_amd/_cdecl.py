"""Reader of the project's own C headers (include/simplenerf_hip.h, include/simplenerf_train.h) for the ctypes binding.

Not a C parser: it reads the subset those headers use -- comments, integer ``#define SNERF_*``, enum bodies, ``typedef struct
{...} name;`` with ``T *a, *b;`` declarators and ``[N]`` / ``[N][M]`` extents, scalar typedefs and prototypes -- and raises
RuntimeError naming the header line for anything else: a declaration skipped in silence is a function bound wrongly.

Types map as the binding passes them: scalars to their ctypes scalar, a pointer to a struct of the headers to POINTER(Class), a
pointer to a pointer to POINTER(c_void_p), a ``const char*`` return to c_char_p, every other pointer to c_void_p."""
from __future__ import annotations

import ctypes
import re

SCALARS = {'int': ctypes.c_int, 'unsigned int': ctypes.c_uint, 'long long': ctypes.c_longlong,
           'unsigned long long': ctypes.c_ulonglong, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
           'char': ctypes.c_char, 'unsigned char': ctypes.c_ubyte, 'void': None}
_TYPE_WORDS = {'const'} | {word for name in SCALARS for word in name.split()}
_SPACE = re.compile(r'\s*')
_FORMS = [(kind, re.compile(pattern)) for kind, pattern in (
    ('open', r'extern\s+"C"\s*\{'), ('close', r'\}'),
    ('enum', r'enum(?:\s+\w+)?\s*\{([^{}]*)\}\s*;'),
    ('struct', r'typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;'),
    ('alias', r'typedef\s+([^;{}()]+);'),
    ('prototype', r'([^;{}()]+?)\b(\w+)\s*\(([^;{}()]*)\)\s*;'))]


class Header:
    """What the headers read so far declare: ``constants`` (the ``#define SNERF_*`` and every enumerator), ``structs`` (typedef name
    -> ctypes.Structure class) and ``functions`` (name -> (restype, argtypes)).  ``by_address``: structs whose records the caller
    keeps in device or pinned memory and passes by address; a pointer to one binds as c_void_p."""

    def __init__(self, by_address=()):
        self.constants, self.structs, self.functions = {}, {}, {}
        self.aliases = {}                      # scalar typedefs: name -> (base type, pointer depth)
        self.by_address = frozenset(by_address)

    def read(self, text: str, name: str = '<header>') -> 'Header':
        text = re.sub(r'/\*.*?\*/|//[^\n]*', lambda m: re.sub(r'[^\n]', ' ', m.group()), text, flags=re.S)
        self._text, self._name = text, name
        for m in re.finditer(r'^[ \t]*#[^\n]*', text, flags=re.M):
            self._directive(m.group(), m.start())
        text = self._text = re.sub(r'^[ \t]*#[^\n]*', lambda m: ' ' * len(m.group()), text, flags=re.M)
        before, pos, depth = set(self.functions), 0, 0
        while True:
            pos = _SPACE.match(text, pos).end()
            if pos == len(text):
                break
            for kind, pattern in _FORMS:
                m = pattern.match(text, pos)
                if m:
                    break
            else:
                self._fail(pos, f'cannot read {" ".join(text[pos:pos + 80].split())!r}')
            if kind in ('open', 'close'):
                depth += 1 if kind == 'open' else -1
                if depth < 0:
                    self._fail(pos, 'unmatched }')
            elif kind == 'enum':
                self._enum(m.group(1), m.start(1))
            elif kind == 'struct':
                fields, at = [], m.start(1)
                for piece in m.group(1).split(';'):
                    base, declarators = self._declaration(piece, at) if piece.strip() else (None, [])
                    for stars, field, extents in declarators:
                        if field is None:
                            self._fail(at, f'a field without a name in {" ".join(piece.split())!r}')
                        fields.append((field, self._ctype(base, stars, extents, at)))
                    at += len(piece) + 1
                self.structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {'_fields_': fields, '__doc__': f'struct {m.group(2)}'})
            elif kind == 'alias':
                base, ((stars, alias, extents),) = self._declaration(m.group(1), m.start(1), single=True)
                if alias is None or extents or base in self.structs:
                    self._fail(pos, f'cannot read the typedef {m.group(1).strip()!r}')
                self.aliases[alias] = (base, stars)
            else:
                base, ((stars, _, _),) = self._declaration(m.group(1) + ' ', m.start(1), single=True)
                params = [] if m.group(3).strip() in ('', 'void') else m.group(3).split(',')
                args, at = [], m.start(3)
                for p in params:
                    p_base, ((p_stars, _, p_extents),) = self._declaration(p, at, single=True)
                    args.append(self._ctype(p_base, p_stars, p_extents, at))
                    at += len(p) + 1
                self.functions[m.group(2)] = (self._ctype(base, stars, [], pos, returns=True), args)
            pos = m.end()
        declared = set(re.findall(r'\b(snerf_[a-z_0-9]+)\s*\(', text))
        if declared != set(self.functions) - before:
            raise RuntimeError(f'{name}: read {len(set(self.functions) - before)} prototypes, the text names {len(declared)}: '
                               f'{sorted(declared ^ (set(self.functions) - before))}')
        return self

    # ---- pieces
    def _fail(self, pos: int, message: str):
        pos += len(self._text[pos:]) - len(self._text[pos:].lstrip())
        raise RuntimeError(f'{self._name}:{self._text.count(chr(10), 0, pos) + 1}: {message}')

    def _int(self, token: str, pos: int) -> int:
        token = token.strip()
        if re.fullmatch(r'[-+]?\s*(0[xX][0-9a-fA-F]+|\d+)', token):
            return int(token.replace(' ', ''), 0)
        if token not in self.constants:
            self._fail(pos, f'cannot resolve the value {token!r}')
        return self.constants[token]

    def _directive(self, line: str, pos: int) -> None:
        kind, rest = re.match(r'\s*#\s*(\w*)\s*(.*?)\s*$', line).groups()
        define = re.fullmatch(r'(\w+)(?:\s+(.+))?', rest)
        if kind == 'define' and define and define.group(1).startswith('SNERF_') and define.group(2):
            self.constants[define.group(1)] = self._int(define.group(2), pos)
        elif not (kind in ('include', 'ifndef', 'endif') or (kind == 'ifdef' and rest == '__cplusplus')
                  or (kind == 'define' and define and not define.group(2) and not define.group(1).startswith('SNERF_'))):
            self._fail(pos, f'cannot read the directive {line.strip()!r}')

    def _enum(self, body: str, pos: int) -> None:
        value = -1
        for piece in re.finditer(r'[^,]+', body):
            if not piece.group().strip():
                continue
            m = re.fullmatch(r'\s*(\w+)\s*(?:=([^=]+))?', piece.group())
            if not m:
                self._fail(pos + piece.start(), f'cannot read the enumerator {piece.group().strip()!r}')
            value = value + 1 if m.group(2) is None else self._int(m.group(2), pos + piece.start())
            self.constants[m.group(1)] = value

    def _declaration(self, text: str, pos: int, single: bool = False):
        """``const float *a, *b[N]`` -> ('float', [(1, 'a', []), (1, 'b', [N])]); a declarator may lack its name (a return type)."""
        tokens = re.findall(r'\w+|[^\w\s]', text)
        words = []
        while tokens and (tokens[0] in _TYPE_WORDS or (not words and (tokens[0] in self.structs or tokens[0] in self.aliases))):
            word = tokens.pop(0)
            if word != 'const':
                words.append(word)
            if word not in _TYPE_WORDS:
                break
        base = ' '.join(words)
        if base not in SCALARS and base not in self.structs and base not in self.aliases:
            self._fail(pos, f'unknown type {" ".join(words + tokens[:1])!r} in {" ".join(text.split())!r}')
        declarators, current = [], []
        for token in tokens + [',']:
            if token != ',':
                current.append(token)
                continue
            stars = 0
            while current and current[0] in ('*', 'const'):
                stars += current.pop(0) == '*'
            field = current.pop(0) if current and re.fullmatch(r'[A-Za-z_]\w*', current[0]) else None
            extents = []
            while len(current) >= 3 and current[0] == '[' and current[2] == ']':
                extents.append(self._int(current[1], pos))
                del current[:3]
            if current:
                self._fail(pos, f'cannot split the declarator in {" ".join(text.split())!r}')
            declarators.append((stars, field, extents))
            current = []
        if single and len(declarators) != 1:
            self._fail(pos, f'expected one declarator in {" ".join(text.split())!r}')
        return base, declarators

    def _ctype(self, base: str, stars: int, extents, pos: int, returns: bool = False):
        if base in self.aliases:
            base, stars = self.aliases[base][0], stars + self.aliases[base][1]
        if stars == 0:
            if base == 'void' and not returns:
                self._fail(pos, 'a void value')
            t = self.structs[base] if base in self.structs else SCALARS[base]
        elif stars >= 2:
            t = ctypes.POINTER(ctypes.c_void_p)
        elif base in self.structs and base not in self.by_address:
            t = ctypes.POINTER(self.structs[base])
        else:
            t = ctypes.c_char_p if returns and base == 'char' else ctypes.c_void_p
        for extent in reversed(extents):
            t = t * extent
        return t
