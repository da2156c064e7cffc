"""What the PNG encoder's tests compare against, in numpy: a PNG decoder for the five filter types (it returns the filter byte of
every row), the restated adaptive filter rule of csrc/simplenerf_png.h, the bound formula and seeded fixtures."""
import struct
import zlib

import numpy

SIGNATURE = b'\x89PNG\r\n\x1a\n'
STRIP_BYTES = 32768


def paeth(a, b, c):
    """The Paeth predictor on int arrays (or ints): the neighbour closest to a + b - c, ties in the order a, b, c."""
    p = a + b - c
    pa, pb, pc = numpy.abs(p - a), numpy.abs(p - b), numpy.abs(p - c)
    return numpy.where((pa <= pb) & (pa <= pc), a, numpy.where(pb <= pc, b, c))


def filter_row(kind: int, row, above, bpp: int):
    """One raw row (uint8, w * bpp) filtered with type ``kind``; ``above`` the RAW row above (zeros for the first row)."""
    row, above = row.astype(numpy.int64), above.astype(numpy.int64)
    left = numpy.concatenate([numpy.zeros(bpp, dtype=numpy.int64), row[:-bpp]])
    above_left = numpy.concatenate([numpy.zeros(bpp, dtype=numpy.int64), above[:-bpp]])
    predicted = (numpy.zeros_like(row), left, above, (left + above) >> 1, paeth(left, above, above_left))[kind]
    return ((row - predicted) & 255).astype(numpy.uint8)


def filter_image(pixels, kinds):
    """-> the bytes a PNG's IDAT inflates to, for uint8 ``pixels`` (h, w) or (h, w, 3) and one filter type per row."""
    h = pixels.shape[0]
    rows = pixels.reshape(h, -1)
    bpp = 1 if pixels.ndim == 2 else pixels.shape[2]
    out = numpy.empty((h, 1 + rows.shape[1]), dtype=numpy.uint8)
    for y in range(h):
        above = rows[y - 1] if y else numpy.zeros_like(rows[0])
        out[y, 0] = kinds[y]
        out[y, 1:] = filter_row(int(kinds[y]), rows[y], above, bpp)
    return out.tobytes()


def adaptive_kinds(pixels):
    """The rule of simplenerf_png.h: per row the type in 0..4 that minimises sum(min(v, 256 - v)) over the row's filtered bytes,
    the lowest type on a tie; the first row's row above is zeros."""
    h = pixels.shape[0]
    rows = pixels.reshape(h, -1)
    bpp = 1 if pixels.ndim == 2 else pixels.shape[2]
    kinds = []
    for y in range(h):
        above = rows[y - 1] if y else numpy.zeros_like(rows[0])
        costs = []
        for kind in range(5):
            v = filter_row(kind, rows[y], above, bpp).astype(numpy.int64)
            costs.append(int(numpy.minimum(v, 256 - v).sum()))
        kinds.append(int(numpy.argmin(costs)))          # (argmin returns the first minimum)
    return kinds


def unfilter(data: bytes, h: int, w: int, bpp: int):
    """-> (pixels (h, w * bpp) uint8, [filter byte of each row]) from the inflated IDAT bytes."""
    stride = 1 + w * bpp
    if len(data) != h * stride:
        raise ValueError(f'{len(data)} filtered bytes, expected {h * stride}')
    out = numpy.zeros((h, w * bpp), dtype=numpy.int64)
    kinds = []
    for y in range(h):
        kind = data[y * stride]
        line = numpy.frombuffer(data, dtype=numpy.uint8, count=w * bpp, offset=y * stride + 1).astype(numpy.int64)
        above = out[y - 1] if y else numpy.zeros(w * bpp, dtype=numpy.int64)
        kinds.append(kind)
        if kind == 0:
            out[y] = line
        elif kind == 2:
            out[y] = (line + above) & 255
        elif kind in (1, 3, 4):
            row = out[y]
            for x in range(w * bpp):
                a = row[x - bpp] if x >= bpp else 0
                c = above[x - bpp] if x >= bpp else 0
                predicted = a if kind == 1 else ((a + above[x]) >> 1) if kind == 3 else int(paeth(a, above[x], c))
                row[x] = (line[x] + predicted) & 255
        else:
            raise ValueError(f'row {y}: filter type {kind}')
    return out.astype(numpy.uint8), kinds


def inflate(blob: bytes):
    """-> (filtered bytes, h, w, bytes per pixel) of an 8-bit grey or RGB PNG with ONE IDAT chunk; checks the signature, every
    chunk's CRC, the chunk order and that the IDAT payload is one complete zlib stream of h * (1 + w * bpp) bytes."""
    if blob[:8] != SIGNATURE:
        raise ValueError('not a PNG signature')
    pos, chunks = 8, []
    while pos < len(blob):
        size, tag = struct.unpack('>I4s', blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + size]
        crc, = struct.unpack('>I', blob[pos + 8 + size:pos + 12 + size])
        if len(data) != size or crc != (zlib.crc32(tag + data) & 0xFFFFFFFF):
            raise ValueError(f'chunk {tag!r}: bad length or CRC')
        chunks.append((tag, data))
        pos += 12 + size
    if [tag for tag, _ in chunks] != [b'IHDR', b'IDAT', b'IEND'] or chunks[2][1]:
        raise ValueError(f'chunks {[tag for tag, _ in chunks]}: expected IHDR, one IDAT, IEND')
    w, h, depth, colour, compression, filtering, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    if (depth, compression, filtering, interlace) != (8, 0, 0, 0) or colour not in (0, 2):
        raise ValueError('not an 8-bit grey or RGB, non-interlaced PNG')
    inflater = zlib.decompressobj()
    data = inflater.decompress(chunks[1][1]) + inflater.flush()
    if not inflater.eof or inflater.unused_data:
        raise ValueError('the IDAT payload is not exactly one zlib stream')
    bpp = 3 if colour == 2 else 1
    if len(data) != h * (1 + w * bpp):
        raise ValueError(f'{len(data)} filtered bytes, expected {h * (1 + w * bpp)}')
    return data, h, w, bpp


def decode(blob: bytes):
    """-> (pixels (h, w) or (h, w, 3) uint8, [filter byte of each row]) of such a PNG."""
    data, h, w, bpp = inflate(blob)
    pixels, kinds = unfilter(data, h, w, bpp)
    return (pixels.reshape(h, w, 3) if bpp == 3 else pixels), kinds


def holds(blob: bytes, pixels) -> bool:
    """Whether such a PNG holds exactly ``pixels``, without un-filtering (for large frames: filtering is one numpy expression per
    row and invertible): its filtered bytes are ``pixels`` filtered with the file's own row types."""
    data, h, w, bpp = inflate(blob)
    if pixels.shape != ((h, w, 3) if bpp == 3 else (h, w)):
        return False
    kinds = [data[y * (1 + w * bpp)] for y in range(h)]
    return max(kinds) <= 4 and filter_image(pixels, kinds) == data


def container(stream: bytes, h: int, w: int, channels: int) -> bytes:
    """A PNG around a zlib stream, built as harness._png_bytes builds it."""
    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)
    header = struct.pack('>IIBBBBB', w, h, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b'IHDR', header) + chunk(b'IDAT', stream) + chunk(b'IEND', b'')


def raw_bytes(h: int, w: int, channels: int) -> int:
    return h * (1 + w * channels)


def bound_bytes(h: int, w: int, channels: int) -> int:
    """The contract's bound on a stream: raw + 10 bytes per started strip + 6."""
    raw = raw_bytes(h, w, channels)
    return raw + 10 * ((raw + STRIP_BYTES - 1) // STRIP_BYTES) + 6


# ---- the structure of a stream: an inflater that reports what it reads
_LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_CODE_LENGTH_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _canonical(lengths):
    """{(length, code): symbol} of the canonical Huffman code (RFC 1951 3.2.2) and its Kraft sum in units of 2^-15."""
    table, code, kraft = {}, 0, 0
    for bits in range(1, 16):
        for symbol, n in enumerate(lengths):
            if n == bits:
                table[(bits, code)] = symbol
                code += 1
                kraft += 1 << (15 - bits)
        code <<= 1
    return table, kraft


def deflate_blocks(stream: bytes):
    """The blocks of a zlib stream, in order: dicts with 'type' (0 stored, 2 dynamic), 'final', 'start' / 'end' (offsets of its output
    in the inflated data), 'ends_on_byte' (the block's last bit is the last bit of a byte), 'matches' [(output offset, length,
    distance)], 'lengths' (the literal/length code lengths), 'distance_lengths', 'code_length_lengths' and the Kraft sums of the
    block's codes ('kraft', 'code_length_kraft'; 32768 = complete).  Fixed-Huffman blocks are not read (the encoder writes none)."""
    data = stream[2:-4]
    pos = 0          # in bits

    def take(n):
        nonlocal pos
        value = 0
        for k in range(n):
            value |= ((data[(pos + k) >> 3] >> ((pos + k) & 7)) & 1) << k
        pos += n
        return value

    def symbol(table):
        code = 0
        for bits in range(1, 16):
            code = (code << 1) | take(1)
            if (bits, code) in table:
                return table[(bits, code)]
        raise ValueError('no such code')

    blocks, out = [], 0
    while True:
        block = {'final': take(1), 'type': take(2), 'start': out, 'matches': []}
        if block['type'] == 0:
            pos = (pos + 7) & ~7
            size, inverse = take(16), take(16)
            if size ^ inverse != 0xFFFF:
                raise ValueError('stored block: LEN / NLEN')
            pos += 8 * size
            out += size
        elif block['type'] == 2:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            code_lengths = [0] * 19
            for k in range(hclen):
                code_lengths[_CODE_LENGTH_ORDER[k]] = take(3)
            cl_table, block['code_length_kraft'] = _canonical(code_lengths)
            lengths = []
            while len(lengths) < hlit + hdist:
                s = symbol(cl_table)
                if s < 16:
                    lengths.append(s)
                elif s == 16:
                    lengths += [lengths[-1]] * (3 + take(2))
                else:
                    lengths += [0] * ((3 + take(3)) if s == 17 else (11 + take(7)))
            if len(lengths) != hlit + hdist:
                raise ValueError('code lengths overrun')
            block['lengths'], block['distance_lengths'], block['code_length_lengths'] = lengths[:hlit], lengths[hlit:], code_lengths
            table, block['kraft'] = _canonical(lengths[:hlit])
            distance_table, _ = _canonical(lengths[hlit:])
            while True:
                s = symbol(table)
                if s < 256:
                    out += 1
                elif s == 256:
                    break
                else:
                    length = _LENGTH_BASE[s - 257] + take(_LENGTH_EXTRA[s - 257])
                    d = symbol(distance_table)
                    if d >= 4:
                        raise ValueError('a distance code this encoder never writes')
                    block['matches'].append((out, length, d + 1))
                    out += length
        else:
            raise ValueError(f'block type {block["type"]}')
        block['end'], block['ends_on_byte'] = out, pos % 8 == 0
        blocks.append(block)
        if block['final']:
            break
    if (pos + 7) // 8 != len(data):
        raise ValueError('bytes after the final block')
    return blocks


def check_contract(stream: bytes, raw: int):
    """Asserts the block structure simplenerf_png.h promises for a stream of ``raw`` filtered bytes; returns the strips' blocks."""
    blocks = deflate_blocks(stream)
    strips = [b for b in blocks if b['end'] > b['start']]
    assert [(b['start'], b['end']) for b in strips] == [(s, min(s + STRIP_BYTES, raw)) for s in range(0, raw, STRIP_BYTES)]
    assert [b['final'] for b in blocks] == [0] * (len(blocks) - 1) + [1] and blocks[-1] is strips[-1]
    for before, block in zip([None] + blocks[:-1], blocks):
        if block['end'] == block['start']:          # the pigz marker: only where a coded strip did not end on a byte boundary
            assert block['type'] == 0 and before is not None and before['type'] == 2 and not before['ends_on_byte']
        elif before is not None:
            assert before['ends_on_byte'] or before['type'] == 0, 'a strip starts inside a byte'
        if block['type'] == 2:
            assert block['kraft'] == 32768 and block['code_length_kraft'] == 32768, 'a code that is not complete'
            assert block['distance_lengths'] == ([1] if block['matches'] else [0])
            for at, length, distance in block['matches']:
                assert distance == 1 and 3 <= length <= 258 and at - 1 >= block['start'], (at, length, distance)
    return strips


def huffman_depth(counts) -> int:
    """The longest code of an unconstrained Huffman code of the non-zero ``counts``."""
    import heapq
    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


# ---- fixtures (numpy only, seeded)
def noise(h: int, w: int, channels: int = 3, seed: int = 0):
    shape = (h, w, 3) if channels == 3 else (h, w)
    return numpy.random.default_rng(seed).integers(0, 256, size=shape, dtype=numpy.uint8)


def smooth(h: int, w: int, channels: int = 3, seed: int = 1, box: int = 9):
    """Box-blurred seeded noise stretched to 0..255: neighbouring pixels differ by a few levels, as in a rendered frame."""
    rng = numpy.random.default_rng(seed)
    field = rng.random((h + box - 1, w + box - 1, channels))
    sums = numpy.cumsum(numpy.cumsum(numpy.pad(field, ((1, 0), (1, 0), (0, 0))), axis=0), axis=1)
    blurred = sums[box:, box:] - sums[:-box, box:] - sums[box:, :-box] + sums[:-box, :-box]
    blurred = (blurred - blurred.min()) / (blurred.max() - blurred.min())
    out = numpy.rint(blurred * 255).astype(numpy.uint8)
    return out if channels == 3 else out[:, :, 0]


RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517)
# a run of r: one literal, then r - 1 bytes as matches of 258 while more than 258 are left, then one match, or 1-2 literals
RUN_MATCHES = (3, 256, 257, 258, 258, 258, 258, 257, 258, 258)


def runs_row():
    """One grey row of runs of the lengths above; neighbouring runs differ in value."""
    row = numpy.concatenate([numpy.full(n, 10 + 7 * k, dtype=numpy.uint8) for k, n in enumerate(RUN_LENGTHS)])
    return row.reshape(1, -1)


def fibonacci_row(chain: bool = False):
    """1 x 28 656 grey: byte value k occurs Fib(k + 1) times for k = 0..20 (1, 1, 2, 3, ... 10946), no two neighbours equal.  With
    filter type 0 the strip's symbol counts are these plus one more 0 (the filter byte) and one end-of-block, and those two spoil
    the Fibonacci chain: an unconstrained Huffman code of them is 11 deep, not 20.

    ``chain``: 1 x 28 654, byte value k occurs Fib(k + 2) times for k = 1..19 (2, 3, 5, ... 10946) and 0 does not occur -- with the
    filter byte (one 0) and the end-of-block the symbol counts are 1, 1, 2, 3, ... 10946 exactly, whose Huffman code is a chain 20
    deep, so this one does need the 15-bit limit."""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    counts = [0] + fib[2:] if chain else list(fib)
    assert sum(counts) == (28654 if chain else 28656)
    # the most frequent value (10946 < half the row) can always be placed: lay the values out by decreasing count into the
    # even positions, then the odd ones -- equal values end up at least two apart
    order = numpy.argsort(-numpy.array(counts), kind='stable')
    values = numpy.concatenate([numpy.full(counts[k], k, dtype=numpy.uint8) for k in order])
    n = len(values)
    row = numpy.empty(n, dtype=numpy.uint8)
    row[0::2] = values[:(n + 1) // 2]
    row[1::2] = values[(n + 1) // 2:]
    assert not (row[1:] == row[:-1]).any()
    return row.reshape(1, -1)
