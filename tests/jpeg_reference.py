"""What the JPEG encoder's tests compare against, in numpy integers, written from the words of csrc/simplenerf_jpeg.h: the restated
encoder (``scan`` -> the entropy-coded segment, ``jfif`` -> the file around it), a baseline decoder of its own (``decode``: it reads
DQT, DHT, SOF0, DRI and SOS from the file, so it decodes other encoders' baseline files too), the bound formula and seeded fixtures."""
import struct

import numpy

BLOCK_BYTES = 208

# ITU-T T.81 Annex K.1 in zig-zag order, Annex K.3 as (codes per length 1..16, symbols in code order)
QUANT_BASE = (
    (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
     103, 99),
    (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66) + (99,) * 50)
_AC_LUMINANCE = bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748'
    '494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3'
    'c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
_AC_CHROMINANCE = bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748'
    '494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2'
    'c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')
# (table class << 4 | table id) -> (bits, values), in the order the DHT segments are written
HUFFMAN = {0x00: ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
           0x10: ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), _AC_LUMINANCE),
           0x01: ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
           0x11: ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), _AC_CHROMINANCE)}
ZIGZAG = numpy.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                      28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                      54, 47, 55, 62, 63])
COS = (4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0)          # round(4096 cos(k pi / 16)), k = 0..8


def dct_matrix():
    """D[u][x] of the header, from its seven constants: cos((2x+1) u pi/16) folded into the first quadrant, by integers alone."""
    d = numpy.zeros((8, 8), dtype=numpy.int64)
    for u in range(8):
        for x in range(8):
            k = (2 * x + 1) * u % 32
            k = 32 - k if k > 16 else k                      # cos is even about pi
            d[u, x] = 2896 if u == 0 else (COS[k] if k <= 8 else -COS[16 - k])
    return d


DCT = dct_matrix()


def quantisers(quality: int):
    """-> (2, 64) int64: the luminance and chrominance quantisers in zig-zag order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return numpy.clip((numpy.array(QUANT_BASE, dtype=numpy.int64) * scale + 50) // 100, 1, 255)


def huffman_codes(bits, values):
    """Annex C: symbol -> (code, length)."""
    codes, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[values[at]] = (code, length)
            code, at = code + 1, at + 1
        code <<= 1
    return codes


def geometry(h: int, w: int, channels: int):
    """-> (MCU size, MCUs per row, MCU rows, blocks per row)"""
    mcu = 16 if channels == 3 else 8
    per_row, rows = -(-w // mcu), -(-h // mcu)
    return mcu, per_row, rows, per_row * (6 if channels == 3 else 1)


def bound_bytes(h: int, w: int, channels: int) -> int:
    _, _, rows, blocks = geometry(h, w, channels)
    return rows * (2 * BLOCK_BYTES * blocks + 2)


def planes(image):
    """-> [sample planes padded to whole MCUs]: one for grey, Y and the subsampled Cb, Cr for colour (int64)."""
    h, w = image.shape[:2]
    channels = 3 if image.ndim == 3 else 1
    mcu, per_row, rows, _ = geometry(h, w, channels)
    ys, xs = numpy.minimum(numpy.arange(rows * mcu), h - 1), numpy.minimum(numpy.arange(per_row * mcu), w - 1)
    padded = image[ys][:, xs].astype(numpy.int64)
    if channels == 1:
        return [padded]
    r, g, b = padded[..., 0], padded[..., 1], padded[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    half = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    return [y, half(cb), half(cr)]


def plane_blocks(plane):
    """(H, W) -> (H/8, W/8, 8, 8)"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def forward(blocks, q):
    """Blocks (..., 8, 8) of samples, quantisers ``q`` (64,) in zig-zag order -> levels (..., 64) in zig-zag order."""
    s = blocks - 128
    t = (numpy.einsum('ux,...yx->...yu', DCT, s) + 1024) >> 11
    f8 = (numpy.einsum('vy,...yu->...vu', DCT, t) + 2048) >> 12
    f8 = f8.reshape(f8.shape[:-2] + (64,))[..., ZIGZAG]
    level = (numpy.abs(f8) + 4 * q) // (8 * q)
    limit = numpy.full(64, 1023)
    low = limit.copy()
    low[0] = 1024
    return numpy.where(f8 < 0, -numpy.minimum(level, low), numpy.minimum(level, limit))


def levels(image, quality: int):
    """-> (MCU rows, blocks per row, 64) int64: every block's levels in scan order (colour: Y00 Y01 Y10 Y11 Cb Cr per MCU)."""
    q = quantisers(quality)
    parts = planes(image)
    if len(parts) == 1:
        return forward(plane_blocks(parts[0]), q[0])
    y, cb, cr = forward(plane_blocks(parts[0]), q[0]), forward(plane_blocks(parts[1]), q[1]), forward(plane_blocks(parts[2]), q[1])
    rows, per_row = cb.shape[:2]
    out = numpy.empty((rows, per_row, 6, 64), dtype=numpy.int64)
    for i in range(4):
        out[:, :, i] = y[i >> 1::2, i & 1::2]
    out[:, :, 4], out[:, :, 5] = cb, cr
    return out.reshape(rows, per_row * 6, 64)


def size_of(v: int) -> int:
    return abs(v).bit_length()


def block_bits(level, predictor, dc, ac, symbols=None):
    """One block's bits as a '0'/'1' string (``symbols``: a list that receives ('dc', category) / ('ac', symbol))."""
    def piece(codes, symbol, value, size):
        code, length = codes[symbol]
        text = format(code, f'0{length}b')
        return text + (format((value if value >= 0 else value - 1) & ((1 << size) - 1), f'0{size}b') if size else '')
    diff = int(level[0]) - predictor
    out = [piece(dc, size_of(diff), diff, size_of(diff))]
    if symbols is not None:
        symbols.append(('dc', size_of(diff)))
    run = 0
    for k in range(1, 64):
        v = int(level[k])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            out.append(piece(ac, 0xF0, 0, 0))
            run -= 16
            if symbols is not None:
                symbols.append(('ac', 0xF0))
        out.append(piece(ac, run << 4 | size_of(v), v, size_of(v)))
        if symbols is not None:
            symbols.append(('ac', run << 4 | size_of(v)))
        run = 0
    if run:
        out.append(piece(ac, 0, 0, 0))
        if symbols is not None:
            symbols.append(('ac', 0))
    return ''.join(out)


def scan_of_levels(level, colour: bool, symbols=None) -> bytes:
    """(MCU rows, blocks per row, 64) levels -> the entropy-coded segment: one restart interval per MCU row."""
    tables = {key: huffman_codes(*HUFFMAN[key]) for key in HUFFMAN}
    out = bytearray()
    rows, blocks = level.shape[:2]
    for r in range(rows):
        predictors, text = [0, 0, 0], []
        for b in range(blocks):
            component = max(0, b % 6 - 3) if colour else 0
            chroma = 1 if component else 0
            text.append(block_bits(level[r, b], predictors[component], tables[chroma], tables[0x10 | chroma], symbols))
            predictors[component] = int(level[r, b, 0])
        text = ''.join(text)
        text += '1' * (-len(text) % 8)
        data = int(text, 2).to_bytes(len(text) // 8, 'big')
        out += data.replace(b'\xff', b'\xff\x00')
        if r != rows - 1:
            out += bytes([0xFF, 0xD0 + r % 8])
    return bytes(out)


def scan(image, quality: int) -> bytes:
    """The restated encoder: uint8 (h, w) or (h, w, 3) -> what snerf_jpeg_scan writes for it."""
    return scan_of_levels(levels(image, quality), image.ndim == 3)


def segment(marker: int, data: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack('>H', len(data) + 2) + data


def jfif(scan_bytes: bytes, h: int, w: int, channels: int, quality: int) -> bytes:
    """The file around an entropy-coded segment: SOI, APP0 (JFIF 1.01, no density), DQT, SOF0, DHT, DRI, SOS, the segment, EOI."""
    q = quantisers(quality)
    colour = channels == 3
    out = b'\xff\xd8' + segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for table in range(2 if colour else 1):
        out += segment(0xDB, bytes([table]) + bytes(int(v) for v in q[table]))
    components = [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] if colour else [(1, 0x11, 0)]
    out += segment(0xC0, struct.pack('>BHHB', 8, h, w, len(components)) + b''.join(bytes(c) for c in components))
    for key in (0x00, 0x10, 0x01, 0x11) if colour else (0x00, 0x10):
        out += segment(0xC4, bytes([key]) + bytes(HUFFMAN[key][0]) + bytes(HUFFMAN[key][1]))
    out += segment(0xDD, struct.pack('>H', geometry(h, w, channels)[1]))
    out += segment(0xDA, bytes([len(components)]) + b''.join(bytes([c[0], c[2] << 4 | c[2]]) for c in components) + bytes([0, 63, 0]))
    return out + scan_bytes + b'\xff\xd9'


def encode(image, quality: int) -> bytes:
    h, w = image.shape[:2]
    return jfif(scan(image, quality), h, w, 3 if image.ndim == 3 else 1, quality)


# ------------------------------------------------------------------------------------------------ the decoder
class Bits:
    def __init__(self, data: bytes):
        self.data, self.at, self.word, self.have = data, 0, 0, 0

    def take(self, n: int) -> int:
        while self.have < n:
            self.word = self.word << 8 | (self.data[self.at] if self.at < len(self.data) else 0xFF)
            self.at, self.have = self.at + 1, self.have + 8
        self.have -= n
        value = self.word >> self.have
        self.word &= (1 << self.have) - 1
        return value

    def symbol(self, lookup) -> int:
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.take(1)
            if (length, code) in lookup:
                return lookup[(length, code)]
        raise ValueError('no Huffman code matches')


def extend(value: int, size: int) -> int:
    return value if size == 0 or value >> (size - 1) else value - (1 << size) + 1


def parse(blob: bytes) -> dict:
    """A baseline file's tables, frame header and entropy-coded intervals (split at the RSTn markers, un-stuffed); the quantised
    levels of every block: {'levels': per component (block rows, block columns, 64) in zig-zag order, 'quant': (64,) per component,
    'size', 'sampling', 'restart_interval', 'restart_markers'}."""
    if blob[:2] != b'\xff\xd8' or blob[-2:] != b'\xff\xd9':
        raise ValueError('not a JPEG file: SOI or EOI missing')
    at, quant, huffman, frame, interval, scan_components = 2, {}, {}, None, 0, None
    while True:
        if blob[at] != 0xFF:
            raise ValueError(f'marker expected at {at}')
        marker, (length,) = blob[at + 1], struct.unpack('>H', blob[at + 2:at + 4])
        data = blob[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            while data:
                if data[0] >> 4:
                    raise ValueError('16-bit quantisation table')
                quant[data[0] & 15] = numpy.array(list(data[1:65]), dtype=numpy.int64)
                data = data[65:]
        elif marker == 0xC4:
            while data:
                bits = list(data[1:17])
                count = sum(bits)
                codes = huffman_codes(bits, data[17:17 + count])
                huffman[data[0]] = {(length_, code): symbol for symbol, (code, length_) in codes.items()}
                data = data[17 + count:]
        elif marker == 0xC0:
            precision, h, w, count = struct.unpack('>BHHB', data[:6])
            frame = {'size': (h, w), 'components': [(data[6 + 3 * i], data[7 + 3 * i] >> 4, data[7 + 3 * i] & 15, data[8 + 3 * i]) for i in range(count)]}
            if precision != 8:
                raise ValueError('not 8-bit')
        elif marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise ValueError(f'not a baseline file: SOF marker {marker:02X}')
        elif marker == 0xDD:
            interval, = struct.unpack('>H', data)
        elif marker == 0xDA:
            count = data[0]
            scan_components = [(data[1 + 2 * i], data[2 + 2 * i] >> 4, data[2 + 2 * i] & 15) for i in range(count)]
            if tuple(data[1 + 2 * count:]) != (0, 63, 0):
                raise ValueError('not a sequential scan')
            break
    if frame is None or [c[0] for c in scan_components] != [c[0] for c in frame['components']]:
        raise ValueError('the scan does not carry every component of the frame')
    # the entropy-coded data: intervals between RSTn markers, FF 00 -> FF
    body, intervals, markers, start, i = blob[at:-2], [], [], 0, 0
    while i < len(body) - 1:
        if body[i] == 0xFF and body[i + 1] != 0:
            if not 0xD0 <= body[i + 1] <= 0xD7:
                raise ValueError(f'marker FF {body[i + 1]:02X} inside the scan')
            intervals.append(body[start:i])
            markers.append(body[i + 1] - 0xD0)
            start, i = i + 2, i + 2
        else:
            i += 2 if body[i] == 0xFF else 1
    intervals.append(body[start:])
    intervals = [piece.replace(b'\xff\x00', b'\xff') for piece in intervals]
    if len(frame['components']) == 1:          # a scan of one component is not interleaved: its MCU is one block whatever its factors
        frame['components'] = [(frame['components'][0][0], 1, 1, frame['components'][0][3])]
    h, w = frame['size']
    hmax, vmax = max(c[1] for c in frame['components']), max(c[2] for c in frame['components'])
    per_row, rows = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    if interval and len(intervals) != -(-(per_row * rows) // interval):
        raise ValueError(f'{len(intervals)} intervals for {per_row * rows} MCUs of restart interval {interval}')
    if not interval and len(intervals) != 1:
        raise ValueError('RSTn markers without a DRI segment')
    out = [numpy.zeros((rows * c[2], per_row * c[1], 64), dtype=numpy.int64) for c in frame['components']]
    mcu = 0
    for piece in intervals:
        reader, predictors = Bits(piece), [0] * len(out)
        for _ in range(interval or per_row * rows):
            if mcu == per_row * rows:
                break
            my, mx = divmod(mcu, per_row)
            for ci, (_, ch, cv, _) in enumerate(frame['components']):
                dc, ac = huffman[scan_components[ci][1]], huffman[0x10 | scan_components[ci][2]]
                for by in range(cv):
                    for bx in range(ch):
                        block = out[ci][my * cv + by, mx * ch + bx]
                        size = reader.symbol(dc)
                        predictors[ci] += extend(reader.take(size), size) if size else 0
                        block[0] = predictors[ci]
                        k = 1
                        while k < 64:
                            symbol = reader.symbol(ac)
                            run, size = symbol >> 4, symbol & 15
                            if size == 0:
                                if run != 15:
                                    break          # EOB
                                k += 16
                                continue
                            k += run
                            if k > 63:
                                raise ValueError('a run past the 63rd coefficient')
                            block[k] = extend(reader.take(size), size)
                            k += 1
            mcu += 1
        if reader.at > len(piece) + 1:
            raise ValueError('an interval ends inside a symbol')
    return {'levels': out, 'quant': [quant[c[3]] for c in frame['components']], 'size': (h, w),
            'sampling': [(c[1], c[2]) for c in frame['components']], 'restart_interval': interval, 'restart_markers': markers}


def idct_matrix():
    u, x = numpy.meshgrid(numpy.arange(8), numpy.arange(8), indexing='ij')
    return numpy.where(u == 0, numpy.sqrt(1 / 8), 0.5) * numpy.cos((2 * x + 1) * u * numpy.pi / 16)          # [u][x], orthonormal


def decode(blob: bytes):
    """-> uint8 (h, w) or (h, w, 3): dequantise, float64 IDCT, + 128, replicate the chroma samples, JFIF YCbCr -> RGB, round, clip."""
    parsed = parse(blob)
    h, w = parsed['size']
    c = idct_matrix()
    hmax, vmax = max(s[0] for s in parsed['sampling']), max(s[1] for s in parsed['sampling'])
    full = []
    for level, q, (ch, cv) in zip(parsed['levels'], parsed['quant'], parsed['sampling']):
        natural = numpy.zeros(level.shape, dtype=numpy.float64)
        natural[..., ZIGZAG] = level * q
        natural = natural.reshape(level.shape[:2] + (8, 8))
        samples = numpy.einsum('vy,...vu,ux->...yx', c, natural, c) + 128
        plane = samples.transpose(0, 2, 1, 3).reshape(level.shape[0] * 8, level.shape[1] * 8)
        full.append(numpy.repeat(numpy.repeat(plane, vmax // cv, axis=0), hmax // ch, axis=1)[:h, :w])
    if len(full) == 1:
        return numpy.clip(numpy.rint(full[0]), 0, 255).astype(numpy.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128
    rgb = numpy.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return numpy.clip(numpy.rint(rgb), 0, 255).astype(numpy.uint8)


def exact_levels(plane, q):
    """round(float64 DCT / q) of a padded sample plane -> (block rows, block columns, 64) in zig-zag order (half away from zero)."""
    c = idct_matrix()
    f = numpy.einsum('vy,...yx,ux->...vu', c, plane_blocks(plane).astype(numpy.float64) - 128, c)
    f = f.reshape(f.shape[:2] + (64,))[..., ZIGZAG] / q
    return (numpy.sign(f) * numpy.floor(numpy.abs(f) + 0.5)).astype(numpy.int64)


def psnr(a, b) -> float:
    error = numpy.mean((a.astype(numpy.float64) - b.astype(numpy.float64)) ** 2)
    return float('inf') if error == 0 else float(10 * numpy.log10(255 ** 2 / error))


# ------------------------------------------------------------------------------------------------ fixtures
def noise(h: int, w: int, channels: int = 3, seed: int = 0):
    shape = (h, w, 3) if channels == 3 else (h, w)
    return numpy.random.default_rng(seed).integers(0, 256, size=shape, dtype=numpy.uint8)


def textured(h: int, w: int, channels: int = 3, seed: int = 2):
    """Ramps, stripes of three periods and a little seeded noise: edges and texture at every frequency of a block."""
    y, x = numpy.mgrid[0:h, 0:w]
    rng = numpy.random.default_rng(seed)
    out = []
    for c in range(3):
        plane = 128 + 60 * numpy.sign(numpy.sin(2 * numpy.pi * (x + 2 * c) / (3 + 2 * c))) * (y % 32 < 16) \
            + 50 * numpy.sin(2 * numpy.pi * (x + y * (c + 1)) / 23.0) + (x * 40 // max(w, 1)) - 20 + rng.integers(-6, 7, size=(h, w))
        out.append(numpy.clip(numpy.rint(plane), 0, 255).astype(numpy.uint8))
    out = numpy.stack(out, axis=-1)
    return out if channels == 3 else out[:, :, 0]


def checkerboard(h: int, w: int, channels: int = 1):
    """0 / 255 alternating per pixel: at quality 100 the largest AC level there is; beside a flat block, the largest DC steps."""
    y, x = numpy.mgrid[0:h, 0:w]
    plane = (((y + x) & 1) * 255).astype(numpy.uint8)
    plane[:, :8] = 0                       # a black block, then a white one: DC differences of category 11 at quality 100
    plane[:, 8:16] = 255
    return numpy.stack([plane] * 3, axis=-1) if channels == 3 else plane


def basis_block(v: int, u: int, coefficient: float = 400.0):
    """An 8 x 8 grey block that is 128 + coefficient x the orthonormal (v, u) DCT basis pattern (vertical, horizontal frequency)."""
    c = idct_matrix()
    return numpy.clip(numpy.rint(128 + coefficient * numpy.outer(c[v], c[u])), 0, 255).astype(numpy.uint8)


def basis_row():
    """8 x 32 grey: the basis patterns (7,7) -- the 63rd zig-zag coefficient alone --, (0,1), (1,0) and (3,4) side by side."""
    return numpy.concatenate([basis_block(7, 7), basis_block(0, 1), basis_block(1, 0), basis_block(3, 4)], axis=1)


# name -> (frame, quality): the smallest inputs at which each step of the encoder can go wrong (tests/test_gpu_jpeg.py says why)
CASES = {
    '1x1 grey': (lambda: noise(1, 1, 1, seed=3), 90),
    '1x1 colour': (lambda: noise(1, 1, 3, seed=3), 90),
    '8x8 grey': (lambda: textured(8, 8, 1), 50),
    '9x7 grey': (lambda: textured(9, 7, 1), 90),
    '16x16 colour': (lambda: textured(16, 16), 50),
    '17x33 colour': (lambda: textured(17, 33), 90),
    '147x40 colour': (lambda: textured(147, 40), 90),
    '16x1008 colour noise': (lambda: noise(16, 1008), 100),
    'checkerboard grey': (lambda: checkerboard(16, 32, 1), 100),
    'checkerboard colour': (lambda: checkerboard(16, 32, 3), 100),
    'basis patterns': (basis_row, 50),
    '17x33 colour, quality 1': (lambda: textured(17, 33), 1),
    '17x33 colour, quality 50': (lambda: textured(17, 33), 50),
    '17x33 colour, quality 100': (lambda: textured(17, 33), 100),
    '23x300 grey, two chunks': (lambda: textured(23, 300, 1), 90),          # transform: 38 MCUs are a chunk of 32 and one of 6
    '8x2048 grey, a full pass': (lambda: noise(8, 2048, 1, seed=4), 50),      # emit: exactly 256 blocks
    '9x2060 grey, two passes': (lambda: textured(9, 2060, 1), 90),           # emit: 258 blocks, bits carried between passes
    '40x700 colour, two passes': (lambda: textured(40, 700), 50),            # 44 MCUs: six chunks, 264 blocks
}
_expected = {}


def expected(name: str):
    """-> (frame, quality, the restated encoder's scan, its symbols), computed once per process."""
    if name not in _expected:
        make, quality = CASES[name]
        image = make()
        symbols = []
        _expected[name] = (image, quality, scan_of_levels(levels(image, quality), image.ndim == 3, symbols), symbols)
    return _expected[name]


# ------------------------------------------------------------------------------------------------ the AVI container
def walk_avi(blob: bytes) -> dict:
    """Walk a RIFF AVI and check what a reader relies on: every size, the even padding, 'MJPG' in ``strh`` and ``strf``, every
    ``idx1`` entry against its chunk.  -> {'avih': its 14 dwords, 'strh', 'strf': the unpacked headers, 'frames': [bytes]}"""
    def chunks(data, at, end):
        out = []
        while at < end:
            tag, (size,) = data[at:at + 4], struct.unpack('<I', data[at + 4:at + 8])
            assert at + 8 + size <= end, (tag, at, size, end)
            out.append((tag, at, data[at + 8:at + 8 + size]))
            at += 8 + size + (size & 1)
        assert at == end or at == end + 1, (at, end)
        return out
    assert blob[:4] == b'RIFF' and blob[8:12] == b'AVI ' and struct.unpack('<I', blob[4:8])[0] == len(blob) - 8
    top = chunks(blob, 12, len(blob))
    assert [tag for tag, _, _ in top] == [b'LIST', b'LIST', b'idx1']
    (_, _, hdrl), (_, movi_at, movi), (_, _, idx1) = top
    assert hdrl[:4] == b'hdrl' and movi[:4] == b'movi'
    (tag_a, _, avih), (tag_l, _, strl) = chunks(hdrl, 4, len(hdrl))
    assert tag_a == b'avih' and len(avih) == 56 and tag_l == b'LIST' and strl[:4] == b'strl'
    (tag_h, _, strh), (tag_f, _, strf) = chunks(strl, 4, len(strl))
    assert tag_h == b'strh' and len(strh) == 56 and tag_f == b'strf' and len(strf) == 40
    assert strh[:4] == b'vids' and strh[4:8] == b'MJPG' and strf[16:20] == b'MJPG'
    frames = chunks(movi, 4, len(movi))
    assert all(tag == b'00dc' for tag, _, _ in frames)
    assert all((8 + len(data)) % 2 == 0 or movi[at + 8 + len(data)] == 0 for _, at, data in frames)
    assert len(idx1) == 16 * len(frames)
    for i, (tag, at, data) in enumerate(frames):
        entry_tag, flags, offset, size = struct.unpack('<4sIII', idx1[16 * i:16 * i + 16])
        assert entry_tag == b'00dc' and flags == 0x10 and size == len(data), i
        assert offset == at and movi[offset:offset + 4] == b'00dc' and struct.unpack('<I', movi[offset + 4:offset + 8])[0] == size, i
        # (counted from the 'movi' tag, which is 8 bytes into its LIST chunk)
        assert blob[movi_at + 8 + offset:movi_at + 8 + offset + 4] == b'00dc', i
    return {'avih': struct.unpack('<14I', avih), 'strh': struct.unpack('<4s4sIHHIIIIIIIi4H', strh),
            'strf': struct.unpack('<IiiHH4sIiiII', strf), 'frames': [data for _, _, data in frames]}
