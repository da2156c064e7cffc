"""The library's stable radix sort and mask compaction on the device (csrc/sort.hip -> ops.sort_values / sort_keys_with_order /
compact_pair) against numpy: the order of the stable sort is unique, so every comparison is exact.

Counts: around a wave (63, 64, 65), around a tile of 2048 keys, several tiles with a ragged tail, 16 384 | 16 385 (the last count
whose 256 x tiles digit counters are scanned in one step | the first that needs a second level), 70 001 and 1 200 003 (two levels,
a few and many chunks)."""
import numpy
import pytest
import torch

from simplenerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE = 2048
COUNTS = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 16384, 16385, 70001, 1200003)
KEY_BITS = (1, 8, 9, 22, 32)
PATTERNS = ('random', 'low3', 'equal', 'ascending', 'descending', 'absent')


def make_keys(pattern: str, count: int, key_bits: int, rng) -> numpy.ndarray:
    """Non-negative int32 keys below 2 ** key_bits."""
    top = 2 ** min(key_bits, 31)
    if pattern == 'random':                 # over the full key_bits
        keys = rng.integers(0, top, count)
    elif pattern == 'low3':                 # long runs of ties
        keys = rng.integers(0, min(top, 8), count)
    elif pattern == 'equal':
        keys = numpy.full(count, top - 1)
    elif pattern == 'ascending':            # (with ties where count exceeds the key range)
        keys = numpy.arange(count) * top // count
    elif pattern == 'descending':
        keys = (numpy.arange(count)[::-1] * top // count)
    else:                                   # one value of the lowest digit never occurs
        keys = rng.integers(0, top, count)
        absent = min(5, top - 1)
        keys = numpy.where((keys & 255) == absent, keys ^ 1, keys)
        assert not ((keys & 255) == absent).any()
    keys = numpy.ascontiguousarray(keys, dtype=numpy.int32)
    assert keys.min() >= 0 and int(keys.max()) < 2 ** key_bits
    return keys


@pytest.mark.parametrize('key_bits', KEY_BITS)
@pytest.mark.parametrize('count', COUNTS)
def test_sort_keys_with_order_is_the_stable_argsort(count, key_bits):
    rng = numpy.random.default_rng(count * 100 + key_bits)
    for pattern in PATTERNS:
        keys = make_keys(pattern, count, key_bits, rng)
        on_device = torch.from_numpy(keys).to(DEV)
        sorted_keys, order = ops.sort_keys_with_order(on_device, key_bits)
        assert sorted_keys.dtype == torch.int32 and order.dtype == torch.int64 and sorted_keys.shape == order.shape == (count,)
        want = numpy.argsort(keys, kind='stable')
        got = order.cpu().numpy()
        assert numpy.array_equal(got, want), (pattern, int((got != want).sum()))
        assert numpy.array_equal(sorted_keys.cpu().numpy(), keys[want]), pattern
        assert numpy.array_equal(on_device.cpu().numpy(), keys), pattern        # the input is not written


def test_key_bits_defaults_to_all_bits():
    keys = numpy.random.default_rng(5).integers(0, 2 ** 31, 5000).astype(numpy.int32)
    sorted_keys, order = ops.sort_keys_with_order(torch.from_numpy(keys).to(DEV))
    assert numpy.array_equal(order.cpu().numpy(), numpy.argsort(keys, kind='stable'))
    empty_keys, empty_order = ops.sort_keys_with_order(torch.empty((0,), dtype=torch.int32, device=DEV), 22)
    assert empty_keys.shape == empty_order.shape == (0,) and ops.sort_values(torch.empty((0,), device=DEV)).shape == (0,)


@pytest.mark.parametrize('count', COUNTS)
def test_sort_values_equals_torch_sort_bit_for_bit(count):
    x = torch.from_numpy(numpy.random.default_rng(count).standard_normal(count).astype(numpy.float32)).to(DEV)
    before = x.clone()
    got = ops.sort_values(x)
    assert got.dtype == torch.float32 and got.shape == (count,)
    assert torch.equal(got.view(torch.int32), torch.sort(x).values.view(torch.int32))
    assert torch.equal(x.view(torch.int32), before.view(torch.int32))


def key_of_float(bits: numpy.ndarray) -> numpy.ndarray:
    """The rule of the sort on the host: NaN -> the canonical quiet NaN; all bits of a negative value flipped, the sign bit otherwise."""
    bits = numpy.where((bits & numpy.uint32(0x7FFFFFFF)) > numpy.uint32(0x7F800000), numpy.uint32(0x7FC00000), bits).astype(numpy.uint32)
    return numpy.where(bits >> numpy.uint32(31) != 0, ~bits, bits ^ numpy.uint32(0x80000000)).astype(numpy.uint32)


def float_of_key(keys: numpy.ndarray) -> numpy.ndarray:
    return numpy.where(keys >> numpy.uint32(31) != 0, keys ^ numpy.uint32(0x80000000), ~keys).astype(numpy.uint32)


@pytest.mark.parametrize('count', (65, 3 * TILE + 17))
def test_sort_values_orders_the_special_values(count):
    """-inf, -1, denormals of both signs, -0 before +0, 1, +inf, then every NaN -- of either sign, quiet or signalling -- as the
    canonical quiet NaN."""
    rng = numpy.random.default_rng(count)
    specials = numpy.array([0xFF800000, 0xBF800000, 0x80000001, 0x80000400, 0x80000000, 0x00000000, 0x00000001, 0x00000400, 0x3F800000,
                            0x7F800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFC12345], dtype=numpy.uint32)
    bits = rng.standard_normal(count).astype(numpy.float32).view(numpy.uint32).copy()
    where = rng.permutation(count)[:min(count, 4 * len(specials))]
    bits[where] = numpy.resize(specials, len(where))
    want = float_of_key(numpy.sort(key_of_float(bits)))
    assert (want == 0x7FC00000).sum() == numpy.isnan(bits.view(numpy.float32)).sum() >= 6
    zeros = numpy.flatnonzero((want & 0x7FFFFFFF) == 0)
    assert len(zeros) >= 2 and want[zeros[0]] == 0x80000000 and want[zeros[-1]] == 0 and numpy.all(numpy.diff(want[zeros].astype(numpy.int64)) <= 0)
    x = torch.from_numpy(bits.view(numpy.int32)).to(DEV).view(torch.float32)
    got = ops.sort_values(x).view(torch.int32).cpu().numpy().view(numpy.uint32)
    assert numpy.array_equal(got, want)
    assert numpy.array_equal(x.view(torch.int32).cpu().numpy().view(numpy.uint32), bits)


@pytest.mark.parametrize('count', (3 * TILE + 17, 70001))
def test_two_calls_and_another_stream_return_the_same_bits(count):
    rng = numpy.random.default_rng(count)
    keys = torch.from_numpy(rng.integers(0, 8, count).astype(numpy.int32)).to(DEV)
    x = torch.from_numpy(rng.standard_normal(count).astype(numpy.float32)).to(DEV)
    y = torch.from_numpy(rng.standard_normal(count).astype(numpy.float32)).to(DEV)
    mask = torch.from_numpy(rng.random(count) < 0.5).to(DEV)

    def run():
        return (*ops.sort_keys_with_order(keys, 22), ops.sort_values(x), *ops.compact_pair(x, y, mask))

    first = [t.clone() for t in run()]
    second = run()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        third = run()
    stream.synchronize()
    for a, b, c in zip(first, second, third):
        raw = (lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t)
        assert torch.equal(raw(a), raw(b)) and torch.equal(raw(a), raw(c))


MASKS = ('none', 'all', 'half', 'sparse', 'bytes255', 'bytes1')


@pytest.mark.parametrize('count', COUNTS)
def test_compact_pair_keeps_the_masked_values_in_order(count):
    rng = numpy.random.default_rng(count + 7)
    a = rng.standard_normal(count).astype(numpy.float32)
    b = rng.standard_normal(count).astype(numpy.float32)
    a_dev, b_dev = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for kind in MASKS:
        if kind in ('none', 'all'):
            mask = numpy.full(count, kind == 'all')
        elif kind == 'sparse':
            mask = rng.random(count) < 0.01
        else:
            mask = rng.random(count) < 0.5
        if kind.startswith('bytes'):
            mask = mask.astype(numpy.uint8) * (255 if kind == 'bytes255' else 1)
        a_kept, b_kept = ops.compact_pair(a_dev, b_dev, torch.from_numpy(mask).to(DEV))
        keep = mask != 0
        assert a_kept.shape == b_kept.shape == (int(keep.sum()),), kind      # the count
        assert a_kept.is_contiguous() and a_kept.dtype == torch.float32
        assert numpy.array_equal(a_kept.cpu().numpy().view(numpy.int32), a[keep].view(numpy.int32)), kind
        assert numpy.array_equal(b_kept.cpu().numpy().view(numpy.int32), b[keep].view(numpy.int32)), kind
    assert numpy.array_equal(a_dev.cpu().numpy(), a) and numpy.array_equal(b_dev.cpu().numpy(), b)
