"""The host halves of the post-processing chain, called in the built library without a GPU: dm_nms_reduce (the greedy
pass over a suppression bit matrix) and dm_rle_string (run boundaries -> COCO's printable counts), each against a plain
Python restatement, and the refusal of more than 65535 masks by the three entry points that launch one grid row per
mask.  Every output buffer is longer than the call may use and starts as a canary: what lies past the result must stay."""
import ctypes

import numpy as np
import pytest

from oracle import ref_ops

VP = ctypes.c_void_p
INVALID_ARG = -1                  # DM_ERR_INVALID_ARG of include/dynamask_hip.h
KEEP_CANARY = -77
CHAR_CANARY = 0x7f                # no byte of a counts string: those lie in [48, 111]


def _lib():
    from dynamask_amd._lib import lib
    return lib()


def _ptr(a):
    return VP(a.ctypes.data)


# ------------------------------------------------------------------------------------------------ dm_nms_reduce
def random_upper_bits(M, density, seed):
    """[M, M] bool, True only above the diagonal."""
    rng = np.random.default_rng(seed)
    return np.triu(rng.random((M, M)) < density, 1)


def pack_rows(bits):
    """[M, M] bool -> the row-major [M, ceil(M / 64)] uint64 matrix of dm_nms_mask: bit j & 63 of word j >> 6 of row i."""
    M = bits.shape[0]
    words = (M + 63) // 64
    padded = np.zeros((M, words * 64), dtype=np.uint8)
    padded[:, :M] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view('<u8').reshape(M, words)


def greedy_walk(bits, max_keep):
    """Walk the boxes in order; keep one unless an earlier kept box suppresses it; stop before keeping more than
    ``max_keep`` (< 0: no limit)."""
    M = bits.shape[0]
    removed = np.zeros(M, dtype=bool)
    keep = []
    for i in range(M):
        if removed[i]:
            continue
        if 0 <= max_keep <= len(keep):
            break
        keep.append(i)
        removed |= bits[i]
    return keep


def max_keeps(bits):
    unlimited = len(greedy_walk(bits, -1))
    return [-1, 1, 63, 64, 65, unlimited, unlimited + 1]


def _reduce(mask, M, max_keep):
    keep = np.full(M + 8, KEEP_CANARY, dtype=np.int32)
    n = _lib().dm_nms_reduce(_ptr(mask), M, _ptr(keep), max_keep)
    return n, keep


@pytest.mark.parametrize('M', [1, 63, 64, 65, 128, 129, 1000, 4161])
def test_nms_reduce_equals_the_greedy_walk(M):
    """M = 4161 is 66 words.  max_keep on both sides of a word and at the unlimited count and one past it."""
    for density in (0.0, 0.002, 0.05, 0.9):
        bits = random_upper_bits(M, density, seed=1000 * M + int(density * 1000))
        mask = pack_rows(bits)
        for max_keep in max_keeps(bits):
            want = greedy_walk(bits, max_keep)
            n, keep = _reduce(mask, M, max_keep)
            what = f'M {M}, density {density}, max_keep {max_keep}'
            assert n == len(want), what
            assert keep[:n].tolist() == want, what
            assert bool((keep[n:] == KEEP_CANARY).all()), f'{what}: keep was written past the count'


def test_nms_reduce_heap_path():
    """More than 1024 words (M = 65 600, 1025 words): the removed bits live on the heap.  A zero matrix with a few hundred
    set bits; the walk restated on the set bits alone."""
    M, words = 65600, 1025
    rng = np.random.default_rng(65600)
    mask = np.zeros((M, words), dtype='<u8')
    ii = rng.integers(0, M - 1, size=400)
    jj = np.array([rng.integers(i + 1, M) for i in ii])
    ii = np.concatenate([ii, [0, 5, 65000]])                    # the last word, and a bit in the word of its own row
    jj = np.concatenate([jj, [M - 1, 6, 65599]])
    suppresses = {}
    for i, j in zip(ii.tolist(), jj.tolist()):
        mask[i, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
        suppresses.setdefault(i, []).append(j)
    for max_keep in (-1, 40000):
        removed, want = set(), []
        for i in range(M):
            if i in removed:
                continue
            if 0 <= max_keep <= len(want):
                break
            want.append(i)
            removed.update(suppresses.get(i, ()))
        assert len(want) < M
        n, keep = _reduce(mask, M, max_keep)
        assert n == len(want)
        assert np.array_equal(keep[:n], np.asarray(want, dtype=np.int32))
        assert bool((keep[n:] == KEEP_CANARY).all())


def test_nms_reduce_of_nothing():
    assert _lib().dm_nms_reduce(None, 0, None, -1) == 0


# ------------------------------------------------------------------------------------------------ dm_rle_string
def counts_of(positions, total):
    """Run boundaries (column-major positions where the value changes; the value before position 0 is 0) -> run lengths."""
    edges = [0] + [int(p) for p in positions] + [int(total)]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def _rle_string(positions, total, cap):
    pos = np.asarray(positions, dtype=np.int32)
    raw = (ctypes.c_char * (max(cap, 0) + 16))(*([CHAR_CANARY] * (max(cap, 0) + 16)))
    n = _lib().dm_rle_string(_ptr(pos) if len(pos) else None, len(pos), int(total), raw, int(cap))
    return n, np.frombuffer(raw, dtype=np.uint8).copy()


def _rle_cases(total):
    """Boundary lists for a mask of ``total`` pixels: none, one at 0, one at total - 1, both, every pixel (small masks),
    random ones, and runs that shrink so that the difference to the count two back is negative."""
    rng = np.random.default_rng(total % 1000003)
    cases = [[], [0], [total - 1]]
    if total >= 2:
        cases.append([0, total - 1])
    if total <= 4096:
        cases.append(list(range(total)))
    for k in (1, 2, 3, 4, 7, 50, 333):
        if k <= total:
            cases.append(np.sort(rng.choice(total, size=k, replace=False) if total <= 10 ** 6
                                 else np.unique(rng.integers(0, total, size=k))).tolist())
    if total >= 4096:
        # counts 1000, 900, 3, 2, 1, 1, ...: from the third on, most differences to two back are negative
        shrinking = np.cumsum([1000, 900, 3, 2, 1, 1, 700, 1, 1]).tolist()
        cases.append(shrinking)
        cases.append([total - 1 - p for p in reversed(shrinking)])
    return cases


@pytest.mark.parametrize('total', [1, 5, 4096, 10 ** 6, 2 ** 31 - 1])
def test_rle_string_equals_the_oracle(total):
    negative = 0
    for positions in _rle_cases(total):
        cnts = counts_of(positions, total)
        negative += sum(1 for i in range(3, len(cnts)) if cnts[i] < cnts[i - 2])
        want = ref_ops.rle_to_string(cnts)
        assert ref_ops.rle_from_string(want) == cnts
        n, buf = _rle_string(positions, total, len(want))
        what = f'total {total}, {len(positions)} boundaries'
        assert n == len(want), what
        assert buf[:n].tobytes() == want, what
        assert bool((buf[n:] == CHAR_CANARY).all()), f'{what}: written past the string'
        # one byte short: -(needed), and nothing at or past cap
        n, buf = _rle_string(positions, total, len(want) - 1)
        assert n == -len(want), what
        assert buf[:len(want) - 1].tobytes() == want[:-1], what
        assert bool((buf[len(want) - 1:] == CHAR_CANARY).all()), f'{what}: written at or past cap'
    assert total < 4096 or negative > 0


# ------------------------------------------------------------------------------------------------ argument validation
def test_more_masks_than_grid_rows_are_refused_before_any_launch():
    """dm_paste_masks, dm_rle_encode_canvas and dm_paste_rle launch dim3(., N): N > 65535 is DM_ERR_INVALID_ARG, decided
    before a pointer is read or a kernel launched (the pointers here point nowhere)."""
    L = _lib()
    p = VP(4096)
    for N, want in ((65536, INVALID_ARG), (2 ** 31 - 1, INVALID_ARG)):
        assert L.dm_paste_masks(p, p, N, 28, 28, 8, 8, 0.5, 0, p, None) == want
        assert L.dm_rle_encode_canvas(p, N, 8, 8, p, p, p, p, 16, None) == want
        assert L.dm_paste_rle(p, p, N, 28, 28, 8, 8, 0.5, 0, p, p, p, p, 16, None) == want
    # the multi-image forms have always refused it
    assert L.dm_paste_masks_multi(p, p, 65536, 28, 28, p, 1, p, 64, 0.5, 0, p, None) == INVALID_ARG
    assert L.dm_paste_rle_multi(p, p, 65536, 28, 28, p, 1, p, 64, 0.5, 0, p, p, p, p, 16, None) == INVALID_ARG


def test_ops_wrappers_name_the_mask_limit():
    from dynamask_amd import ops
    assert ops.MAX_MASKS_PER_LAUNCH == 65535
    ops._chk_mask_count(65535, 'paste_masks')
    with pytest.raises(ValueError, match='65536 masks.*at most 65535'):
        ops._chk_mask_count(65536, 'paste_masks')
