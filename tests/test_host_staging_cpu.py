"""The layout of the two staging blocks of the synchronous host entries (`stage_layout`, csrc/bmpc_host_staging.hpp), as host clang
compiles it into an emulation library of its own (tests/emu/emu_staging.py).  The rules are stated here on their own -- not read
from the C side: every present slice starts on a 256-byte boundary, the slices follow each other in table order without overlap,
an absent row takes no room and reports absent, the block ends where the last present slice does, rounded up to 256."""
import itertools

import pytest

ALIGN = 256
SIZES = (1, 255, 256, 257, 48 * 257, 2 ** 33)          # bytes of a present row; 0 stands for an absent one


def check(rows):
    from tests.emu import emu_staging
    off, total = emu_staging.stage_layout(rows)
    assert len(off) == len(rows)
    end = 0                                             # where the last present slice ends
    for (present, size), o in zip(rows, off):
        if not present:
            assert o is None, rows
            continue
        assert o is not None and o % ALIGN == 0, rows
        assert o >= end, rows                           # table order, and clear of every slice before it
        end = o + size
    assert total == -(-end // ALIGN) * ALIGN, rows      # (no wrap: Python's integers, 2^33 included)
    return off, total


@pytest.mark.parametrize("shift", range(len(SIZES)))
def test_every_subset_of_a_five_row_table(shift):
    """Five rows whose sizes are five consecutive ones of {1, 255, 256, 257, 48 * 257, 2^33} (every rotation, so that each size
    stands first, last and after the 2^33 row), every subset of them present.  An absent row is given both as (absent, 0 bytes)
    and as (absent, its bytes): neither takes room."""
    sizes = [SIZES[(shift + i) % len(SIZES)] for i in range(5)]
    for mask in itertools.product((False, True), repeat=5):
        got = check([(p, s if p else 0) for p, s in zip(mask, sizes)])
        assert got == check([(p, s) for p, s in zip(mask, sizes)])
        if not any(mask):
            assert got == ([None] * 5, 0)


def test_tight_and_large():
    """The slices are as close as the boundary allows (the next present one starts at the end of the one before it, rounded
    up), and a row of 2^33 bytes moves the ones behind it past 2^33: the arithmetic is 64-bit."""
    off, total = check([(True, 1), (False, 0), (True, 256), (True, 257), (True, 2 ** 33), (True, 255), (True, 48 * 257)])
    assert off == [0, None, 256, 512, 1024, 1024 + 2 ** 33, 1280 + 2 ** 33]
    assert total == 1280 + 2 ** 33 + 12544 and total % ALIGN == 0 and 48 * 257 <= 12544 < 48 * 257 + ALIGN


def test_a_table_shaped_like_the_roll_out_outputs():
    """The seventeen outputs of `bmpc_rollout_out` at B = 3, S = 5, h = 10 (elements per instance x bytes per element, in the
    descriptor's order): all wanted, without the four ground rows, the reduced rows alone, and each row alone."""
    B, S, h = 3, 5, 10
    per_instance = [S * 8, S * 8, 12 * S * 4, 6 * S * 4, 12 * S * h * 4, S * 4, S * 4, S * 4, S * 4, 2 * S * 4, 2 * S * 4, S * 4, 4, 4,
                    S * 8, 12 * h * 8, 8]
    assert len(per_instance) == 17
    size = [B * w for w in per_instance]
    check([(True, s) for s in size])
    check([(not 8 <= i < 12, s) for i, s in enumerate(size)])
    check([(i >= 12, s) for i, s in enumerate(size)])
    for k in range(17):
        off, total = check([(i == k, s) for i, s in enumerate(size)])
        assert off[k] == 0 and total == -(-size[k] // ALIGN) * ALIGN
