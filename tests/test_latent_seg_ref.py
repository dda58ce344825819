"""tests/latent_seg_ref.py, the numpy restatement of the segmented latent-store form
(CCMI_LATENT_SEG): round trips at every width boundary and every partial-segment width,
hand-written words, and the sizes it gives for the oracle's latents of one class-D stream."""
from pathlib import Path

import numpy as np
import pytest

import latent_seg_ref as R

ROOT = Path(__file__).resolve().parents[1]
COOL = ROOT / "tests" / "golden" / "cool"

# (lowest, highest) value pairs and the code each needs
BOUNDARIES = [((0, 0), 0), ((-1, 0), 1), ((0, 1), 1), ((-2, 1), 1), ((-3, 0), 2), ((0, 2), 2), ((-8, 7), 2),
              ((-9, 0), 3), ((0, 8), 3), ((-128, 127), 3), ((-129, 0), 4), ((0, 128), 4), ((-32768, 32767), 4),
              ((-32769, 0), 5), ((0, 32768), 5), ((-2 ** 31, 2 ** 31 - 1), 5)]


@pytest.mark.parametrize("pair,code", BOUNDARIES)
def test_width_boundaries_round_trip(pair, code):
    lo, hi = pair
    for w in (64, 22):
        for at_lo, at_hi in ((0, w - 1), (w - 1, 0), (w // 2, w // 2 + 1)):
            g = np.zeros((1, w), dtype=np.int64)
            g[0, at_hi] = hi
            g[0, at_lo] = lo
            desc, words = R.pack_grid(g)
            assert int(desc[0]) == code, (pair, w, at_lo, at_hi)  # offset 0
            assert len(words) == (w * R.WIDTHS[code] + 31) // 32
            assert np.array_equal(R.unpack_grid(desc, words, 1, w), g)


@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 128, 150])
def test_round_trip_over_widths_and_random_data(w):
    rng = np.random.default_rng(1000 + w)
    h = 5
    nseg = (w + 63) // 64
    # every segment draws from a range of its own: all six codes occur over the rows
    g = np.zeros((h, w), dtype=np.int64)
    spans = [0, 1, 7, 100, 30000, 2 ** 31 - 1]
    for r in range(h):
        for s in range(nseg):
            span = spans[(r + s) % 6]
            c = min(64 * s + 64, w) - 64 * s
            g[r, 64 * s: 64 * s + c] = rng.integers(-span - 1, span + 1, size=c) if span else 0
    desc, words = R.pack_grid(g)
    assert desc.dtype == np.uint32 and words.dtype == np.uint32 and len(desc) == h * nseg
    # offsets: the words before each segment, in (r, s) order, no gaps
    off = 0
    for i, d in enumerate(desc):
        c = min(64 * (i % nseg) + 64, w) - 64 * (i % nseg)
        assert int(d) >> 3 == off
        off += (c * R.WIDTHS[int(d) & 7] + 31) // 32
    assert off == len(words)
    assert np.array_equal(R.unpack_grid(desc, words, h, w), g)
    # determined by the values alone
    d2, w2 = R.pack_grid(g.astype(np.int32))
    assert np.array_equal(desc, d2) and np.array_equal(words, w2)


def test_hand_written_words():
    # 2 bits: 64 values 1, -1, -2, 0 repeating -> fields 01, 11, 10, 00 from bit 0: byte 0b00101101 = 0x2D
    g = np.tile(np.array([1, -1, -2, 0]), 16).reshape(1, 64)
    desc, words = R.pack_grid(g)
    assert list(desc) == [1] and [hex(x) for x in words] == ["0x2d2d2d2d"] * 4
    # 4 bits, a partial segment of 11 values after a full all-zero one: 7, -8, -1, 3, 0, 0, 0, 0, 1, 2, -3
    g = np.zeros((1, 75), dtype=np.int64)
    g[0, 64:] = [7, -8, -1, 3, 0, 0, 0, 0, 1, 2, -3]
    desc, words = R.pack_grid(g)
    assert list(desc) == [0, (0 << 3) | 2]
    assert [hex(x) for x in words] == ["0x3f87", "0xd21"]  # the last word's trailing 20 bits are 0
    # a second row starts where the first ends
    g2 = np.vstack([g, g])
    desc, words = R.pack_grid(g2)
    assert list(desc) == [0, 2, 2 << 3, (2 << 3) | 2] and len(words) == 4


def test_sizes_for_a_class_d_stream(oracle_c):
    """The oracle's latents of one committed 416 x 240 stream: the round trip, and the store
    bytes against the int16 and int8 forms (no stream of the set needs more than int8)."""
    from test_encode import oracle_latents
    f = sorted(COOL.glob("D-*.cool"))[0]
    sizes, lat, _, _ = oracle_latents(oracle_c, f.read_bytes(), with_params=False)
    seg = i8 = i16 = 0
    for (h, w), v in zip(sizes, lat):
        g = v.reshape(h, w)
        desc, words = R.pack_grid(g)
        assert np.array_equal(R.unpack_grid(desc, words, h, w), g)
        assert max(int(d) & 7 for d in desc) <= 3
        seg += R.grid_bytes(desc, words)
        i8 += R.align(h * w, 16)
        i16 += R.align(2 * h * w, 16)
    print(f"{f.name}: latents at int16 {i16} bytes, int8 {i8}, segmented {seg} ({seg / i16:.3f} of int16)")
    assert seg < i8 < i16
