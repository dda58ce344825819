"""The tile decomposition of the path-A ARM (fwd_arm.hip, arm_tile_of: multiply-high-and-shift
constants instead of integer divisions, exported as ccmi_arm_tile_map) against plain integer
division, on the host: every tile id of a launch maps to one (frame, grid, first row, first
column), and the 8 x 64 tiles of a grid cover it exactly once."""
import ctypes as C

import numpy as np
import pytest

TY, TX = 8, 64
FRAMES = [(1, 1), (3, 5), (8, 64), (9, 65), (12, 137), (17, 200), (720, 1280), (1080, 1920)]
MAX_TILES = 2 ** 31 - 1     # what a launch accepts


def _sizes(hw, n):
    h, w = hw
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def per_frame_total(sizes):
    return sum(-(-w // TX) * -(-h // TY) for h, w in sizes)


def _map(lib, sizes, batch, first=0, count=None):
    """(rc, tile count of the launch, int array [count, 4]) of ccmi_arm_tile_map."""
    n = len(sizes)
    h = (C.c_int * n)(*[s[0] for s in sizes])
    w = (C.c_int * n)(*[s[1] for s in sizes])
    total = C.c_int64(-1)
    if count is None:
        rc = lib.ccmi_arm_tile_map(n, h, w, batch, 0, 0, None, C.byref(total))
        if rc:
            return rc, total.value, None
        count = total.value - first
    out = np.full((count, 4), -1, dtype=np.int32)
    rc = lib.ccmi_arm_tile_map(n, h, w, batch, first, count, out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(total))
    return rc, total.value, out


def _expect(sizes, ids):
    """The same by integer division (numpy int64 //, %), for the tile ids `ids`."""
    tiles_x = [-(-w // TX) for _, w in sizes]
    per_grid = [tx * -(-h // TY) for tx, (h, _) in zip(tiles_x, sizes)]
    start = np.concatenate([[0], np.cumsum(per_grid)]).astype(np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    b, t = ids // start[-1], ids % start[-1]
    grid = np.searchsorted(start, t, side="right") - 1
    lt = t - start[grid]
    tx = np.asarray(tiles_x, dtype=np.int64)[grid]
    return np.stack([b, grid, (lt // tx) * TY, (lt % tx) * TX], axis=1), int(start[-1])


@pytest.mark.parametrize("batch", [1, 3, 32])
@pytest.mark.parametrize("grids", [1, 2, 7])
@pytest.mark.parametrize("hw", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_tile_equals_integer_division(ccmi_lib, hw, grids, batch):
    sizes = _sizes(hw, grids)
    rc, total, got = _map(ccmi_lib, sizes, batch)
    want, per_frame = _expect(sizes, np.arange(per_frame_total(sizes) * batch))
    assert rc == 0 and total == per_frame * batch == len(got)
    assert np.array_equal(got, want)
    # one (frame, grid, y0, x0) per tile id, and the tiles of every grid cover it exactly once
    assert len(np.unique(got, axis=0)) == total
    for b in (0, batch - 1):
        for l, (h, w) in enumerate(sizes):
            cover = np.zeros((h, w), dtype=np.int32)
            for _, _, y0, x0 in got[(got[:, 0] == b) & (got[:, 1] == l)]:
                assert y0 < h and x0 < w
                cover[y0:y0 + TY, x0:x0 + TX] += 1
            assert bool((cover == 1).all()), (b, l)


def test_tiles_x_of_one_and_not_a_power_of_two(ccmi_lib):
    """Among the frames above: (3, 5) has tiles_x = 1 in every grid, (12, 137) has 3 and
    (1080, 1920) has 30, 15, 8, 4, 2, 1, 1."""
    assert [-(-w // TX) for _, w in _sizes((3, 5), 2)] == [1, 1]
    assert [-(-w // TX) for _, w in _sizes((12, 137), 1)] == [3]
    assert [-(-w // TX) for _, w in _sizes((1080, 1920), 7)] == [30, 15, 8, 4, 2, 1, 1]


LARGEST = [
    ([(1, 1)], MAX_TILES),                          # one tile a frame, 2^31 - 1 frames
    (_sizes((9, 65), 2), MAX_TILES // 5),           # 5 tiles a frame (not a power of two)
    (_sizes((12, 137), 3), MAX_TILES // 9),         # 6 + 2 + 1 tiles a frame, tiles_x 3, 2, 1
    (_sizes((1080, 1920), 7), MAX_TILES // per_frame_total(_sizes((1080, 1920), 7))),
    ([(8, 64 * 30000)], MAX_TILES // 30000),        # 30000 tiles in a row
]


@pytest.mark.parametrize("sizes,batch", LARGEST, ids=["1x1", "9x65", "12x137", "1080p", "wide"])
def test_largest_launch(ccmi_lib, sizes, batch):
    """The largest batch a launch of these grids accepts: its first tiles, its last ones and ids
    spread over the whole range; one frame more is refused."""
    per_frame = per_frame_total(sizes)
    total = per_frame * batch
    assert total <= MAX_TILES < total + per_frame
    rc, n, _ = _map(ccmi_lib, sizes, batch, count=0)
    assert rc == 0 and n == total
    rng = np.random.default_rng(per_frame)
    firsts = [0, total - 4096] + [int(x) for x in rng.integers(0, total - 4096, size=24)]
    for first in firsts:
        rc, _, got = _map(ccmi_lib, sizes, batch, first=first, count=4096)
        want, _ = _expect(sizes, first + np.arange(4096))
        assert rc == 0 and np.array_equal(got, want), first
    import ccmi
    if batch < MAX_TILES:  # (a batch is an int itself)
        rc, _, _ = _map(ccmi_lib, sizes, batch + 1, count=0)
        assert rc == ccmi.ERR_ARG and "tiles" in ccmi.last_error()
    rc, _, _ = _map(ccmi_lib, sizes, batch, first=total - 1, count=2)   # a tile past the launch
    assert rc == ccmi.ERR_ARG


def test_frame_of_too_many_latents_is_refused(ccmi_lib):
    import ccmi
    rc, n, _ = _map(ccmi_lib, [(32768, 32768)], 1, count=0)             # 2^30 latents: accepted
    assert rc == 0 and n == 4096 * 512
    rc, _, _ = _map(ccmi_lib, [(32768, 32768), (1, 1)], 1, count=0)     # one more
    assert rc == ccmi.ERR_ARG and "2^30" in ccmi.last_error()
    rc, _, _ = _map(ccmi_lib, [(3, 0)], 1, count=0)
    assert rc == ccmi.ERR_ARG
