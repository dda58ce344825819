"""The bit-exact .cool decoder over generated streams: architecture x geometry against the oracle.

Every comparison is between integers and exact.  tests/cool_gen.py draws a stream from
nothing (header, networks, latents); the GPU writer codes it; the C oracle (plain loops, any
architecture) decodes it; the HIP decoder must give the oracle's latents, synthesis input,
synthesis output and output bytes, in a batch and alone.

What the committed streams hold (encode.parse over tests/golden/**/*.cool, 93 streams; layers as
n_out-ks, r = residual, a = ReLU; frame type 0 rgb / 1 yuv420):

  grids d  nh ups pre n_ups n_pre layers                  br type blk  max|syn w| streams sizes
  7     8  0  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1     8   7136       1       1
  7     8  1  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1     0   7136       1       1
  7     8  1  8   7   6     6     8-1a|3-1|3-3r           1  0   -16   3472       1       1
  7     8  1  8   7   6     6     8-1a|3-1|3-3r           1  1   -16   9600       4       1
  7     8  2  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  0   -16   7360       5       3
  7     8  2  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1   -16   9120       4       1
  7     16 0  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1   -16   7136       1       1
  7     16 2  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  0   -16   12848      4       3
  7     16 2  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1   -16   13504      13      2
  7     16 2  8   7   6     6     48-1a|3-1|3-3ra|3-3r    1  0   -16   13848      33      3
  7     16 2  8   7   6     6     48-1a|3-1|3-3ra|3-3r    1  1   -16   17872      22      3
  7     16 3  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1     8   7136       1       1
  7     24 2  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1   -16   7136       1       1
  7     32 0  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1     0   7136       1       1
  7     32 1  8   7   6     6     16-1a|3-1|3-3ra|3-3r    1  1   -16   7136       1       1

So: one grid count (7), one upsampling (8 / 7, six kernels each), one branch, no synthesis weight
near 2^23 (the largest is 17872), heads of 8, 16 and 48, and two stacks.  One listed gap is
partly covered already: n_sp = 1 runs in five committed streams (8-1a|3-1|3-3r), with one
residual/ReLU pattern; its cases stay here.  Nine (d, nh) ARM pairs run, none with nh = 4.

Picture checks.  Before any GPU comparison every case's oracle planes (syn_out, before the
clamp, unit 1 << 12) must show a picture: half of the samples of planes 0..2 strictly inside
(0, unit), 64 distinct values per plane, a sample below 0 and one above the unit.  Where the
sample count or the arithmetic leaves no room, and only there, a check is stated as follows:
  * a plane of fewer than 64 samples (1x1, 2x3) must hold as many distinct values as samples;
  * frames of fewer than 64 samples (1x1, 2x3) need not reach both clamps;
  * a one-branch stack whose last layer has a ReLU never goes below 0: it must hold a sample
    equal to 0 (the ReLU acted) in place of one below 0.
test_generated_cases_show_a_picture checks the same on the CPU, on the oracle's stage wrappers
fed with the generator's networks, so a draw that degenerates fails without a GPU.

What the lists reach: 21 of the 28 ARM launches a build can take (all 8 chain and 10
one-latent (d, nh), the speculative kernel for nh = 0 and, in test_decode_arch_wide_gpu.py, for
(16, 2) past the chain kernel's LDS bound); 64 (CIN, F24, n_sp) forms of the fused synthesis (30 of
the batch kernel, 30 of the single-frame one, 4 of the window one; the committed streams reach
(7, on, 1) and (7, on, 2)); generic layers of kernel size 1, 3, 5 and 7; blends of 2, 3 and 8
branches; 8 upsampling pairs.  Which lists answer to which arithmetic: the F24 choice of the
batch kernel to the f24, roi and mixed lists (a weight outside 24 bits); the residual term of a
3x3 layer to every list with that layer; the padding of the 2x upsampling, pad = ks / 2 with
ks = ups_k / 2, to the lists with ups_k = 4 or 8 where ks is even, and to those with 6, 10 or 14
where it is odd.
"""
import ctypes as C
import itertools
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import cool_gen as G

ROOT = Path(__file__).resolve().parents[1]
UNIT = 1 << 12


# ---------------------------------------------------------------- the oracle
class _Frame(C.Structure):
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("frame_data_type", C.c_int), ("bitdepth", C.c_int),
                ("n_layers", C.c_int), ("lh", C.c_int * 8), ("lw", C.c_int * 8),
                ("lat", C.POINTER(C.c_int32) * 8), ("syn_in", C.POINTER(C.c_int32)), ("n_out", C.c_int),
                ("syn_out", C.POINTER(C.c_int32)), ("t_arm", C.c_double), ("t_ups", C.c_double), ("t_syn", C.c_double)]


@lru_cache(maxsize=None)
def oracle():
    """The oracle library with the stage wrappers bound; rebuilt first (make decides) since a
    library from before the wrappers would load and lack them."""
    subprocess.run(["make", "-s", "-C", str(ROOT / "oracle")], check=True)
    L = C.CDLL(str(ROOT / "oracle" / "_build" / "libccoracle.so"))
    P, I = C.c_void_p, C.c_int
    L.cco_decode_frame_mem.argtypes = [P, C.c_size_t, P]
    L.cco_frame_free.argtypes = [P]
    L.cco_output_size.argtypes = [P, I, I, I]
    L.cco_output_size.restype = C.c_size_t
    L.cco_write_output.argtypes = [P, I, I, I, P]
    L.cco_ups_forward.argtypes = [I, P, P, P, I, I, I, I, P, P]
    L.cco_syn_forward.argtypes = [I, I, I, I, P, P, P, P]
    return L


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def oracle_ups(lat_q8, sizes, kernels, ups_k, n_ups, pre_k, n_pre):
    """cco_ups_forward: lat_q8 flat int32 (value << 8) -> [L, H, W] int32."""
    lh, lw = _i32([s[0] for s in sizes]), _i32([s[1] for s in sizes])
    lat_q8, kernels = _i32(lat_q8), _i32(kernels)
    out = np.zeros((len(sizes), sizes[0][0], sizes[0][1]), dtype=np.int32)
    assert oracle().cco_ups_forward(len(sizes), lh.ctypes.data, lw.ctypes.data, lat_q8.ctypes.data, ups_k, n_ups, pre_k,
                                    n_pre, kernels.ctypes.data, out.ctypes.data) == 0
    return out


def oracle_syn(x, layers, params):
    """cco_syn_forward: x [C, H, W] int32, layers [(n_out, ks, residual, relu)] -> [n_out, H, W]."""
    x, params = _i32(x), _i32(params)
    lay = _i32([[n, k, int(bool(r)), int(bool(a))] for n, k, r, a in layers])
    out = np.zeros((layers[-1][0], x.shape[1], x.shape[2]), dtype=np.int32)
    assert oracle().cco_syn_forward(x.shape[0], x.shape[1], x.shape[2], len(layers), lay.ctypes.data, params.ctypes.data,
                                    x.ctypes.data, out.ctypes.data) == 0
    return out


def oracle_decode(data, formats=()):
    """cco_decode_frame_mem: (sizes, latents << 8 flat, syn_in, syn_out, [bytes per (bitdepth,
    chroma, is_yuv) of formats])."""
    L = oracle()
    fr = _Frame()
    buf = C.create_string_buffer(data, len(data))
    assert L.cco_decode_frame_mem(buf, len(data), C.byref(fr)) == 0, "the oracle refuses the stream"
    try:
        sizes = [(fr.lh[l], fr.lw[l]) for l in range(fr.n_layers)]
        lat = np.concatenate([np.ctypeslib.as_array(fr.lat[l], shape=(h * w,)).copy() for l, (h, w) in enumerate(sizes)])
        npx = fr.h * fr.w
        syn_in = np.ctypeslib.as_array(fr.syn_in, shape=(fr.n_layers * npx,)).copy().reshape(fr.n_layers, fr.h, fr.w)
        syn_out = np.ctypeslib.as_array(fr.syn_out, shape=(fr.n_out * npx,)).copy().reshape(fr.n_out, fr.h, fr.w)
        outs = []
        for bd, chroma, yuv in formats:
            bd = bd or fr.bitdepth
            chroma = chroma or (420 if fr.frame_data_type == 1 else 444)
            o = C.create_string_buffer(L.cco_output_size(C.byref(fr), bd, chroma, int(yuv)) + 64)
            n = L.cco_output_size(C.byref(fr), bd, chroma, int(yuv))
            assert L.cco_write_output(C.byref(fr), bd, chroma, int(yuv), o) == 0
            outs.append(o.raw[:n])
        return sizes, lat, syn_in, syn_out, outs
    finally:
        L.cco_frame_free(C.byref(fr))


def oracle_tail(frame, lat):
    """The oracle's syn_in / syn_out of a generated frame without a stream: the stage wrappers on
    the generator's decoded networks; branches blended as run_syn does."""
    d = frame.desc
    nets = G.decoded_nets(frame)
    flat = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in lat]) << 8
    syn_in = oracle_ups(flat, frame.grid_sizes, nets["ups"], d.ups_k, d.n_ups, d.pre_k, d.n_pre)
    layers = G.layers_of(d)
    per = len(nets["syn"]) // d.n_branches
    outs = [oracle_syn(syn_in, layers, nets["syn"][b * per: (b + 1) * per]) for b in range(d.n_branches)]
    if d.n_branches == 1:
        return syn_in, outs[0]
    bl = [int(v) for v in nets["blend"]]
    cl = [np.clip(o[:3].astype(np.int64), 0, UNIT) for o in outs]
    acc = (cl[0] * bl[0] + cl[1] * bl[1]) >> 12
    for b in range(2, d.n_branches):
        acc = acc + ((cl[b] * bl[b]) >> 12)
    return syn_in, acc.astype(np.int32)


def assert_picture(syn_out, layers, name, n_branches=1):
    """The module docstring's picture checks on pre-clamp planes."""
    p = np.asarray(syn_out)[:3].astype(np.int64)
    npx = p.shape[1] * p.shape[2]
    inside = np.count_nonzero((p > 0) & (p < UNIT))
    assert 2 * inside >= p.size, f"{name}: {inside} of {p.size} samples inside (0, unit)"
    need = min(64, npx)  # a plane of fewer than 64 samples: every sample distinct
    for c in range(3):
        assert len(np.unique(p[c])) >= need, f"{name}: plane {c} holds {len(np.unique(p[c]))} values"
    if npx >= 64:
        assert (p > UNIT).any(), f"{name}: no sample above the unit"
        if n_branches == 1 and G._flags(layers)[-1][1]:
            assert (p == 0).any(), f"{name}: the last layer's ReLU never acts"
        else:
            assert (p < 0).any(), f"{name}: no sample below 0"


# ---------------------------------------------------------------- cases
def fused(hid, sp=()):
    """hid-1 ReLU | 3-1 | 3-3 per entry of sp = ((residual, relu), ...): the fused form."""
    return [(hid, 1, 0, 1), (3, 1, 0, 0)] + [(3, 3, int(r), int(a)) for r, a in sp]


PRESET = ((1, 1), (1, 0), (1, 0))  # 3x3 layers of the presets: residual ReLU, then residual linear


def case(H, W, layers=None, *, n_grids=7, d=16, nh=2, ups=(8, 7), n_ups=None, n_pre=None, **kw):
    """make() arguments of one stream; odd sizes are rgb, even ones yuv420."""
    c = dict(H=H, W=W, n_grids=n_grids, dim_arm=d, n_hidden=nh, ups_k=ups[0], pre_k=ups[1],
             n_ups=n_ups or n_grids - 1, n_pre=n_pre or n_grids - 1, layers=layers or fused(16, PRESET[:2]),
             frame_type="rgb" if (H | W) & 1 else "yuv420")
    c.update(kw)
    return c


def _tile(n):
    return 32 - 2 * n, 64 - 2 * n


# one fused tile is (32 - 2 n_sp) x (64 - 2 n_sp): exactly one tile, and one more row and column
# (a second tile in both directions, of one sample); at that size every residual/ReLU pattern of
# the 3x3 layers, among them a plain ReLU layer followed by a residual linear one
SYN_TILES = {}
for _n in range(4):
    _h, _w = _tile(_n)
    _pat = list(itertools.product(((0, 0), (0, 1), (1, 0), (1, 1)), repeat=_n))
    # the exact tile twice (another head): lists decode per frame type, and this is the only even size
    _l = [case(_h, _w, fused(16, PRESET[:_n])), case(_h, _w, fused(40, PRESET[:_n]))] + \
        [case(_h + 1, _w + 1, fused(16, p)) for p in _pat]
    for _i in range(0, len(_l), 17):
        SYN_TILES[f"nsp{_n}_{_i // 17}"] = _l[_i: _i + 17]
# frames smaller than any tile, of one row, of one column: fewer grids where a grid would repeat 1x1
SYN_TILES["tiny"] = [case(1, 1, n_grids=2), case(2, 3, n_grids=3), case(1, 70, n_grids=7), case(70, 1, n_grids=7),
                     case(1, 70, fused(16), n_grids=4), case(70, 1, fused(16, PRESET), n_grids=5)]

# dec_syn_fused<CIN, 3>: every grid count, 45 x 83 is odd at every level; head widths up to the
# widest a header byte holds (48 > 40: the preset's widest; 255 stays in registers, hid * 12 <= 6144)
# every grid count meets every n_sp, so that each dec_syn_fused<CIN, 3> runs with each tile size
CIN = {f"grids{g}": [case(45, 83, fused(hid, PRESET[:n]), n_grids=g)
                     for hid, n in ((1, 2), (3, 0), (16, 1), (40, 3), (48, 2), (255, 1))] for g in range(2, 9)}

# the F24 switch: one weight at each side of both ends of 24 signed bits, and one far outside, in
# layer 0, in layer 1 and in the last 3x3 layer; the first stream has small weights only (F24 on)
BIG = ((1 << 23) - 1, 1 << 23, -(1 << 23), -(1 << 23) - 1, 1 << 27)
F24 = {"nsp2": [case(45, 83)] + [case(45, 83, big_syn_weight=v, big_layer=l) for l in (0, 1, 3) for v in BIG],
       "nsp0": [case(45, 83, fused(16))] + [case(45, 83, fused(16), big_syn_weight=v, big_layer=0) for v in BIG]}

# the per-frame tail (dec_syn_layer / dec_syn_fused_generic / dec_blend_kernel)
TAIL_STACKS = {
    "k135": dict(layers=[(9, 1, 0, 1), (6, 3, 0, 1), (3, 5, 0, 0)]),           # 1x1 alone, 3x3, 5x5
    "first3x3": dict(layers=[(8, 3, 0, 1), (3, 1, 0, 0)]),                     # first layer spatial
    "k7": dict(layers=[(16, 1, 0, 1), (3, 1, 0, 0), (3, 3, 1, 1), (3, 7, 1, 0)]),  # fused pair, then 3x3 and 7x7
    "wide5": dict(layers=[(16, 1, 0, 1), (5, 1, 0, 0), (5, 3, 1, 0)]),         # five planes out, three count
    "nsp4": dict(layers=fused(16, PRESET + ((1, 0),))),                        # one 3x3 layer past kMaxSp
    "br2": dict(layers=fused(16, PRESET[:2]), n_branches=2),                   # branches over a fused stack
    "br3": dict(layers=fused(16, PRESET[:2]), n_branches=3),
    "br8": dict(layers=fused(8, PRESET[:1]), n_branches=8),
    "br2g": dict(layers=[(8, 3, 0, 1), (3, 1, 0, 0)], n_branches=2),           # ... over a generic stack
    "br3g": dict(layers=[(8, 3, 0, 1), (3, 1, 0, 0)], n_branches=3),
    "br8g": dict(layers=[(6, 1, 0, 1), (3, 3, 0, 0)], n_branches=8),
}
# each size: the stacks, and two batchable streams of the same geometry in the same call
TAIL = {f"{h}x{w}": [case(h, w, n_grids=5, **a) for a in TAIL_STACKS.values()] + [case(h, w, n_grids=5), case(h, w, fused(8, PRESET[:1]), n_grids=5)]
        for h, w in ((21, 37), (33, 65))}

# dec_ups_level: ks = ups_k / 2 taps per phase, pad = ks / 2 (odd ks for 6, 10, 14); (14, 15) is
# the largest pair a header carries (4-bit fields, ups_k even; the decoder takes ups_k <= 16 and
# pre_k <= 15).  17 x 65 and 33 x 129: the first row and column of a second 16 x 64 tile, at
# levels 0 and 1
UPS_PAIRS = ((4, 1), (4, 3), (6, 5), (8, 1), (8, 9), (10, 7), (14, 15))
UPS = {f"u{u}p{p}": [case(17, 65, ups=(u, p), n_grids=6), case(33, 129, ups=(u, p)), case(45, 83, ups=(u, p)),
                     case(1, 70, ups=(u, p), n_grids=5), case(70, 1, ups=(u, p), n_grids=5)] for u, p in UPS_PAIRS}
# (L - 2 - k) % n: fewer kernels than levels, every kernel drawn apart, so a wrong modulo shows
UPS["modulo"] = [case(45, 83, n_grids=6, n_ups=a, n_pre=b, ups=(6, 5)) for a in (1, 2, 5) for b in (1, 2, 5)]

# launch_dec_arm: every (d, nh); 9 x 131 with 3 grids has rows of 131 / 66 / 33 latents, which
# cross the chain kernel's 64-latent chunks at 64 | 65 and 128 | 129
ARM_PAIRS = [(d, nh) for d in (8, 16, 24, 32) for nh in range(5)]
ARM = {"product": [case(9, 131, n_grids=3, d=d, nh=nh, hls_sig_blksize=(-16, 8, 0)[i % 3]) for i, (d, nh) in enumerate(ARM_PAIRS)],
       # rows of 1, 2, 3, 5 latents and 64 | 65: one ARM per kernel (chain, speculative, one-latent)
       "narrow": [case(40, 1, n_grids=3, d=16, nh=2), case(40, 2, n_grids=3, d=8, nh=4), case(40, 3, n_grids=3, d=8, nh=0),
                  case(40, 5, n_grids=3, d=16, nh=0), case(3, 64, n_grids=3, d=24, nh=1), case(3, 65, n_grids=3, d=32, nh=4)]}

# dec_tail_same_group: four architectures of one geometry and grid count (head width, residual
# flags, F24 and upsampling kernel sizes differ), and two of another n_sp
MIXED = {"groups": [case(34, 66, fused(16, ((1, 1), (1, 0)))), case(34, 66, fused(40, ((0, 1), (1, 0)))),
                    case(34, 66, fused(3, ((0, 0), (0, 0))), ups=(4, 3)), case(34, 66, big_syn_weight=1 << 23, big_layer=0, ups=(10, 7)),
                    case(34, 66, fused(16, PRESET[:1])), case(34, 66, fused(16, PRESET))]}

# regions and latent stores (tests/test_decode_arch_roi_gpu.py): dec_roi_plan derives every window
# from the upsampling taps and the synthesis halo; the last stream of a list takes the per-frame tail
ROI = {f"{h}x{w}": [case(h, w, fused(16, PRESET[:n]), ups=u) for u in ((4, 3), (6, 5), (10, 7)) for n in (0, 1, 3)] +
       [case(h, w, big_syn_weight=-(1 << 23) - 1, big_layer=1), case(h, w, **TAIL_STACKS["k135"])] for h, w in ((34, 66), (45, 83))}

GROUPS = {"tiles": SYN_TILES, "cin": CIN, "f24": F24, "tail": TAIL, "ups": UPS, "arm": ARM, "mixed": MIXED, "roi": ROI}
LISTS = {f"{g}-{k}": v for g, d in GROUPS.items() for k, v in d.items()}
_SEED = {}
for _k, _v in LISTS.items():
    for _i, _c in enumerate(_v):
        _c.setdefault("seed", 1000 * len(_SEED) + _i)
    _SEED[_k] = True


@lru_cache(maxsize=None)
def made(key):
    """[(CoolFrame, latents)] of a case list: drawn once, shared, left unchanged."""
    return [G.make(**c) for c in LISTS[key]]


# ---------------------------------------------------------------- CPU: the generator
def test_generator_slots_sizes_bounds_and_seed():
    for key in ("tiles-nsp2_0", "tail-21x37", "ups-u14p15", "arm-product", "f24-nsp0"):
        for c, (fr, lat) in zip(LISTS[key], made(key)):
            d = fr.desc
            # slot lengths from the header's arithmetic, written out apart from the generator
            arm_w = d.n_hidden_arm * d.dim_arm ** 2 + 2 * d.dim_arm
            syn_w, cin = (d.n_branches if d.n_branches > 1 else 0), d.n_grids
            for n_out, ks, _, _ in c["layers"]:
                syn_w += d.n_branches * n_out * cin * ks * ks
                cin = n_out
            want = {"arm_w": arm_w, "arm_b": d.n_hidden_arm * d.dim_arm + 2, "ups_b": 0,
                    "ups_w": d.n_ups * ((d.ups_k + 1) // 2) + d.n_pre * ((d.pre_k + 1) // 2),
                    "syn_w": syn_w, "syn_b": d.n_branches * sum(l[0] for l in c["layers"])}
            assert {k: len(v) for k, v in fr.nn.items()} == want == G.slot_lengths(d)
            h, w = c["H"], c["W"]
            for l, (gh, gw) in enumerate(fr.grid_sizes):
                assert (gh, gw) == (-(-h // 2 ** l), -(-w // 2 ** l)) and lat[l].shape == (gh * gw,)
            assert lat[0].any() and lat[1].any() and lat[0].dtype == np.int32
            assert max(int(np.abs(a).max()) for a in lat) < d.ac_max_val_latent <= 16
            top = max(int(np.abs(v).max(initial=0)) for v in fr.nn.values())
            assert d.ac_max_val_nn == min(65535, top + 2)  # a 16-bit field: a planted 2^23 saturates it
            if "big_syn_weight" in c:
                assert G.planted_at(fr, c["big_layer"]) == c["big_syn_weight"]
                assert d.q_step_index[4] == 0 and d.expgol_count[4] > 12
            else:
                assert top < d.ac_max_val_nn
            fr2, lat2 = G.make(**c)
            assert all(np.array_equal(fr.nn[k], fr2.nn[k]) for k in fr.nn) and bytes(fr.desc) == bytes(fr2.desc)
            assert all(np.array_equal(a, b) for a, b in zip(lat, lat2))
    a, b = G.make(**dict(LISTS["cin-grids4"][2], seed=1)), G.make(**dict(LISTS["cin-grids4"][2], seed=2))
    assert not np.array_equal(a[0].nn["syn_w"], b[0].nn["syn_w"]) and not np.array_equal(a[1][0], b[1][0])


def test_distinct_kernels_per_index():
    """What makes a wrong modulo show: no two upsampling or refine kernels of a frame are equal."""
    for fr, _ in made("ups-modulo") + made("ups-u10p7"):
        nets = G.decoded_nets(fr)
        for ks in (nets["ups_k"], nets["pre_k"]):
            assert len({tuple(k) for k in ks}) == len(ks)


@pytest.mark.parametrize("key", sorted(LISTS))
def test_generated_cases_show_a_picture(key):
    """The picture checks on the CPU: oracle stage wrappers on the generator's own networks.  (The
    GPU tests repeat them on the oracle's decode of the written stream.)"""
    for i, (c, (fr, lat)) in enumerate(zip(LISTS[key], made(key))):
        _, syn_out = oracle_tail(fr, lat)
        assert_picture(syn_out, c["layers"], f"{key}[{i}]", c.get("n_branches", 1))


GOLDEN = ROOT / "tests" / "golden" / "cool"


@pytest.mark.parametrize("name", ["D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool", "kodim01-lmbda-00001.cool"])
def test_oracle_stage_wrappers_reproduce_frame_decode(name, ccmi_lib):
    """cco_ups_forward / cco_syn_forward on a committed stream's latents and parsed networks give
    the syn_in / syn_out planes cco_decode_frame_mem returns; so does oracle_tail, from the
    integers alone, which pins cool_gen.decoded_nets' reading of the slots."""
    from ccmi import encode
    data = (GOLDEN / name).read_bytes()
    sizes, lat, syn_in, syn_out, _ = oracle_decode(data)
    fr = encode.parse(data)
    d = fr.desc
    nets = G.decoded_nets(fr)
    got_in = oracle_ups(lat, sizes, nets["ups"], d.ups_k, d.n_ups, d.pre_k, d.n_pre)
    assert np.array_equal(got_in, syn_in)
    assert np.array_equal(oracle_syn(syn_in, G.layers_of(d), nets["syn"]), syn_out)
    grids, p = [], 0
    for h, w in sizes:
        grids.append(lat[p: p + h * w] >> 8)
        p += h * w
    a, b = oracle_tail(fr, grids)
    assert np.array_equal(a, syn_in) and np.array_equal(b, syn_out)


# ---------------------------------------------------------------- GPU: streams against the oracle
def _formats(fr):
    """[(bitdepth, chroma, as_yuv)]: the stream's own format and one other."""
    return [(0, 0, True), (10, 420, True)] if fr.desc.frame_data_type == 1 else [(0, 0, False), (16, 0, False)]


@lru_cache(maxsize=None)
def written(key):
    import torch
    return [G.write(fr, lat, torch.device("cuda:0")) for fr, lat in made(key)]


def check_streams(key, gpu):
    import torch
    from ccmi import decode
    cases, frames, datas = LISTS[key], made(key), written(key)
    refs = []
    for i, (c, (fr, lat), data) in enumerate(zip(cases, frames, datas)):
        name = f"{key}[{i}]"
        sizes, olat, syn_in, syn_out, obytes = oracle_decode(data, _formats(fr))
        refs.append(obytes)
        assert_picture(syn_out, c["layers"], name, c.get("n_branches", 1))
        d = fr.desc
        # the stream carries the generator's integers, the planted weight among them
        _, ups, syn = decode.weights_i32(data)
        nets = G.decoded_nets(fr)
        assert np.array_equal(ups, nets["ups"]) and np.array_equal(syn, nets["syn"]), name
        if "big_syn_weight" in c:
            assert G.planted_at(fr, c["big_layer"]) == c["big_syn_weight"]
        # latents: GPU == oracle == written
        got = decode.decode_latents(data)
        assert decode.last_arm_flags() == [0], name
        p = 0
        for g, a in zip(got, lat):
            assert np.array_equal(g, a), name
            assert np.array_equal(olat[p: p + a.size], a.astype(np.int32) << 8), name
            p += a.size
        # the stage entry points (single-frame kernels) on the oracle's latents
        got_in = decode.ups_forward_i32(torch.from_numpy(olat).to(gpu), sizes, torch.from_numpy(ups).to(gpu), d.ups_k,
                                        d.n_ups, d.pre_k, d.n_pre)
        assert np.array_equal(got_in.cpu().numpy(), syn_in), name
        if d.n_branches == 1:
            got_out = decode.syn_forward_i32(torch.from_numpy(syn_in).to(gpu), G.layers_of(d), torch.from_numpy(syn).to(gpu))
            assert np.array_equal(got_out.cpu().numpy(), syn_out), name
    # the output bytes: the list in one call (streams of one frame type share the output format), and alone
    for yuv in (True, False):
        idx = [i for i, (fr, _) in enumerate(frames) if (fr.desc.frame_data_type == 1) == yuv]
        if not idx:
            continue
        for k, (bd, chroma, as_yuv) in enumerate(_formats(frames[idx[0]][0])):
            outs = decode.decode_batch([datas[i] for i in idx], bd, chroma, as_yuv)
            assert decode.last_arm_flags() == [0] * len(idx)
            for i, o in zip(idx, outs):
                assert o == refs[i][k], f"{key}[{i}] in the batch, format {bd}/{chroma}"
            for i in idx:
                o, = decode.decode_batch([datas[i]], bd, chroma, as_yuv)
                assert o == refs[i][k], f"{key}[{i}] alone, format {bd}/{chroma}"
    return refs


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(k for k in LISTS if not k.startswith("mixed")))
def test_generated_streams_decode_to_the_oracle(key, gpu, ccmi_lib):
    check_streams(key, gpu)


@pytest.mark.gpu
def test_arm_product_in_one_batch(gpu, ccmi_lib):
    """The 20 (d, nh) streams in ONE decode_batch, which makes one ARM launch per (d, nh) group;
    then with the narrow rgb frames beside them, so that the groups of a launch mix geometries."""
    from ccmi import decode
    frames, datas = made("arm-product"), written("arm-product")
    assert len(datas) == 20 and all(fr.desc.frame_data_type == 0 for fr, _ in frames)
    narrow = [d for d, (fr, _) in zip(written("arm-narrow"), made("arm-narrow")) if fr.desc.frame_data_type == 0]
    assert len(narrow) >= 4
    want = [oracle_decode(data, [(0, 0, False)])[4][0] for data in datas + narrow]
    for batch in (datas, datas + narrow, narrow + datas[::-1]):
        outs = decode.decode_batch(batch, 0, 0, False)
        assert decode.last_arm_flags() == [0] * len(batch)
        ref = want[:20] if batch is datas else want if batch[0] is datas[0] else want[20:] + want[:20][::-1]
        for i, (o, r) in enumerate(zip(outs, ref)):
            assert o == r, i


@pytest.mark.gpu
def test_mixed_architectures_share_a_call(gpu, ccmi_lib):
    """Architectures of one geometry in one decode_batch and one decode_batch_tensors call: each
    frame equals its stand-alone decode (check_streams: the oracle's bytes) and the tensors hold
    the same samples."""
    from ccmi import decode
    key = "mixed-groups"
    refs = check_streams(key, gpu)
    datas = written(key)
    h, w = LISTS[key][0]["H"], LISTS[key][0]["W"]
    outs = decode.decode_batch_tensors(datas)
    for i, (o, r) in enumerate(zip(outs, refs)):
        got = np.concatenate([o[k].cpu().numpy().reshape(-1) for k in "yuv"])
        assert got.dtype == np.uint8 and got.tobytes() == r[0], i
        assert o["y"].shape == (h, w)


# ---------------------------------------------------------------- GPU: stages, for what no stream carries
def _stage_params(rng, c_in, layers, draw=None):
    """Per layer weights, then biases: from draw(n), or weights of about 1.5 / sqrt(fan-in) and
    biases of up to a quarter of full scale."""
    parts, c = [], c_in
    for n_out, ks, _, _ in layers:
        a = int(1.5 * UNIT / np.sqrt(c * ks * ks))
        parts += [draw(n_out * c * ks * ks), draw(n_out)] if draw else \
            [rng.integers(-a, a + 1, n_out * c * ks * ks), rng.integers(-(1 << 22), (1 << 22) + 1, n_out)]
        c = n_out
    return np.concatenate(parts).astype(np.int32)


def _wild(rng):
    """int32 values at and near the type's ends, and over its whole range."""
    edge = np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1, (1 << 23), -(1 << 23) - 1, 1 << 30], dtype=np.int64)

    def draw(n):
        v = rng.integers(-(1 << 31), 1 << 31, n)
        pick = rng.random(n) < 0.3
        v[pick] = rng.choice(edge, int(pick.sum()))
        return v.astype(np.int32)
    return draw


# (name, c_in, H, W, layers, wild): the reference is the oracle's own loops (cco_syn_forward),
# which wrap as the int32 reference does (-fwrapv on both sides)
STAGE_SYN = [
    ("cin1", 1, 33, 65, fused(16, PRESET[:2]), False),                        # dec_syn_fused<1, 3>
    ("cin1_nsp0", 1, 29, 61, fused(5), False),
    ("hid600", 7, 33, 65, fused(600, PRESET[:2]), False),                     # hid * 12 > 3 * 2048: weights re-read
    ("hid513_cin8", 8, 31, 63, fused(513, PRESET), False),                    # the first width past the bound 512
    ("hid512_cin8", 8, 31, 63, fused(512, PRESET), False),                    # the last one within it
    ("wild_fused", 7, 33, 65, fused(16, PRESET), True),                       # every sum wraps
    ("wild_generic", 4, 21, 37, [(6, 1, 0, 1), (6, 3, 1, 1), (3, 5, 0, 0)], True),  # a residual layer keeps its width
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,c_in,h,w,layers,wild", STAGE_SYN, ids=[s[0] for s in STAGE_SYN])
def test_syn_stage_matches_the_oracle_loops(name, c_in, h, w, layers, wild, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    rng = np.random.default_rng(sum(map(ord, name)))
    draw = _wild(rng) if wild else None
    params = _stage_params(rng, c_in, layers, draw)
    x = (draw(c_in * h * w) if wild else rng.integers(-3 * UNIT, 3 * UNIT, c_in * h * w).astype(np.int32)).reshape(c_in, h, w)
    want = oracle_syn(x, layers, params)
    assert len(np.unique(want)) > 64
    got = decode.syn_forward_i32(torch.from_numpy(x).to(gpu), layers, torch.from_numpy(params).to(gpu))
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("ups_k,pre_k,n_grids,h,w", [(8, 7, 7, 33, 65), (6, 5, 3, 17, 65), (14, 15, 5, 9, 131)])
def test_ups_stage_wraps_as_the_oracle_loops(ups_k, pre_k, n_grids, h, w, gpu, ccmi_lib):
    """Latents and kernels over the whole int32 range: every product and sum wraps."""
    import torch
    from ccmi import decode
    rng = np.random.default_rng(ups_k * 100 + pre_k)
    draw = _wild(rng)
    sizes = G.grid_sizes(h, w, n_grids)
    n = n_grids - 1
    kernels = np.concatenate([G._mirror(draw((ups_k + 1) // 2), ups_k) for _ in range(n)] +
                             [G._mirror(draw((pre_k + 1) // 2), pre_k) for _ in range(n)]).astype(np.int32)
    lat = draw(sum(a * b for a, b in sizes))
    want = oracle_ups(lat, sizes, kernels, ups_k, n, pre_k, n)
    got = decode.ups_forward_i32(torch.from_numpy(lat).to(gpu), sizes, torch.from_numpy(kernels).to(gpu), ups_k, n, pre_k, n)
    assert np.array_equal(got.cpu().numpy(), want)
