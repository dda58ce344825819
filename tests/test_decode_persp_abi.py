"""The host side of CCMI_WARP_PROJECTIVE (0x800 or'ed into ccmi_warp.pad; matrix = [n][9]): which pad
values the plan takes, the checks of step 3a' in ccmi.h on both sides of each bound, and what the plan
of a matrix with the row 0 0 1 shares with its 6-entry call.  As tests/test_decode_warp_abi.py: no
compute, the plan calls make no GPU call, the latent handles are plan-only, and the run entry points
are only ever called with arguments the plan rejects.

The expected decisions come from tests/persp_ref.py (quantities / refusal / window), which restates
ccmi.h; the bounds are walked one float32 step at a time by bisection on one matrix entry.

The argument table's entry of a projective frame is 16 bytes longer than an affine one (nine floats for
six, rounded to 8), so the workspace of a 0 0 1 call equals the 6-entry call's up to that table growth,
rounded to 256 per call, and exactly for one frame; geometry, ccmi_roi_info and window are equal."""
import ctypes as C
import math

import numpy as np
import pytest

import persp_ref as PR
import test_decode_resample_abi as RA
import test_decode_warp_abi as WA
from test_decode_resample_abi import E_BF16, E_F16, FAKE, Geom, Handle, I, Info, P, Rect, Z, _args, _fields, _first, _fmt, \
    _header_only, _is_arg_error
from test_decode_warp_abi import IDENT, Warp, ccmi_frame

PERSP = 0x800
IDENT9 = (1, 0, 0, 0, 1, 0, 0, 0, 1)
PADS_OK = (0x800, 0x801, 0x900, 0x901, 0xB00, 0xB01)
PADS_BAD = (0x400, 0x401, 0xA00, 0xA01, 0xC00, 0x802, 0x1800, 0x1000, 0x880, -1, -0x800)


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    lib.ccmi_decode_batch_dev_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_decode_batch_dev_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_warp.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_flt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_latents_render_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_latents_render_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_flt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for name in ("ccmi_decode_batch_dev_fmt_plan", "ccmi_decode_batch_dev_warp_plan", "ccmi_decode_batch_dev_warp",
                 "ccmi_decode_batch_dev_col_plan", "ccmi_decode_batch_dev_flt_plan", "ccmi_decode_batch_dev_tone_plan",
                 "ccmi_latents_decode", "ccmi_latents_render_warp_plan", "ccmi_latents_render_col_plan",
                 "ccmi_latents_render_flt_plan", "ccmi_latents_render_tone_plan", "ccmi_decode_last_tail_groups"):
        getattr(lib, name).restype = C.c_int
    return lib


def _pwarp(mats, ow, oh, pad=PERSP, fill=(0.0, 0.0, 0.0)):
    """(ccmi_warp with [n][9] matrices, the array it points to)"""
    a = np.ascontiguousarray(np.asarray(mats, dtype=np.float32).reshape(-1, 9))
    w = Warp(out_w=ow, out_h=oh, pad=pad, matrix=a.ctypes.data)
    for c in range(3):
        w.fill[c] = fill[c]
    return w, a


def _rejected(lib, data, mats, ow, oh, frame, *words, pad=PERSP, fill=(0.0, 0.0, 0.0), chroma=444):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned"""
    w, keep = _pwarp(mats, ow, oh, pad, fill)
    rc, _, _, _, got = WA._plan(lib, data, _fmt(), w, chroma=chroma)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    rc = WA._run(lib, data, _fmt(), w, [1 << 30] * len(data), chroma=chroma)
    _is_arg_error(rc, frame, *words)


def _accepted(lib, data, mats, ow, oh, pad=PERSP, chroma=444):
    import ccmi
    w, keep = _pwarp(mats, ow, oh, pad)
    rc, geom, info, win, need = WA._plan(lib, data, _fmt(), w, chroma=chroma)
    assert rc == 0 and need > 0, (mats, ccmi.last_error())
    return geom, info, win, need


# ------------------------------------------------------------------ pad values
def test_pad_values(L, data):
    for pad in PADS_OK:
        _accepted(L, data[:2], [IDENT9] * 2, 8, 8, pad)
    for pad in PADS_BAD:
        _rejected(L, data[:2], [IDENT9] * 2, 8, 8, 0, "pad", str(pad), pad=pad)
    from ccmi import decode
    assert decode.WARP_PROJECTIVE == 0x800


def test_the_matrix_is_read_nine_entries_a_frame(L, data):
    """Frame 1's matrix starts at entry 9: a NaN there names frame 1, one at entry 6 frame 0."""
    mats = np.array([IDENT9] * 3, np.float32)
    for flat, frame in ((6, 0), (8, 0), (9, 1), (17, 1), (18, 2), (26, 2)):
        bad = mats.copy().reshape(-1)
        bad[flat] = np.nan
        _rejected(L, data, bad.reshape(3, 9), 8, 8, frame, "matrix entry %d" % (flat % 9), "finite")


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), -float("inf")))
def test_non_finite_matrix_entry_or_fill(L, data, bad):
    for k in range(9):
        m = list(IDENT9)
        m[k] = bad
        for pad in (0x800, 0xB01):
            _rejected(L, data, [IDENT9, m, IDENT9], 8, 8, 1, "matrix", "finite", pad=pad)
    fill = [0.0, bad, 0.0]
    _rejected(L, data, [IDENT9] * 3, 8, 8, 0, "fill", "finite", fill=fill)


def test_the_existing_checks_apply_unchanged(L, data):
    for ow, oh in ((0, 8), (8, 16385)):
        _rejected(L, data[:2], [IDENT9] * 2, ow, oh, 0, "output size", "16384")
    for ow, oh in ((16384, 1), (1, 16384)):
        geom, *_ = _accepted(L, data[:1], [IDENT9], ow, oh)
        assert (geom[0].width, geom[0].height, geom[0].elems) == (ow, oh, 3 * ow * oh)
    for h, w in ((63, 64), (64, 63), (21, 37)):
        odd = [_header_only(64, 64), _header_only(h, w)]
        _rejected(L, odd, [IDENT9] * 2, 8, 8, 1, "even", "444", chroma=0)
        _rejected(L, odd, [IDENT9] * 2, 8, 8, 1, "even", chroma=420)
        geom, *_ = _accepted(L, odd, [IDENT9] * 2, 8, 8, chroma=444)
        assert geom[1].chroma == 444


# ------------------------------------------------------------------ the bounds, each on both sides
def test_the_reach_bound_of_all_three_rows(L, data):
    """S_r <= 2^22: at the bound accepted, one float32 step above refused.  The last row is 0 0 2 for rows
    0 and 1, so that S_r / D' stays below the second bound."""
    top = 2.0 ** 22
    over = float(np.nextafter(np.float32(top), np.float32(np.inf)))
    for row in (0, 1, 2):
        def mat(a, b, c):
            m = [1, 0, 0, 0, 1, 0, 0, 0, 2.0]
            m[3 * row: 3 * row + 3] = [a, b, c]
            return m
        for m in (mat(0, 0, top), mat(top / 16, 0, 0), mat(0, top / 16, 0)):
            assert PR.refusal(m, 16, 16, 240, 416) is None
            _accepted(L, data[:2], [IDENT9, m], 16, 16)
        for m in (mat(0, 0, over), mat(over / 16, 0, 0), mat(1e30, 0, 0)):
            assert PR.refusal(m, 16, 16, 240, 416) == "2^22"
            _rejected(L, data[:2], [IDENT9, m], 16, 16, 1, "2^22", "row %d" % row)
    # negative entries count by magnitude in rows 0 and 1
    _accepted(L, data[:2], [IDENT9, [0, 0, -top, 0, 1, 0, 0, 0, 2]], 16, 16)
    _rejected(L, data[:2], [IDENT9, [0, 0, -over, 0, 1, 0, 0, 0, 2]], 16, 16, 1, "2^22")


def test_a_denominator_that_is_not_positive_at_one_corner_only(L, data):
    ow, oh = 8, 6
    for corner in range(4):
        sx, sy = (1 if corner & 1 else -1), (1 if corner & 2 else -1)
        # wn = -sx (cx - 4) - sy (cy - 3) + c: least at the corner (sx, sy), where it is c - 3.5 - 2.5
        def mat(c):
            return [1, 0, 0, 0, 1, 0, -sx, -sy, c + 4 * sx + 3 * sy]
        q = PR.quantities(mat(6.0), oh, ow, 240, 416)
        assert q["D"] == 0.0
        _rejected(L, data[:2], [IDENT9, mat(6.0)], ow, oh, 1, "denominator", "not positive")
        _rejected(L, data[:2], [IDENT9, mat(5.0)], ow, oh, 1, "denominator")
        _accepted(L, data[:2], [IDENT9, mat(6.5)], ow, oh)  # positive at all four: 0.5, and 7 to 12.5 elsewhere
    for m in ([1, 0, 0, 0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0, -1], [0] * 9, [-1, 0, 0, 0, -1, 0, 0, 0, -1]):
        _rejected(L, data[:2], [m, IDENT9], ow, oh, 0, "denominator")


RANK = {"denominator": 0, "2^22": 1, "too strong": 2, None: 3}
WORDS = {"denominator": ("denominator",), "2^22": ("2^22", "after the division"), "too strong": ("too strong for float32 positions",)}


def _first_with_rank(make, lo, hi, rank, oh, ow, H, W_):
    """The least float32 c in (lo, hi] whose matrix make(c) has at least this rank (the rank grows with c)."""
    a, b = np.float32(lo).view(np.int32).item(), np.float32(hi).view(np.int32).item()
    def r(bits):
        return RANK[PR.refusal(make(np.int32(bits).view(np.float32).item()), oh, ow, H, W_)]
    assert r(a) < rank <= r(b)
    while b - a > 1:
        mid = (a + b) // 2
        if r(mid) >= rank:
            b = mid
        else:
            a = mid
    return np.int32(a).view(np.float32).item(), np.int32(b).view(np.float32).item()


@pytest.mark.parametrize("which", (0, 1, 2))
def test_each_bound_one_float32_step_inside_and_outside(L, data, which):
    """A denominator that falls to c - 7.5 at the right edge of an 8-wide output: raising c one float32
    step at a time crosses D' > 0, then S_0 / D' <= 2^22 (row 0 reaches 2^13), then E <= 7/8, in that order;
    at each crossing the plan's decision changes between two adjacent float32 values of m22.  On the
    416 x 240 stream (which 0), the 1280 x 720 stream (1) and with the roles of the axes exchanged (2)."""
    import ccmi
    stream, (H, W_) = (data[0], (240, 416)) if which != 1 else (data[1], (720, 1280))
    ow, oh = (8, 5) if which != 2 else (5, 8)

    def make(c):
        if which != 2:
            return [0, 0, 2.0 ** 13, 0, 1, 0, -1, 0, c]
        return [1, 0, 0, 0, 0, 2.0 ** 13, 0, -1, c]
    seen = []
    for rank in (1, 2, 3):
        below, above = _first_with_rank(make, 7.5, 64.0, rank, oh, ow, H, W_)
        assert np.nextafter(np.float32(below), np.float32(np.inf)) == np.float32(above)
        for c in (below, above):
            why = PR.refusal(make(c), oh, ow, H, W_)
            seen.append(why)
            if why is None:
                _accepted(L, [stream], [make(c)], ow, oh)
            else:
                _rejected(L, [stream], [make(c)], ow, oh, 0, *WORDS[why])
    assert seen == ["denominator", "2^22", "2^22", "too strong", "too strong", None]


def test_the_position_error_bound_depends_on_the_frame(L, data):
    """E_r carries the frame's size: one matrix is accepted on the 416 x 240 frame and too strong for the
    1280 x 720 one."""
    ow = oh = 8
    def make(c):
        return [1, 0, 0, 0, 1, 0, -1, 0, c]
    below, above = _first_with_rank(make, 7.5, 64.0, 3, oh, ow, 240, 416)
    assert PR.refusal(make(above), oh, ow, 240, 416) is None
    assert PR.refusal(make(above), oh, ow, 720, 1280) == "too strong"
    _accepted(L, data[:1], [make(above)], ow, oh)
    _rejected(L, data[:2], [make(above)] * 2, ow, oh, 1, "too strong for float32 positions")


# ------------------------------------------------------------------ the row 0 0 1 against the 6-entry call
def test_a_0_0_1_matrix_plans_as_its_6_entry_call(L, data):
    import ccmi
    rng = np.random.default_rng(81)
    for i, stream in enumerate(data):
        H, W_, chroma = ccmi_frame(L, stream)
        for (oh, ow), n in (((224, 224), 40), ((17, 39), 1), ((1, 1), 2)):
            mats = WA._random_matrices(rng, n, H, W_, oh, ow)
            for flags in (0, 1, 0x100, 0x301):
                w6, keep6 = WA._warp(mats, ow, oh, flags, (0.1, 0.2, 0.3))
                rc, g6, i6, win6, need6 = WA._plan(L, [stream] * n, _fmt(E_BF16), w6)
                assert rc == 0, ccmi.last_error()
                w9, keep9 = _pwarp([PR.as9(m) for m in mats], ow, oh, flags | PERSP, (0.1, 0.2, 0.3))
                rc, g9, i9, win9, need9 = WA._plan(L, [stream] * n, _fmt(E_BF16), w9)
                assert rc == 0, ccmi.last_error()
                assert win9 == win6
                assert [_fields(a) for a in g9] == [_fields(b) for b in g6]
                for a, b in zip(i9, i6):
                    assert list(a.arm_rows) == list(b.arm_rows) and (a.windowed, a.n_grids) == (b.windowed, b.n_grids)
                grow = need9 - need6
                assert grow % 256 == 0 and 0 <= grow <= 256 * math.ceil(16 * n / 256), (need9, need6)
                if n == 1:
                    assert need9 == need6
                a, b = C.c_int(7), C.c_int(7)
                assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def test_windows_follow_the_rule_and_hold_every_tap(L, data):
    """200 seeded homographies per stream: window[] is persp_ref.window() -- the rule of ccmi.h recomputed
    here --, never empty, inside the frame, even at 420, and holds every in-frame tap of the float32
    contract, bilinear and bicubic."""
    import ccmi
    rng = np.random.default_rng(82)
    projective = 0
    for i, stream in enumerate(data):
        H, W_, chroma = ccmi_frame(L, stream)
        for oh, ow in ((224, 224), (17, 39), (1, 1), (8, 300)):
            n = 50
            mats = PR.accepted_homographies(rng, n, H, W_, oh, ow)
            projective += sum(bool(m[6] != 0 or m[7] != 0) for m in mats)
            for pad, reach in ((PERSP, 1), (PERSP | 0x101, 2)):
                w, keep = _pwarp(mats, ow, oh, pad, (0.1, 0.2, 0.3))
                rc, geom, info, win, need = WA._plan(L, [stream] * n, _fmt(E_F16), w)
                assert rc == 0, ccmi.last_error()
                for j, m in enumerate(mats):
                    x, y, ww, hh = win[j]
                    assert win[j] == PR.window(m, oh, ow, H, W_, even=chroma == 420, reach=reach), (i, j, m)
                    assert ww >= 1 and hh >= 1 and x >= 0 and y >= 0 and x + ww <= W_ and y + hh <= H
                    if chroma == 420:
                        assert (x | y | ww | hh) & 1 == 0
                    ty, tx = PR.taps_in_frame(m, oh, ow, H, W_, reach)
                    assert not ((tx < x) | (tx >= x + ww) | (ty < y) | (ty >= y + hh)).any(), (i, j, m)
                    assert (geom[j].width, geom[j].height, geom[j].elems) == (ow, oh, 3 * ow * oh)
                rc, _, finfo, fneed = WA._plan_fmt(L, [stream] * n, win, _fmt(E_F16))
                assert rc == 0, ccmi.last_error()
                for a, b in zip(info, finfo):
                    assert list(a.arm_rows) == list(b.arm_rows) and (a.windowed, a.n_grids) == (b.windowed, b.n_grids)
                grow = need - fneed
                assert grow % 256 == 0 and 0 <= grow <= 256 * math.ceil(48 * n / 256), (need, fneed)
    assert projective >= 400


def test_windows_of_explicit_homographies(L, data):
    """On the 416 x 240 stream at 444, 8 x 8 outputs.  wn = 1 + cx / 8 runs from 1.0625 to 1.9375: the
    quotient of xn = 100 wn + 16 (cx - 4) ... stated as numbers, and an output outside the frame."""
    d = [data[0]] * 3
    mats = [(2, 0, 100, 0, 2, 50, 0.125, 0, 1),      # xs = (2 cx + 100) / wn, ys = (2 cy + 50) / wn
            (1, 0, 5000, 0, 1, 20, 0, 0.125, 1),     # to the right of the frame
            (0, 0, 7, 0, 0, 9, 0.5, 0.5, 1)]         # constant numerators: towards the origin
    _, _, win, _ = _accepted(L, d, mats, 8, 8, PERSP | 1)
    assert win == [PR.window(m, 8, 8, 240, 416) for m in mats]
    # frame 0: xs from 101 / 1.0625 = 95.06 (cx 0.5) down to 115 / 1.9375 = 59.35 (cx 7.5): columns 57 .. 96;
    # ys from 51 / 1.9375 = 26.32 to 65 / 1.0625 = 61.18: rows 24 .. 62
    assert win[0] == (57, 24, 40, 39)
    assert win[1] == (415, 12, 1, 9)
    _, _, cwin, _ = _accepted(L, d, mats, 8, 8, PERSP | 0x101)
    assert cwin[0] == (56, 23, 42, 41) and cwin == [PR.window(m, 8, 8, 240, 416, reach=2) for m in mats]


# ------------------------------------------------------------------ every plan that carries a warp
def test_the_same_errors_from_the_col_flt_tone_and_latent_store_plans(L, data):
    import ccmi
    n = 3
    keep, sp, ln = _args(data)
    f = _fmt(E_F16)
    good = [IDENT9, (1, 0, 3, 0, 1, 2, 0.001, 0.002, 1), (0.5, 0, 9, 0, 0.5, 9, 0, 0, 2)]
    cases = ((good, PERSP, None, ()),
             (good, 0xB01, None, ()),
             (good, 0xA00, 0, ("pad",)),
             (good, 0x400, 0, ("pad",)),
             ([good[0], good[1], (1, 0, 0, 0, 1, 0, 0, 0, float("nan"))], PERSP, 2, ("matrix entry 8", "finite")),
             ([good[0], (1, 0, 0, 0, 1, 0, -1, 0, 4), good[2]], PERSP, 1, ("denominator",)),
             ([good[0], (1, 0, 0, 0, 1, 0, 0, 0, 2.0 ** 23), good[2]], PERSP, 1, ("2^22", "row 2")),
             ([(1, 0, 0, 0, 1, 0, -1, 0, 7.5005), good[1], good[2]], PERSP, 0, ("too strong for float32 positions",)))
    sizes = [ccmi_frame(L, s)[:2] for s in data]
    with Handle(L, data) as H:
        for mats, pad, frame, words in cases:
            w, keepw = _pwarp(mats, 8, 8, pad)
            if frame is not None and "pad" not in words:
                assert PR.refusal(mats[frame], 8, 8, *sizes[frame]) in " ".join(words)
            outs = []
            for run in range(8):
                geom, win, need = (Geom * n)(), (Rect * n)(), C.c_size_t(0)
                r, fw, g, wn, nd = None, C.byref(f), geom, win, C.byref(need)
                rc = (lambda: L.ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, 444, fw, C.byref(w), g, None, wn, nd),
                      lambda: L.ccmi_decode_batch_dev_col_plan(sp, ln, n, r, 0, 444, fw, None, C.byref(w), None, g, None, wn, nd),
                      lambda: L.ccmi_decode_batch_dev_flt_plan(sp, ln, n, r, 0, 444, fw, None, C.byref(w), None, None, g, None, wn, nd),
                      lambda: L.ccmi_decode_batch_dev_tone_plan(sp, ln, n, r, 0, 444, fw, None, C.byref(w), None, None, None, g, None, wn, nd),
                      lambda: L.ccmi_latents_render_warp_plan(H.h, None, n, 0, 444, fw, C.byref(w), g, None, wn, nd),
                      lambda: L.ccmi_latents_render_col_plan(H.h, None, n, r, 0, 444, fw, None, C.byref(w), None, g, None, wn, nd),
                      lambda: L.ccmi_latents_render_flt_plan(H.h, None, n, r, 0, 444, fw, None, C.byref(w), None, None, g, None, wn, nd),
                      lambda: L.ccmi_latents_render_tone_plan(H.h, None, n, r, 0, 444, fw, None, C.byref(w), None, None, None, g, None, wn, nd),
                      )[run]()
                if frame is None:
                    assert rc == 0, (run, ccmi.last_error())
                    outs.append(([(x.x, x.y, x.w, x.h) for x in win], [_fields(x) for x in geom]))
                else:
                    _is_arg_error(rc, frame, *words)
                    assert need.value == 0
            if frame is None:
                assert all(o == outs[0] for o in outs)
                reach = 2 if pad & 0x100 else 1
                assert outs[0][0] == [PR.window(m, 8, 8, hh, ww, reach=reach) for m, (hh, ww) in
                                      zip(mats, sizes)]


# ------------------------------------------------------------------ the Python keywords (no GPU call)
def test_python_keyword_shapes_and_exclusions():
    from ccmi import decode
    w, a = decode._warp(None, 2, (8, 6), None, "edge", 0.5, decode._interp("bicubic", True), np.eye(3))
    assert (w.pad, w.out_w, w.out_h) == (0xB01, 6, 8) and a.shape == (2, 3, 3) and a.dtype == np.float32
    w, a = decode._warp(None, 2, (8, 6), None, "fill", 0.0, perspective=[np.eye(3).tolist()] * 2)
    assert w.pad == 0x800 and a.flags["C_CONTIGUOUS"]
    assert decode._warp(None, 2, (8, 6), None, "fill", 0.0) == (None, None)
    w, a = decode._warp(np.eye(3)[:2], 2, (8, 6), None, "fill", 0.0)
    assert w.pad == 0 and a.shape == (2, 2, 3)  # affine= is as it was
    with pytest.raises(ValueError, match="excludes affine"):
        decode._warp(np.eye(3)[:2], 2, (8, 6), None, "fill", 0.0, perspective=np.eye(3))
    with pytest.raises(ValueError, match="perspective needs size"):
        decode._warp(None, 2, None, None, "fill", 0.0, perspective=np.eye(3))
    with pytest.raises(ValueError, match="perspective excludes roi"):
        decode._warp(None, 2, (8, 6), [(0, 0, 4, 4)] * 2, "fill", 0.0, perspective=np.eye(3))
    for bad in (np.eye(3)[:2], np.zeros((3, 3, 3)), np.zeros(9)):
        with pytest.raises(ValueError, match=r"perspective takes \[2, 3, 3\]"):
            decode._warp(None, 2, (8, 6), None, "fill", 0.0, perspective=bad)
    import inspect
    for fn in (decode.decode_batch_model, decode.LatentStore.render_model, decode.LatentStore.render_model_workspace_bytes,
               decode.LatentStore.warp_plan):
        assert list(inspect.signature(fn).parameters)[-1] == "perspective"
