"""Register, scratch and LDS use of the projective warp kernels, read from the gfx950 code-object
metadata of the built libccmi.so in the form of tests/test_decode_cubic_resources.py (no GPU needed):
dec_pwarp<T>, dec_pwcubic<T>, their _col and _stat forms, each per frame and _batch -- 28 kernels.
Every one must be there exactly once, use no scratch, spill nothing and use no LDS; 128 VGPRs is the
hard bound (4 waves per SIMD) and is asserted.  Each kernel's count is printed beside its affine
counterpart's (dec_warp / dec_wcubic, which must be there too), with the waves per SIMD both reach.
VGPRs as built, projective (affine), per frame / _batch:
    dec_pwarp_stat                 48 / 48   (47 / 47)
    dec_pwarp<float>               63 / 63   (63 / 63)      _col 64 / 64   (61 / 65)
    dec_pwarp<F16|Bf16>            56 / 56   (55 / 55)      _col 57 / 57   (57 / 57)
    dec_pwcubic_stat               72 / 75   (64 / 64)
    dec_pwcubic<float>             83 / 90   (83 / 90)      _col 91 / 91   (91 / 91)
    dec_pwcubic<F16|Bf16>          80 / 83   (72 / 82)      _col 78 / 84   (80 / 83)
The bilinear kernels all keep 8 waves.  An occupancy step below the affine counterpart: dec_pwcubic_stat
and its _batch (7 and 6 waves for 8: dec_wcubic_stat asks the compiler for 8 waves, and with the
division's temporaries that request spills two registers, so the projective form is left to the allocator)
and the per-frame dec_pwcubic<F16|Bf16> (6 waves for 7).
"""
import re

from kernel_meta import LIB
from test_decode_cubic_resources import KEYS, MAX_VGPRS, TYPES, _metadata

PLAIN = ("%s_stat(", "%s_stat_batch(")
TYPED = ("%s<", "%s_batch<", "%s_col<", "%s_col_batch<")
PAIRS = (("dec_pwarp", "dec_warp"), ("dec_pwcubic", "dec_wcubic"))


def _waves(vgprs):
    """waves per SIMD of a wave64 kernel on gfx950: 512 VGPRs a lane, granules of 8, at most 8 waves"""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def _one(meta, form, t):
    hits = [(d, v) for d, v in meta.items() if "::" + form in d and
            (t is None or re.search(r"<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d))]
    assert len(hits) == 1, (form, t, [d for d, _ in hits])
    return hits[0]


def test_projective_kernels_use_no_scratch_no_lds_and_fit_the_registers(tmp_path):
    meta = _metadata(LIB, tmp_path)
    wanted = [(form, None) for form in PLAIN] + [(form, t) for form in TYPED for t in TYPES]
    lines, lower, count = [], [], 0
    for new, old in PAIRS:
        for form, t in wanted:
            d, v = _one(meta, form % new, t)
            _, a = _one(meta, form % old, t)
            count += 1
            line = "%-28s %-6s %3d VGPRs, %d waves (affine %3d, %d waves)" % (
                form % new, t or "", v["vgpr_count"], _waves(v["vgpr_count"]), a["vgpr_count"], _waves(a["vgpr_count"]))
            lines.append(line)
            for key in KEYS.split("|"):
                assert key in v or key.endswith("spill_count"), line
            assert v["private_segment_fixed_size"] == 0, line
            assert v.get("vgpr_spill_count", 0) == 0, line
            assert v.get("sgpr_spill_count", 0) == 0, line
            assert v["group_segment_fixed_size"] == 0, line
            assert v["vgpr_count"] <= MAX_VGPRS, line
            if _waves(v["vgpr_count"]) < _waves(a["vgpr_count"]):
                lower.append(line)
    assert count == 28
    print("\n".join(lines))
    print("an occupancy step below the affine counterpart: %s" % (lower or "none"))
