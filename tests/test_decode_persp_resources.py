"""Register, scratch and LDS use of the projective warp kernels, read from the gfx950 code-object
metadata of the built libccmi.so in the form of tests/test_decode_cubic_resources.py (no GPU needed):
the plain, colour and statistics forms of Warp<false, true> and Warp<true, true>, each per frame and of a
tail group -- 28 kernels.  Every one must be there exactly once, use no scratch, spill nothing and use
no LDS; 128 VGPRs is the hard bound (4 waves per SIMD) and is asserted.  Each kernel's count is printed
beside its affine counterpart's (Warp<false, false> / Warp<true, false>, which must be there too), with
the waves per SIMD both reach.  VGPRs as built, projective (affine), per frame / tail group:
    dec_fmt_stat<Warp<false, .>>           48 / 48   (47 / 47)
    dec_fmt<Warp<false, .>, float>         63 / 63   (63 / 63)      dec_fmt_col 64 / 64   (61 / 65)
    dec_fmt<Warp<false, .>, F16|Bf16>      56 / 56   (55 / 55)      dec_fmt_col 57 / 57   (57 / 57)
    dec_fmt_stat<Warp<true, .>>            72 / 75   (64 / 64)
    dec_fmt<Warp<true, .>, float>          83 / 90   (83 / 90)      dec_fmt_col 91 / 91   (91 / 91)
    dec_fmt<Warp<true, .>, F16|Bf16>       80 / 83   (72 / 82)      dec_fmt_col 78 / 84   (80 / 83)
The bilinear kernels all keep 8 waves.  An occupancy step below the affine counterpart: the cubic
statistics pass, both forms (7 and 6 waves for 8: the affine one asks the compiler for 8 waves, and with
the division's temporaries that request spills two registers, so the projective form is left to the
allocator) and the per-frame dec_fmt<Warp<true, true>, F16|Bf16> (6 waves for 7).
"""
from kernel_meta import LIB, TYPES, check_fmt_kernel, fmt_kernel, metadata, waves

MAX_VGPRS = 128  # the hard bound
PAIRS = (("pwarp", "warp"), ("pwcubic", "wcubic"))


def test_projective_kernels_use_no_scratch_no_lds_and_fit_the_registers(tmp_path):
    meta = metadata(LIB, tmp_path)
    wanted = [("stat", None)] + [(form, t) for form in ("plain", "col") for t in TYPES]
    lines, lower = [], []
    for new, old in PAIRS:
        for form, t in wanted:
            for table in (False, True):
                d, v = fmt_kernel(meta, new, form, t, table)
                _, a = fmt_kernel(meta, old, form, t, table)
                check_fmt_kernel(d, v, MAX_VGPRS, lines)
                lines[-1] += " (affine %3d VGPRs, %d waves)" % (a["vgpr_count"], waves(a["vgpr_count"]))
                if waves(v["vgpr_count"]) < waves(a["vgpr_count"]):
                    lower.append(lines[-1])
    assert len(lines) == 28
    print("\n".join(lines))
    print("an occupancy step below the affine counterpart: %s" % (lower or "none"))
