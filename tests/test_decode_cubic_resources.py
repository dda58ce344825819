"""Register, scratch and LDS use of the bicubic output kernels, read from the gfx950 code-object
metadata of the built libccmi.so in the form of tests/test_decode_resample_resources.py (no GPU
needed): the horizontal pass dec_resize_h<true> and the plain, colour and statistics forms of
Resize<true> and Warp<true, false>, each per frame and of a tail group -- 30 kernels.  Every one must
be there exactly once, use no scratch, spill nothing and use no LDS.  128 VGPRs is the hard bound (4
waves per SIMD) and is asserted; 64 (8 waves) is the aim: the resize kernels and the warp's statistics
pass meet it (they ask the compiler for 8 waves, which it grants without a spill), the typed warp
kernels do not (at 64 they spill 13 to 60 registers, so they are left to the allocator: 5 to 7 waves)
and are printed.  VGPRs as built (per frame / tail group):
    dec_resize_h<true>                     36 / 36
    dec_fmt<Resize<true>, float>           58 / 58   <F16|Bf16> 60 / 60   dec_fmt_col 60 / 60   dec_fmt_stat 60 / 60
    dec_fmt_stat<Warp<true, false>>        64 / 64
    dec_fmt<Warp<true, false>, float>      83 / 90   dec_fmt_col 91 / 91
    dec_fmt<Warp<true, false>, F16|Bf16>   72 / 82   dec_fmt_col 80 / 83"""
from kernel_meta import LIB, TYPES, check_fmt_kernel, fmt_kernel, metadata

MAX_VGPRS = 128  # the hard bound
AIM_VGPRS = 64   # 8 waves per SIMD


def test_cubic_kernels_use_no_scratch_no_lds_and_fit_the_registers(tmp_path):
    meta = metadata(LIB, tmp_path)
    wanted = [("cubic", "h", None), ("cubic", "stat", None), ("wcubic", "stat", None)]
    wanted += [(g, form, t) for g in ("cubic", "wcubic") for form in ("plain", "col") for t in TYPES]
    lines, over = [], []
    for g, form, t in wanted:
        for table in (False, True):
            d, v = fmt_kernel(meta, g, form, t, table)
            check_fmt_kernel(d, v, MAX_VGPRS, lines)
            if v["vgpr_count"] > AIM_VGPRS:
                over.append(lines[-1])
    assert len(lines) == 30
    print("\n".join(lines))
    print("above %d VGPRs: %s" % (AIM_VGPRS, over or "none"))
