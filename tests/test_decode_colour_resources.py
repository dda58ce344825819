"""Register / scratch use of the colour forms of the output kernels (dec_fmt_col<G, T, false | true>
for G = Plain, Resize<false> and Warp<false, false>, and the six statistics kernels dec_fmt_stat<G,
false | true>), read from the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_warp_resources.py (no GPU needed).

The op table is read with scalar loads and the frame's mean is kept in a scalar register, so the
colour stage adds no per-thread state beyond the pixel it works on; no kernel may use scratch, spill
or take LDS.  Bounds: 64 VGPRs, which keep 8 waves per SIMD, for everything but the float32
instantiations of the warp's colour form, whose 12 float32 outputs and 12 tap values are live next to
the op loop: 72 VGPRs, 7 waves per SIMD, one fewer than the plain warp (as built: 61 per frame and 65
of a tail group; the fp16 / bf16 instantiations 57)."""
from kernel_meta import LIB, TYPES, check_fmt_kernel, fmt_kernel, metadata

GEOMETRIES = ("plain", "resize", "warp")
MAX_VGPRS = 64       # 8 waves per SIMD
MAX_VGPRS_WARP_F32 = 72  # 7 waves per SIMD


def test_colour_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for g in GEOMETRIES:
        for table in (False, True):
            for t in TYPES:
                bound = MAX_VGPRS_WARP_F32 if g == "warp" and t == "float" else MAX_VGPRS
                check_fmt_kernel(*fmt_kernel(meta, g, "col", t, table), bound, lines)
    assert len(lines) == 18
    for g in GEOMETRIES:
        for table in (False, True):
            check_fmt_kernel(*fmt_kernel(meta, g, "stat", None, table), MAX_VGPRS, lines)
    assert len(lines) == 24
    print("\n".join(lines))
