"""Register / scratch use of the formatted-output kernels (dec_fmt<Plain, T, false>, the per-frame
cropping form, and dec_fmt<Plain, T, true>, the tail groups' form), read from the gfx950
code-object metadata of the built libccmi.so as tests/test_kernel_resources.py does (no GPU
needed).  The stage keeps 4 pixels x 3 channels per thread in registers and must use no
scratch and spill nothing.

As built: 35 VGPRs for the F16 and Bf16 instantiations of the two forms, 39 for the two float
ones; the planar float32 output kernel it stands in for has 29."""
from kernel_meta import LIB, TYPES, check_fmt_kernel, fmt_kernel, metadata

MAX_VGPRS = 64  # 8 waves per SIMD


def test_formatted_output_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for table in (False, True):
        for t in TYPES:
            check_fmt_kernel(*fmt_kernel(meta, "plain", "plain", t, table), MAX_VGPRS, lines)
    assert len(lines) == 6
    print("\n".join(lines))
