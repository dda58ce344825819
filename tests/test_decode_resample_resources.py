"""Register / scratch use of the resampling output kernels (dec_resize_h<false>,
dec_resize_h_batch<false>, dec_fmt<Resize<false>, T, false | true>), read from the gfx950
code-object metadata of the built libccmi.so in the form of tests/test_decode_fmt_resources.py (no
GPU needed).  The vertical stage keeps 4 pixels x 3 channels of accumulators per thread in
registers; no kernel may use scratch or spill."""
from kernel_meta import LIB, TYPES, check_fmt_kernel, fmt_kernel, metadata

MAX_VGPRS = 64  # 8 waves per SIMD


def test_resampling_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for table in (False, True):
        check_fmt_kernel(*fmt_kernel(meta, "resize", "h", None, table), MAX_VGPRS, lines)
        for t in TYPES:
            check_fmt_kernel(*fmt_kernel(meta, "resize", "plain", t, table), MAX_VGPRS, lines)
    assert len(lines) == 8
    print("\n".join(lines))
