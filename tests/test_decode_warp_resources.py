"""Register / scratch use of the warping output kernels (dec_fmt<Warp<false, false>, T, false | true>),
read from the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_resample_resources.py (no GPU needed).  A thread works through its 4 pixels one
at a time, so 12 tap values are live and not 48; no kernel may use scratch, spill or take LDS, and 64
VGPRs keep 8 waves per SIMD for a stage that is bound by its gathers."""
from kernel_meta import LIB, TYPES, check_fmt_kernel, fmt_kernel, metadata

MAX_VGPRS = 64  # 8 waves per SIMD


def test_warping_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for table in (False, True):
        for t in TYPES:
            check_fmt_kernel(*fmt_kernel(meta, "warp", "plain", t, table), MAX_VGPRS, lines)
    assert len(lines) == 6
    print("\n".join(lines))
