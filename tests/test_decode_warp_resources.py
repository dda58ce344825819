"""Register / scratch use of the warping output kernels (dec_warp<T>, dec_warp_batch<T>), read from
the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_resample_resources.py (no GPU needed).  A thread works through its 4 pixels one
at a time, so 12 tap values are live and not 48; no kernel may use scratch or spill, and 64 VGPRs
keep 8 waves per SIMD for a stage that is bound by its gathers."""
import re

from kernel_meta import LIB, metadata

TYPED = ("dec_warp<", "dec_warp_batch<")
TYPES = ("float", "F16", "Bf16")
MAX_VGPRS = 64  # 8 waves per SIMD


def test_warping_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for form in TYPED:
        for t in TYPES:
            hits = [(d, v) for d, v in meta.items() if form in d and
                    re.search(r"<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d)]
            assert len(hits) == 1, (form, t, [d for d, _ in hits])
            d, v = hits[0]
            lines.append(f"{d[:110]}: {v}")
            assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
            assert v["private_segment_fixed_size"] == 0, lines[-1]
            assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
            assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
            assert v.get("group_segment_fixed_size", 0) == 0, lines[-1]  # no LDS
            assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
    print("\n".join(lines))
