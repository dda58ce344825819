"""Register / scratch use of the latent-file kernels (dec_lat_file_gather, dec_lat_file_sum,
dec_lat_seg_verify), read from the gfx950 code-object metadata of the built libccmi.so in the
form of tests/test_latent_seg_resources.py (no GPU needed).  They are memory-bound: no kernel may
use scratch or spill, and each fits 8 waves per SIMD."""
from kernel_meta import LIB, metadata

NEW = ("dec_lat_file_gather(", "dec_lat_file_sum(", "dec_lat_seg_verify(")
MAX_VGPRS = 64  # 8 waves per SIMD


def test_latent_file_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for form in NEW:
        hits = [(d, v) for d, v in meta.items() if form in d]
        assert len(hits) == 1, (form, [d for d, _ in hits])
        d, v = hits[0]
        line = f"{d[:110]}: {v}"
        assert "vgpr_count" in v and "private_segment_fixed_size" in v, line
        assert v["private_segment_fixed_size"] == 0, line
        assert v.get("vgpr_spill_count", 0) == 0, line
        assert v.get("sgpr_spill_count", 0) == 0, line
        assert v["vgpr_count"] <= MAX_VGPRS, line
        lines.append(line)
    print("\n".join(lines))
