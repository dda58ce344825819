"""Register / scratch use of the segmented latent store's kernels (dec_lat_seg_width,
dec_lat_seg_scan, dec_lat_seg_pack, dec_lat_unpack_seg), read from the gfx950 code-object
metadata of the built libccmi.so in the form of tests/test_decode_resample_resources.py (no GPU
needed).  They are memory-bound copies: no kernel may use scratch or spill, and each fits 8
waves per SIMD.  The typed pack / unpack kernels of the other storage forms are still there."""
import re

from kernel_meta import LIB, metadata

NEW = ("dec_lat_seg_width(", "dec_lat_seg_scan(", "dec_lat_seg_pack(", "dec_lat_unpack_seg(")
TYPED = ("dec_lat_pack<", "dec_lat_unpack<")
TYPES = ("signed char", "short", "int")
MAX_VGPRS = 64  # 8 waves per SIMD


def _lean(d, v):
    line = f"{d[:110]}: {v}"
    assert "vgpr_count" in v and "private_segment_fixed_size" in v, line
    assert v["private_segment_fixed_size"] == 0, line
    assert v.get("vgpr_spill_count", 0) == 0, line
    assert v.get("sgpr_spill_count", 0) == 0, line
    assert v["vgpr_count"] <= MAX_VGPRS, line
    return line


def test_segmented_store_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for form in NEW:
        hits = [(d, v) for d, v in meta.items() if form in d]
        assert len(hits) == 1, (form, [d for d, _ in hits])
        lines.append(_lean(*hits[0]))
    print("\n".join(lines))


def test_typed_pack_and_unpack_are_still_there(tmp_path):
    meta = metadata(LIB, tmp_path)
    for form in TYPED:
        for t in TYPES:
            hits = [d for d in meta if form in d and re.search(r"<%s>" % t, d)]
            assert len(hits) == 1, (form, t, hits)
