"""Register / scratch / LDS use of the mix kernels (dec_mix_batch<T>; T = float, F16, Bf16), read from the
gfx950 code-object metadata of the built libccmi.so in the form of tests/test_decode_filter_resources.py
(no GPU needed).

The kernel is a stream: the frame's entry and its partner's come in by scalar loads, a thread keeps one
group of 4 pixels x 3 channels of the frame and, while it blends, of the partner, and the draws of a noise
rectangle are made one element at a time.  No kernel may use scratch or spill, none has static LDS (the
design uses none), and 64 VGPRs keep 8 waves per SIMD as far as registers go (measured: 58 VGPRs for float,
54 for F16 and Bf16; 0 bytes of LDS and of scratch for all three)."""
import re

from kernel_meta import LIB, TYPES, metadata

MAX_VGPRS = 64  # 8 waves per SIMD


def test_mix_kernels_use_no_scratch_no_lds_and_64_vgprs(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for t in TYPES:
        hits = [(d, v) for d, v in meta.items()
                if re.search(r"dec_mix_batch<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d)]
        assert len(hits) == 1, (t, [d for d, _ in hits])
        d, v = hits[0]
        lines.append(f"{d[:100]}: {v}")
        assert "vgpr_count" in v and "private_segment_fixed_size" in v and "group_segment_fixed_size" in v, lines[-1]
        assert v["private_segment_fixed_size"] == 0, lines[-1]
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, lines[-1]
        assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
        assert v["group_segment_fixed_size"] == 0, lines[-1]
    print("\n".join(lines))
