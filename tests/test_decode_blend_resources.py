"""Register / scratch / LDS use of the blend kernels (dec_blend_batch<T>; T = float, F16, Bf16), read from
the gfx950 code-object metadata of the built libccmi.so in the form of tests/test_decode_mix_resources.py
(no GPU needed).

The kernel is dec_mix_batch with a uniform loop over a frame's terms: the entry, its blend entry and the
sources' entries come in by scalar loads, a thread keeps one group of 4 pixels x 3 channels of the frame's
sum and, while it mixes, of the partner's, and the terms are summed a channel at a time (4 loads of a term in flight).  No kernel may
use scratch or spill, none has static LDS, and 64 VGPRs keep 8 waves per SIMD as far as registers go
(measured: 64 VGPRs for float, 57 for F16 and Bf16, with 8 waves per SIMD asked of the compiler; 0 bytes of
LDS and of scratch for all three)."""
import re

from kernel_meta import LIB, TYPES, metadata

MAX_VGPRS = 64  # 8 waves per SIMD


def test_blend_kernels_use_no_scratch_no_lds_and_64_vgprs(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for t in TYPES:
        hits = [(d, v) for d, v in meta.items()
                if re.search(r"dec_blend_batch<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d)]
        assert len(hits) == 1, (t, [d for d, _ in hits])
        d, v = hits[0]
        lines.append(f"{d[:100]}: {v}")
        assert "vgpr_count" in v and "private_segment_fixed_size" in v and "group_segment_fixed_size" in v, lines[-1]
        assert v["private_segment_fixed_size"] == 0, lines[-1]
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, lines[-1]
        assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
        assert v["group_segment_fixed_size"] == 0, lines[-1]
    print("\n".join(lines))
