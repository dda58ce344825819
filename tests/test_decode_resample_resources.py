"""Register / scratch use of the resampling output kernels (dec_resample_h, dec_resample_h_batch,
dec_resample_v<T>, dec_resample_v_batch<T>), read from the gfx950 code-object metadata of the
built libccmi.so in the form of tests/test_decode_fmt_resources.py (no GPU needed).  The vertical
stage keeps 4 pixels x 3 channels of accumulators per thread in registers; no kernel may use
scratch or spill."""
import re

from kernel_meta import LIB, metadata

PLAIN = ("dec_resample_h(", "dec_resample_h_batch(")
TYPED = ("dec_resample_v<", "dec_resample_v_batch<")
TYPES = ("float", "F16", "Bf16")
MAX_VGPRS = 64  # 8 waves per SIMD


def test_resampling_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    wanted = [(form, None) for form in PLAIN] + [(form, t) for form in TYPED for t in TYPES]
    lines = []
    for form, t in wanted:
        hits = [(d, v) for d, v in meta.items() if form in d and
                (t is None or re.search(r"<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d))]
        assert len(hits) == 1, (form, t, [d for d, _ in hits])
        d, v = hits[0]
        lines.append(f"{d[:110]}: {v}")
        assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
        assert v["private_segment_fixed_size"] == 0, lines[-1]
        assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
        assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
        assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
    print("\n".join(lines))
