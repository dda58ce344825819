"""Register / scratch use of the formatted-output kernels (dec_output_fmt<T>, the per-frame
cropping form, and dec_output_fmt_batch<T>, the tail groups' form), read from the gfx950
code-object metadata of the built libccmi.so as tests/test_kernel_resources.py does (no GPU
needed).  The stage keeps 4 pixels x 3 channels per thread in registers and must use no
scratch and spill nothing.

As built: 35 VGPRs for the F16 and Bf16 instantiations of the two forms, 39 for the two float
ones; the planar float32 output kernel it stands in for has 29."""
import re

from kernel_meta import LIB, metadata

FORMS = ("dec_output_fmt<", "dec_output_fmt_batch<")
TYPES = ("float", "F16", "Bf16")
MAX_VGPRS = 64  # 8 waves per SIMD


def test_formatted_output_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for form in FORMS:
        for t in TYPES:
            hits = [(d, v) for d, v in meta.items() if form in d and re.search(r"<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d)]
            assert len(hits) == 1, (form, t, [d for d, _ in hits])
            d, v = hits[0]
            lines.append(f"{d[:110]}: {v}")
            assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
            assert v["private_segment_fixed_size"] == 0, lines[-1]
            assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
            assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
            assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
    print("\n".join(lines))
