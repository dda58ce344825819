"""Register / scratch use of the colour forms of the output kernels (dec_output_fmt_col<T>,
dec_resample_v_col<T>, dec_warp_col<T>, their _batch forms and the six statistics kernels), read
from the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_warp_resources.py (no GPU needed).

The op table is read with scalar loads and the frame's mean is kept in a scalar register, so the
colour stage adds no per-thread state beyond the pixel it works on; no kernel may use scratch, spill
or take LDS.  Bounds: 64 VGPRs, which keep 8 waves per SIMD, for everything but the float32
instantiations of the warp's colour form, whose 12 float32 outputs and 12 tap values are live next to
the op loop: 72 VGPRs, 7 waves per SIMD, one fewer than the plain warp (measured: 61 and 65; the
fp16 / bf16 instantiations 57)."""
import re

from kernel_meta import LIB, metadata

TYPED = ("dec_output_fmt_col<", "dec_output_fmt_col_batch<", "dec_resample_v_col<", "dec_resample_v_col_batch<",
         "dec_warp_col<", "dec_warp_col_batch<")
TYPES = ("float", "F16", "Bf16")
STATS = ("dec_output_fmt_stat(", "dec_output_fmt_stat_batch(", "dec_resample_v_stat(", "dec_resample_v_stat_batch(",
         "dec_warp_stat(", "dec_warp_stat_batch(")
MAX_VGPRS = 64       # 8 waves per SIMD
MAX_VGPRS_WARP_F32 = 72  # 7 waves per SIMD


def _check(d, v, bound, lines):
    lines.append(f"{d[:110]}: {v}")
    assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
    assert v["private_segment_fixed_size"] == 0, lines[-1]
    assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
    assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
    assert v.get("group_segment_fixed_size", 0) == 0, lines[-1]  # no LDS
    assert v["vgpr_count"] <= bound, lines[-1]


def test_colour_kernels_use_no_scratch(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for form in TYPED:
        for t in TYPES:
            hits = [(d, v) for d, v in meta.items() if form in d and
                    re.search(r"%s(\w+::)*(\(anonymous namespace\)::)?%s>" % (re.escape(form), t), d)]
            assert len(hits) == 1, (form, t, [d for d, _ in hits])
            bound = MAX_VGPRS_WARP_F32 if form.startswith("dec_warp") and t == "float" else MAX_VGPRS
            _check(*hits[0], bound, lines)
    for form in STATS:
        hits = [(d, v) for d, v in meta.items() if form in d]
        assert len(hits) == 1, (form, [d for d, _ in hits])
        _check(*hits[0], MAX_VGPRS, lines)
    print("\n".join(lines))
