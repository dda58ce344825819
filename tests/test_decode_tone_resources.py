"""Register / scratch / LDS use of the tone kernels (dec_tone_stat, dec_tone_apply, dec_tone_sharp and their
_batch forms), read from the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_filter_resources.py (no GPU needed).

The op list, the segment and the terminator are scalars (uniform per block), a thread holds one pixel's
three channels at a time: no kernel may use scratch or spill, 128 VGPRs keep four waves per SIMD, and the
static LDS is the figure DESIGN.md states: the statistics kernel's 3 x 256 histogram (3,072 bytes), the
apply kernel's three byte LUTs with the scan's wave totals and steps (768 + 48 + 12 = 828 bytes), the
sharpness kernel's 34 x 34 tile of three channels (13,872 bytes)."""
import pytest

from kernel_meta import LIB, metadata
from test_decode_filter_resources import _lds

MAX_VGPRS = 128  # four waves per SIMD
LDS = {"dec_tone_stat": 3 * 256 * 4, "dec_tone_apply": 3 * 256 + 12 * 4 + 3 * 4, "dec_tone_sharp": 3 * 34 * 34 * 4}


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_tone_kernels_use_no_scratch_and_the_stated_lds(tmp_path, kernel):
    meta = metadata(LIB, tmp_path)
    lds = _lds(tmp_path)
    lines = []
    for form in (kernel + "(", kernel + "_batch("):
        hits = [(d, v) for d, v in meta.items() if "::" + form in d]
        assert len(hits) == 1, (form, [d for d, _ in hits])
        d, v = hits[0]
        lines.append(f"{d[:110]}: {v} lds {lds.get(d)}")
        assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
        assert v["private_segment_fixed_size"] == 0, lines[-1]
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, lines[-1]
        assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
        assert lds.get(d) == LDS[kernel], lines[-1]
    print("\n".join(lines))
