"""Budget of the upsampling pyramid's default-form kernel (fwd_ups.hip), from the gfx950
code-object metadata of the built libccmi.so (no GPU needed).

ups_level_rows<8, 7> is bound by how many tiles the chip has in flight, so it wants many resident
workgroups, each with its whole tile's loads outstanding.  Its LDS is the refine half's 22 x 136
staged floats and 22 x 128 horizontal results (a channel's 20 x 68 and 20 x 128 lie over them):
23,232 bytes, six workgroups of the 160 KiB of a CU, twenty-four waves.  Six waves per SIMD hold
at most 80 VGPRs (512 a lane slot, granules of 8); with more, the registers and not the LDS would
set the residency."""
import pytest

from kernel_meta import LIB, metadata, waves

# kernel: (max VGPRs, least waves per SIMD, LDS bytes)
BUDGET = {
    "ups_level_rows<8, 7>": (80, 6, 23232),
}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return metadata(LIB, tmp_path_factory.mktemp("ups_meta"))


@pytest.mark.parametrize("kernel", list(BUDGET))
def test_ups_kernel_budget(meta, kernel):
    max_vgprs, min_waves, lds = BUDGET[kernel]
    hits = [(d, v) for d, v in meta.items() if kernel + "(" in d]
    assert len(hits) == 1, (kernel, [d for d, _ in hits])
    d, v = hits[0]
    line = f"{kernel}: {v}"
    print(line)
    assert v["vgpr_count"] <= max_vgprs and waves(v["vgpr_count"]) >= min_waves, line
    assert v["private_segment_fixed_size"] == 0, line
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, line
    assert v["group_segment_fixed_size"] == lds, line
    assert lds <= 64 * 1024, line


def test_the_per_level_kernels_remain(meta):
    """the per-level form's kernels stay in the library (CCMI_UPS_FORM_LEVELS, other tap counts)"""
    for kernel in ("ups_level_fixed<8, 7>(", "ups_level_kernel("):
        assert any(kernel in d for d in meta), kernel
