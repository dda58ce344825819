"""Budgets of the path-A ARM's pairs form after staging by wave-uniform rows (fwd_arm.hip,
arm_stage_tile), from the gfx950 code-object metadata of the built libccmi.so (no GPU needed).

The kernel is bound by its vector-instruction issue and runs 7 waves per SIMD at dim_arm 16 (8 at
dim_arm 8); 7 waves hold up to 72 VGPRs (512 a lane slot, granules of 8).  The row descriptors and the tile lookup live in
SGPRs, which must not push anything into scratch, and the tile (12 rows of 72 floats) is all the
LDS the kernel has."""
import pytest

from kernel_meta import LIB, metadata, waves

KERNELS = ["arm_fwd_pairs_kernel<16, 2, true>", "arm_fwd_pairs_kernel<16, -1, true>",
           "arm_fwd_pairs_kernel<8, 2, true>", "arm_fwd_pairs_kernel<8, -1, true>"]
MAX_VGPRS = 72
TILE_BYTES = 12 * 72 * 4


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return metadata(LIB, tmp_path_factory.mktemp("arm_stage_meta"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_pairs_kernel_budget(meta, kernel):
    hits = [(d, v) for d, v in meta.items() if kernel + "(" in d]
    assert len(hits) == 1, (kernel, [d for d, _ in hits])
    d, v = hits[0]
    line = f"{kernel}: {v}"
    print(line)
    assert v["vgpr_count"] <= MAX_VGPRS and waves(v["vgpr_count"]) >= 7, line
    assert v["private_segment_fixed_size"] == 0, line
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, line
    assert v["group_segment_fixed_size"] == TILE_BYTES, line
