"""Register / scratch / LDS use of the MS-SSIM kernels (dist_msssim.hip: ms_pool, ms_stat, ms_reduce,
ms_grad), read from the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_mix_resources.py (no GPU needed).

No kernel may use scratch or spill; static LDS stays at or under 80 KiB so that two workgroups share a
CU's 160 KiB (measured: 32,128 bytes for ms_stat, 29,184 for ms_grad, 1,024 for ms_reduce, none for ms_pool); VGPRs stay at or under the
occupancy step just above what was measured (MEASURED below: 22, 104, 36 and 64 VGPRs, so 8, 4, 8 and 8
waves per SIMD as far as registers go; ms_stat's 4 waves are the 4 workgroups its LDS admits less one)."""
import re

from kernel_meta import LIB, metadata, waves

MAX_LDS = 80 * 1024
# kernel -> (VGPRs measured, the step they must stay under)
MEASURED = {"ms_pool": (22, 64), "ms_stat": (104, 128), "ms_reduce": (36, 64), "ms_grad": (64, 64)}


def test_msssim_kernels_use_no_scratch_and_fit_two_workgroups_per_cu(tmp_path):
    meta = metadata(LIB, tmp_path)
    lines = []
    for k, (_, cap) in MEASURED.items():
        hits = [(d, v) for d, v in meta.items() if re.search(r"(?<![\w])%s\(" % k, d.replace("(anonymous namespace)::", ""))]
        assert len(hits) == 1, (k, [d for d, _ in hits])
        d, v = hits[0]
        lines.append(f"{k}: {v}, {waves(v.get('vgpr_count', 512))} waves")
        print(lines[-1])
        assert "vgpr_count" in v and "private_segment_fixed_size" in v and "group_segment_fixed_size" in v, lines[-1]
        assert v["private_segment_fixed_size"] == 0, lines[-1]
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, lines[-1]
        assert v["group_segment_fixed_size"] <= MAX_LDS, lines[-1]
        assert v["vgpr_count"] <= cap, lines[-1]
