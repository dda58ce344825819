"""Register and LDS budget of the fused decode kernels whose row layout and last layer
fwd_syn.hip's stride-2 row pairs changed (CPU only: the built library's code-object
metadata, kernel_meta.py).  Three workgroups per CU need at most 80 VGPRs (6 waves per SIMD) and
160 KB / 3 = 54,613 B of LDS each."""
import pytest

import kernel_meta as km

LDS_MAX = 160 * 1024 // 3  # 54,613 B
THREE_CHANNEL = ("7, 3, true, false, 48, false", "7, 3, true, false, 0, false", "7, 3, true, false, 48, true")
FOUR_CHANNEL = ("7, 4, true, false, 0, false", "7, 4, true, false, 48, false")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return km.metadata(km.LIB, tmp_path_factory.mktemp("fused_rows_meta"))


def _kernel(meta, args):
    hits = [d for d in meta if "syn_fused_kernel<%s>" % args in d]
    assert len(hits) == 1, (args, hits)
    print("syn_fused_kernel<%s>: %s" % (args, meta[hits[0]]))
    return meta[hits[0]]


@pytest.mark.parametrize("args", THREE_CHANNEL)
def test_three_channel_kernels_keep_three_workgroups(meta, args):
    v = _kernel(meta, args)
    assert v["vgpr_count"] <= 80, v
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v["private_segment_fixed_size"] == 0, v
    assert v["group_segment_fixed_size"] <= LDS_MAX, v


@pytest.mark.parametrize("args", FOUR_CHANNEL)
def test_four_channel_kernels_keep_their_lds(meta, args):
    v = _kernel(meta, args)
    assert v["group_segment_fixed_size"] <= LDS_MAX, v
    assert v["private_segment_fixed_size"] == 0, v
