"""The packed weight copy of the path-A ARM's pairs form, without a GPU: the permutation
(ccmi_arm_pack_host, the host form of fwd_common.h's arm_pack_src that arm_pack_kernel applies)
against a numpy transposition, and the register budget of arm_fwd_pairs_kernel from the built
library's code-object metadata."""
import ctypes as C

import numpy as np
import pytest

from kernel_meta import LIB, metadata

ROW = 16  # floats: every row starts on a 64-byte boundary


def _reference(params, d, nh):
    """The layout ccmi.h documents, built from the public parameter order with numpy."""
    rs = -(-d // ROW) * ROW
    blocks, at = [], 0
    for _ in range(nh):
        W = params[at:at + d * d].reshape(d, d)  # [out j][in i]
        b = params[at + d * d:at + d * d + d]
        at += d * d + d
        layer = np.zeros((d + 1, rs), np.float32)
        layer[:d, :d] = W.T  # row i = the d weights that multiply input i
        layer[d, :d] = b
        blocks.append(layer.reshape(-1))
    Wo = params[at:at + 2 * d].reshape(2, d)
    bo = params[at + 2 * d:at + 2 * d + 2]
    blocks += [Wo.T.reshape(-1), bo]  # (W_out[0][i], W_out[1][i]) for i < d, then b_out
    flat = np.concatenate(blocks)
    stride = -(-flat.size // ROW) * ROW
    return np.concatenate([flat, np.zeros(stride - flat.size, np.float32)]), rs


@pytest.mark.parametrize("nh", range(5))
@pytest.mark.parametrize("d", [8, 16, 24, 32])
def test_pack_host_is_the_documented_transposition(ccmi_lib, d, nh):
    n = nh * (d * d + d) + 2 * d + 2
    params = (np.arange(n, dtype=np.float32) + 1.0)  # every value distinct and non-zero
    ref, rs = _reference(params, d, nh)
    out = np.full(ref.size + 8, -1.0, np.float32)
    fp = C.POINTER(C.c_float)
    got = ccmi_lib.ccmi_arm_pack_host(params.ctypes.data_as(fp), d, nh, out.ctypes.data_as(fp))
    assert got == ref.size and got % ROW == 0  # frame stride: a multiple of 64 bytes
    np.testing.assert_array_equal(out[:got], ref)
    assert np.all(out[got:] == -1.0)  # nothing written past the block
    # alignment: each hidden row and the output block start on a 64-byte boundary
    assert rs % ROW == 0 and (nh * (d + 1) * rs) % ROW == 0
    # a permutation: every parameter appears exactly once
    np.testing.assert_array_equal(np.sort(out[:got][out[:got] != 0]), params)


def test_pack_host_rejects_bad_arguments(ccmi_lib):
    buf = np.zeros(64, np.float32)
    fp = C.POINTER(C.c_float)
    assert ccmi_lib.ccmi_arm_pack_host(None, 16, 2, buf.ctypes.data_as(fp)) == -1
    assert ccmi_lib.ccmi_arm_pack_host(buf.ctypes.data_as(fp), 16, -1, buf.ctypes.data_as(fp)) == -1


def test_pairs_kernel_register_budget(tmp_path):
    """At most 72 VGPRs (7 waves / SIMD, as the row form), no VGPR or SGPR spill, no scratch."""
    meta = metadata(LIB, tmp_path)
    for key in ("arm_fwd_pairs_kernel<16, 2, ", "arm_fwd_pairs_kernel<16, -1, ",
                "arm_fwd_pairs_kernel<8, 2, ", "arm_fwd_pairs_kernel<8, -1, "):
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 2, f"kernel {key}: plain and scaled-ReLU form expected in libccmi.so, found {hits}"
        for n, v in hits:
            assert v.get("vgpr_count", 0) <= 72, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0, (n, v)
            assert v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
