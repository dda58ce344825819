"""Wide, flat frames: where launch_dec_arm leaves the chain kernel for the speculative one, and
where no ARM kernel takes the row (dec_arm.hip; d = 16, nh = 2, no block map, so max_blocks = 1).

With pitch = max_w + 2 * kPad = max_w + 16 and 160 KB = 163840 bytes of LDS:
  chain        4 * (4 + 17 * 50 + 2 + 16 * 16 + 16 + (256 + 8) * 16 + 4 * pitch) + 1 + 16
               = 21425 + 16 * pitch <= 163840   ->  pitch <= 8900  ->  max_w <= 8884
  speculative  4 * 4 * pitch + 1 + 16 + 4 * 17 * 50 * 2
               = 6817 + 16 * pitch <= 163840    ->  pitch <= 9813  ->  max_w <= 9797
  one-latent   4 * 5 * pitch + 1 + 16
               = 17 + 20 * pitch <= 163840      ->  pitch <= 8191  ->  max_w <= 8175
So 8884 is the widest latent row the chain kernel takes (163825 bytes of dynamic LDS), 8885 the
first that falls to the speculative kernel, and 9798 the first no kernel takes: past the
speculative kernel's bound, and the one-latent kernel gave up at 8176 already.  max_w is the
widest row of a call's run, so a small frame beside a wide one leaves the chain kernel with it."""
import pytest

import cool_gen as G
import test_decode_arch_gpu as A

pytestmark = pytest.mark.gpu

W_CHAIN, W_SPEC, W_NONE = 8884, 8885, 9798


def _wide(w, seed):
    return A.case(2, w, n_grids=3, d=16, nh=2, hls_sig_blksize=0, seed=seed)


def _stream(c, gpu):
    fr, lat = G.make(**c)
    data = G.write(fr, lat, gpu)
    fmt = A._formats(fr)[0]
    return fr, lat, data, fmt, A.oracle_decode(data, [fmt])


@pytest.mark.parametrize("w", [W_CHAIN, W_SPEC])
def test_widest_chain_row_and_first_speculative_row(w, gpu, ccmi_lib):
    import numpy as np
    from ccmi import decode
    c = _wide(w, 9000 + w)
    fr, lat, data, fmt, (sizes, olat, _, syn_out, (want,)) = _stream(c, gpu)
    assert sizes[0] == (2, w)
    A.assert_picture(syn_out, c["layers"], f"2x{w}")
    got = decode.decode_latents(data)
    assert decode.last_arm_flags() == [0]
    for g, a in zip(got, lat):
        assert np.array_equal(g, a)
    out, = decode.decode_batch([data], *fmt)
    assert out == want


def test_first_row_no_kernel_takes_is_refused_and_the_next_call_is_clean(gpu, ccmi_lib):
    from ccmi import ERR_UNSUPPORTED, decode
    _, _, data, fmt, _ = _stream(_wide(W_NONE, 9001), gpu)
    _, _, small, sfmt, (_, _, _, _, (want,)) = _stream(A.case(45, 83, seed=9002), gpu)
    with pytest.raises(decode.CcmiError, match="too large for LDS ring") as e:
        decode.decode_batch([data], *fmt)
    assert e.value.code == ERR_UNSUPPORTED
    out, = decode.decode_batch([small], *sfmt)
    assert out == want and decode.last_arm_flags() == [0]


def test_small_frame_beside_a_wide_one_leaves_the_chain_kernel_too(gpu, ccmi_lib):
    from ccmi import decode
    _, _, wide, fmt, (_, _, _, _, (want_w,)) = _stream(_wide(W_SPEC, 9003), gpu)
    _, _, small, sfmt, (_, _, _, _, (want_s,)) = _stream(A.case(45, 83, seed=9004), gpu)
    assert fmt == sfmt  # both rgb: one call, one (d, nh) group, one max_w
    outs = decode.decode_batch([small, wide], *fmt)
    assert decode.last_arm_flags() == [0, 0]
    assert outs[0] == want_s and outs[1] == want_w
