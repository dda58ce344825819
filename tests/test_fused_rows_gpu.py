"""The fused decode kernel's row layout (fwd_syn.hip): a thread's four rows as stride-2 pairs
{row q, row q + 2}, a last layer that evaluates the chroma channels of a 4:2:0 output on even
rows only, and (a build option, CCMI_FUSED_RUN_RECS) the head's weight records staged once per run.

All of it keeps every pixel's arithmetic, so the checks are equalities: the 4:2:0 planes against
the 4:4:4 planes of the same library (the 4:4:4 path evaluates every row: a wrong pair or half
shows as whole rows differing), frames of a batch against batch-of-one runs (records staged per
run must stay per frame), the walk against single-window runs; and the oracle for the decoders
no other test runs through these paths.
"""
import numpy as np
import pytest
import torch

from test_forward import _ties_only, _tol
from test_fused_walk import FORMATS, _case, _decode

import forward_oracle as fo

# hop sizes, the smallest that reach each case: degenerate and the first chroma sample; odd height,
# a second window of one row, two strips; a two-window run; three windows, odd both ways; two runs;
# a three-column image
HOP_SIZES = [(1, 1), (2, 2), (29, 70), (60, 64), (61, 61), (189, 130), (188, 3)]
N_SP1 = "3-1-linear-none|3-3-residual-relu"
N_SP3 = "16-1-linear-relu|3-1-linear-none|3-3-residual-relu|3-3-residual-none|3-3-linear-none"
TAIL4 = "16-1-linear-relu|4-1-linear-none|4-3-residual-relu|4-3-linear-none"
CASES_420 = [(H, W, None) for H, W in HOP_SIZES] + [(95, 70, N_SP1), (120, 96, N_SP3)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,layers", CASES_420,
                         ids=["hop_%dx%d" % s for s in HOP_SIZES] + ["n_sp1_95x70", "n_sp3_120x96"])
def test_420_planes_equal_444_planes(H, W, layers, gpu, ccmi_lib):
    """8 and 10 bit: the 4:2:0 luma plane is the 4:4:4 one, each chroma plane the 4:4:4 plane at
    even rows and columns."""
    mp, lat, _ = _case(H, W, layers)
    assert mp.layers[-1][0] == 3
    h2, w2 = H >> 1, W >> 1
    for bd in (8, 10):
        full = _decode([mp], [lat], gpu, bd, False)[0]
        sub = _decode([mp], [lat], gpu, bd, True)[0]
        assert full.shape == (3, H, W) and sub.numel() == H * W + 2 * h2 * w2
        luma = sub[:H * W].view(H, W)
        bad = (luma != full[0]).any(dim=1).nonzero().flatten().tolist()
        assert torch.equal(luma, full[0]), (H, W, bd, "luma rows", bad[:8])
        for m in (1, 2):
            c = sub[H * W + (m - 1) * h2 * w2:H * W + m * h2 * w2].view(h2, w2)
            want = full[m][0:2 * h2:2, 0:2 * w2:2]
            bad = (c != want).any(dim=1).nonzero().flatten().tolist()
            assert torch.equal(c, want), (H, W, bd, "chroma", m, "rows", bad[:8])


@pytest.mark.gpu
def test_n_sp3_three_channels(gpu, ccmi_lib):
    """Three 3x3 layers on three channels, through the post stage: the oracle (raw, and 8-bit
    4:4:4 up to rounding ties) and single-window runs bit for bit, per format."""
    mp, lat, ref = _case(120, 96, N_SP3)
    assert len(mp.layers) == 5 and mp.layers[-1][0] == 3
    tol = _tol(ref)
    raw = _decode([mp], [lat], gpu, 0, False)[0].cpu().numpy()
    print("n_sp 3, 3 channels: max |err| %.3g (tol %.3g)" % (float(np.abs(raw - ref).max()), tol))
    np.testing.assert_allclose(raw, ref, rtol=0, atol=tol)
    _ties_only(_decode([mp], [lat], gpu, 8, False)[0].cpu().numpy(), ref, tol)
    for bd, yuv in FORMATS:
        a = _decode([mp], [lat], gpu, bd, yuv, walk=True)
        b = _decode([mp], [lat], gpu, bd, yuv, walk=False)
        assert torch.equal(a, b), (bd, yuv, int((a != b).sum()))


@pytest.mark.gpu
def test_batch_frames_keep_their_records(gpu, ccmi_lib):
    """Three hop frames with their own weights, two runs each: frame b of the batch equals a
    batch-of-one run of frame b (8-bit 4:2:0 and raw)."""
    mps = [fo.ModelParams.random(189, 70, seed=160 + i) for i in range(3)]
    lats = []
    for i, mp in enumerate(mps):
        g = torch.Generator().manual_seed(1600 + i)
        lats.append([0.5 * torch.randn(h, w, generator=g) for h, w in mp.sizes])
    for bd, yuv in ((8, True), (0, False)):
        both = _decode(mps, lats, gpu, bd, yuv)
        for i in range(3):
            one = _decode([mps[i]], [lats[i]], gpu, bd, yuv)[0]
            assert torch.equal(both[i], one), (i, bd, int((both[i] != one).sum()))


@pytest.mark.gpu
def test_four_channel_tail_matches_oracle(gpu, ccmi_lib):
    """The four-channel tail (the row pairs alone: no post stage)."""
    mp, lat, ref = _case(61, 70, TAIL4)
    tol = _tol(ref)
    raw = _decode([mp], [lat], gpu, 0, False)[0].cpu().numpy()
    print("4-channel tail: max |err| %.3g (tol %.3g)" % (float(np.abs(raw - ref).max()), tol))
    np.testing.assert_allclose(raw, ref, rtol=0, atol=tol)
