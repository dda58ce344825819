"""The fused decode kernel's walk: a workgroup evaluates a run of consecutive 32-row windows of
one column strip and carries the 3x3 layers' last two rows from window to window, so only a
run's first window pays the vertical halo (fwd_syn.hip, ccmi_fused_run_plan).

GPU tests: the walk against the oracle (test_forward.py's tolerance rule) and, bit for bit,
against single-window runs (decode_forward(walk=False), stages bit 4), at the smallest sizes
that reach each case of the walk.  CPU tests: the run plan tiles every height, and the sizes
used here really exercise runs of several windows at the built cap.
"""
import math

import numpy as np
import pytest
import torch

import forward_oracle as fo
from test_forward import HEADS, _ties_only, _tol

# (H, W): why
SIZES = [
    (29, 70),    # second window emits one row
    (60, 64),    # a 2-window run exactly
    (61, 61),    # 3 windows
    (189, 130),  # splits into two runs at cap 6
    (381, 70),   # three runs
    (188, 3),    # one full run, a 3-column image
    (1, 1),      # degenerate
]
N_SP_HOP = 2
# (H, W, layers or None for hop, fold)
VARIANTS = [
    (189, 130, None, True),
    (95, 70, "3-1-linear-none|3-3-residual-relu", False),                                                   # n_sp = 1
    (120, 96, "16-1-linear-relu|4-1-linear-none|4-3-residual-relu|4-3-residual-none|4-3-linear-none", False),  # n_sp = 3
    (45, 70, "16-1-linear-relu|3-1-linear-none", False),                                                    # head only
]
FORMATS = ((0, False), (8, False), (8, True), (10, True))  # raw, 8-bit 444, 8-bit 420, 10-bit 420

_CASES = {}


def _case(H, W, layers=None):
    """(model, latents, oracle output) of a size, computed once and shared (never modified)."""
    key = (H, W, layers)
    if key not in _CASES:
        seed = 1000 + 7 * H + W
        kw = {} if layers is None else {"layers": fo.parse_layers(layers)}
        mp = fo.ModelParams.random(H, W, seed=seed, **kw)
        g = torch.Generator().manual_seed(seed)
        lat = [0.5 * torch.randn(h, w, generator=g) for h, w in mp.sizes]
        _CASES[key] = (mp, lat, fo.forward(mp, lat)["syn"].numpy())
    return _CASES[key]


def _decode(mps, lats, dev, bitdepth, yuv420, head=0, fold=False, walk=True):
    from ccmi import forward as F
    mp0 = mps[0]
    lat = torch.stack([torch.cat([x.reshape(-1) for x in l]) for l in lats]).to(dev)
    ups_p = torch.stack([F.pack_ups(mp.ups_full(), mp.pre_full()) for mp in mps]).to(dev)
    syn_p = torch.stack([F.pack_syn(mp.syn) for mp in mps]).to(dev)
    return F.decode_forward(lat, mp0.sizes, ups_p, mp0.ups_k, len(mp0.ups_half), mp0.pre_k, len(mp0.pre_half),
                            mp0.layers, syn_p, mp0.gain, True, bitdepth, yuv420, head, fold, walk)


def _check(mp, lat, ref, dev, head, fold=False):
    """Walk vs oracle (raw and 8-bit), then walk vs single-window runs bit for bit, per format."""
    tol = _tol(ref)
    raw = _decode([mp], [lat], dev, 0, False, head, fold)
    err = float(np.abs(raw[0].cpu().numpy() - ref).max())
    print(f"{mp.H}x{mp.W} head {head} fold {fold}: max |err| {err:.3g} (tol {tol:.3g})")
    np.testing.assert_allclose(raw[0].cpu().numpy(), ref, rtol=0, atol=tol)
    formats = FORMATS if mp.layers[-1][0] == 3 else FORMATS[:1]  # post-processing needs 3 planes
    if len(formats) > 1:
        dec = _decode([mp], [lat], dev, 8, False, head, fold)[0].cpu().numpy()
        _ties_only(dec, ref, tol)
    for bd, yuv in formats:
        a = _decode([mp], [lat], dev, bd, yuv, head, fold, walk=True)
        b = _decode([mp], [lat], dev, bd, yuv, head, fold, walk=False)
        assert torch.equal(a, b), (mp.H, mp.W, bd, yuv, int((a != b).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("H,W", SIZES)
def test_walk_hop_matches_oracle_and_single_windows(H, W, head, gpu, ccmi_lib):
    """Hop decoder (48-wide head, 7 grids, two 3x3 layers), both head forms."""
    mp, lat, ref = _case(H, W)
    assert mp.n_grids == 7 and mp.layers[0][0] == 48 and len(mp.layers) == 2 + N_SP_HOP
    _check(mp, lat, ref, gpu, head)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,layers,fold", VARIANTS, ids=["fold", "n_sp1", "n_sp3_4ch", "head_only"])
def test_walk_variants(H, W, layers, fold, gpu, ccmi_lib):
    """The folded level-2 -> 1 instantiation, one and three 3x3 layers (4 channels), no 3x3 layer."""
    mp, lat, ref = _case(H, W, layers)
    _check(mp, lat, ref, gpu, 1, fold)


@pytest.mark.gpu
def test_walk_batch_own_weights(gpu, ccmi_lib):
    """Three frames with their own weights in one launch: frame b equals a batch-of-1 run of frame b."""
    mps = [fo.ModelParams.random(96, 160, seed=60 + i) for i in range(3)]
    lats = []
    for i, mp in enumerate(mps):
        g = torch.Generator().manual_seed(600 + i)
        lats.append([0.5 * torch.randn(h, w, generator=g) for h, w in mp.sizes])
    for bd, yuv in ((0, False), (8, True)):
        both = _decode(mps, lats, gpu, bd, yuv)
        for i in range(3):
            assert torch.equal(both[i], _decode([mps[i]], [lats[i]], gpu, bd, yuv)[0]), (i, bd)
            assert torch.equal(both[i], _decode([mps[i]], [lats[i]], gpu, bd, yuv, walk=False)[0]), (i, bd)


# ----------------------------------------------------------------------------- CPU: the run plan

def _plan(h, n_sp, cap=0):
    from ccmi import forward as F
    return F.fused_run_plan(h, n_sp, cap)


def test_sizes_reach_the_walk(ccmi_lib):
    """A build with a small cap must not quietly test nothing: among the sizes above, at the built
    cap, some frame splits into two or more runs and some run walks three or more windows."""
    plans = [_plan(H, N_SP_HOP)[1] for H, _ in SIZES]
    assert any(len(runs) >= 2 for runs in plans), plans
    assert any(w >= 3 for runs in plans for _, w in runs), plans


def test_run_plan_tiles_every_height(ccmi_lib):
    """Runs tile [0, H) in order, hold 1 .. cap windows (cap 1 without 3x3 layers), and never use
    more windows than single-window runs would: every H in 1 .. 2200, n_sp in 0 .. 4."""
    for h in range(5):
        for H in range(1, 2201):
            cap, runs = _plan(H, h)
            assert cap >= 1 and (h > 0 or cap == 1)
            pos = 0
            for i, (start, wins) in enumerate(runs):
                assert start == pos and 1 <= wins <= cap, (H, h, runs)
                pos = start + 32 * wins - 2 * h
                assert pos > start
                if i < len(runs) - 1:
                    assert pos < H, (H, h, runs)
            assert pos >= H, (H, h, runs)  # the last run is clipped at H
            assert sum(w for _, w in runs) <= math.ceil(H / (32 - 2 * h)), (H, h, runs)


def test_run_plan_720_rows(ccmi_lib):
    cap, runs = _plan(720, 2, 6)
    assert cap == 6 and [w for _, w in runs] == [6, 6, 6, 5]
    assert [s for s, _ in runs] == [0, 188, 376, 564]
    assert _plan(720, 2, 1)[1] == [(28 * i, 1) for i in range(26)]  # cap 1: every window pays the halo
    assert _plan(45, 0, 6) == (1, [(0, 1), (32, 1)])
