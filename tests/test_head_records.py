"""The fused kernel's head weight records (fwd_syn.hip: s_head, stage_head, head_hidden2 /
head_out2, the MFMA head's a1 gather).

A hidden unit's record holds w0[0..c_in), b0, w1[0..c_mid) dense from slot 0 and is read as
ceil((c_in + 1 + c_mid) / 4) 128-bit vectors; every FMA takes its weight as one half of an
aligned register pair of those.  Each field multiplies a different input (or is the bias), so a
field read from the wrong slot or the wrong half shows as an error of the order of the output,
far above the float tolerance.

Tolerance: test_forward.py's rule for the synthesis output, |err| <= 2e-5 (1 + |ref|_max)
(fp32 everywhere, summation order differs from PyTorch's).  Size 45 x 70: two column strips and
a second window, the smallest frame with both.
"""

import numpy as np
import pytest
import torch

import forward_oracle as fo

H, W = 45, 70


def _tol(ref):
    return 2e-5 * (1.0 + float(np.abs(ref).max()))


def _layers(hid, c_mid, relu):
    return fo.parse_layers(f"{hid}-1-linear-{'relu' if relu else 'none'}|{c_mid}-1-linear-none|"
                           f"{c_mid}-3-residual-relu|{c_mid}-3-residual-none")


def _lats(mp, seed):
    g = torch.Generator().manual_seed(seed)
    return [0.5 * torch.randn(h, w, generator=g) for h, w in mp.sizes]


def _fused(mps, lats, dev, bitdepth=0, yuv420=False, head=0):
    from ccmi import forward as F
    mp0 = mps[0]
    lat = torch.stack([torch.cat([x.reshape(-1) for x in l]) for l in lats]).to(dev)
    ups_p = torch.stack([F.pack_ups(mp.ups_full(), mp.pre_full()) for mp in mps]).to(dev)
    syn_p = torch.stack([F.pack_syn(mp.syn) for mp in mps]).to(dev)
    return F.decode_forward(lat, mp0.sizes, ups_p, mp0.ups_k, len(mp0.ups_half), mp0.pre_k, len(mp0.pre_half),
                            mp0.layers, syn_p, mp0.gain, True, bitdepth, yuv420, head)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("hid", [5, 16, 48, 64])
@pytest.mark.parametrize("c_mid", [3, 4])
@pytest.mark.parametrize("n_grids", [1, 2, 4, 7, 8])
def test_record_shape_matches_oracle(n_grids, c_mid, hid, relu, gpu, ccmi_lib):
    """One case per record shape (2 + c_mid .. 9 + c_mid fields, three or four vectors), odd and
    even unit counts, the unrolled 48-wide head (7 grids, ReLU) and the runtime-width loop.
    With one grid there is no upsampling to fuse: the same kernel on a one-channel input."""
    from ccmi import forward as F
    L = _layers(hid, c_mid, relu)
    seed = 1000 * n_grids + 100 * c_mid + hid + int(relu)
    mp = fo.ModelParams.random(H, W, layers=L, n_grids=n_grids, seed=seed)
    if n_grids == 1:
        x = torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed)) * 4
        ref = fo.synthesis(x, L, mp.syn).numpy()
        out = F.syn_forward(x.to(gpu), L, F.pack_syn(mp.syn).to(gpu)).cpu().numpy()
    else:
        lat = _lats(mp, seed)
        ref = fo.forward(mp, lat)["syn"].numpy()
        out = _fused([mp], [lat], gpu)[0].cpu().numpy()
    err = float(np.abs(out - ref).max())
    print(f"n_grids {n_grids} c_mid {c_mid} hid {hid} relu {relu}: max err {err:.3g}, tol {_tol(ref):.3g}")
    np.testing.assert_allclose(out, ref, rtol=0, atol=_tol(ref))


@pytest.fixture(scope="module", params=[(45, 70), (61, 61)], ids=lambda s: f"{s[0]}x{s[1]}")
def hop(request):
    """A random hop decoder (7 grids, 48-wide head), its latents and the oracle's output."""
    h, w = request.param
    mp = fo.ModelParams.random(h, w, seed=h + w)
    assert mp.n_grids == 7 and mp.layers[0][0] == 48
    lat = _lats(mp, h * w)
    return mp, lat, fo.forward(mp, lat)["syn"].numpy()


@pytest.mark.gpu
def test_hop_unrolled_head_bitwise_generic(hop, gpu, ccmi_lib):
    """The unrolled head against the runtime-width loop, which reads the same records through
    the same statements: bit for bit in the raw output and the three post-processed formats
    (8-bit table and general quotient, 444 and 420)."""
    import ccmi
    mp, lat, _ = hop
    for bd, yuv in ((0, False), (8, False), (8, True), (10, True)):
        a = _fused([mp], [lat], gpu, bd, yuv, ccmi.HEAD_DEFAULT)
        b = _fused([mp], [lat], gpu, bd, yuv, ccmi.HEAD_GENERIC)
        assert torch.equal(a, b), (bd, yuv)


@pytest.mark.gpu
def test_hop_mfma_head_matches_oracle(hop, gpu, ccmi_lib):
    """The MFMA head gathers w0 and the bias from the records by slot (a1)."""
    import ccmi
    mp, lat, ref = hop
    out = _fused([mp], [lat], gpu, head=ccmi.HEAD_MFMA)[0].cpu().numpy()
    err = float(np.abs(out - ref).max())
    print(f"MFMA head {mp.H} x {mp.W}: max err {err:.3g}, tol {_tol(ref):.3g}")
    np.testing.assert_allclose(out, ref, rtol=0, atol=_tol(ref))


@pytest.mark.gpu
def test_three_frames_own_records(gpu, ccmi_lib):
    """Three frames with their own weights in one launch: the records are staged per frame, so
    frame b equals a batch-of-1 run of frame b."""
    mps = [fo.ModelParams.random(H, W, seed=70 + i) for i in range(3)]
    lats = [_lats(mp, 700 + i) for i, mp in enumerate(mps)]
    both = _fused(mps, lats, gpu)
    for i in range(3):
        assert torch.equal(both[i], _fused([mps[i]], [lats[i]], gpu)[0]), i
