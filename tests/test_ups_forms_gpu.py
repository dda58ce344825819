"""The upsampling pyramid's default form (fwd_ups.hip: the channel-looping row kernel
ups_level_rows, a workgroup per 32 x 128 destination tile and run of at most three of its jobs)
against the form it replaced, one channel of a 16 x 64 tile per workgroup (CCMI_UPS_FORM_LEVELS,
stages bit 5 of ccmi_decode_forward_f32).  Both forms run the same fmaf chains in the same order,
so every comparison is torch.equal on every output element: there is no tolerance.  Parity of the
values with the oracle stays with tests/test_forward.py.

The sizes are the smallest that reach each path: grids of one element; a finest grid narrower
and lower than one tile; more than one tile both ways with odd widths (rows that are not 16-byte
aligned take the narrower stores), a last tile one column wide (129 x 257) and a full last tile;
a tile whose second refine half lies outside the grid (37 and 70 rows) and one where it does not;
chains of seven levels whose ceil-halves are odd somewhere.  With n_grids 2, 3, 5 and 7 a level
has 2 .. 7 jobs: runs of two and of three jobs, a run that starts with the refine and runs that do
not, one workgroup per tile and up to three.
"""
import ctypes as C

import pytest
import torch

import forward_oracle as fo

FINEST = [(1, 1), (1, 3), (9, 65), (23, 40), (37, 130), (70, 300), (129, 257)]
B = 3
PAD = 5  # floats of NaN between the frames' parameter blocks


def _chain(H, W, n):
    sizes = [(H, W)]
    while len(sizes) < n:
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def _n_grids(H, W):
    """2, 3, 5 and 7 where the size has that many distinct levels, else as many as it has (2 at the least)"""
    distinct = len(set(_chain(H, W, 12)))
    return sorted({max(2, min(n, distinct, 7)) for n in (2, 3, 5, 7)})


CASES = [(H, W, n) for H, W in FINEST for n in _n_grids(H, W)]
_INPUTS = {}


def _inputs(sizes, ups_k, n_ups, pre_k, n_pre, dev):
    """(latents [B, N], parameters [B, P + PAD] with NaN in the padding) of a case, made once and never modified"""
    key = (tuple(sizes), ups_k, n_ups, pre_k, n_pre)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(17 + 31 * sizes[0][0] + sizes[0][1] + 1000 * len(sizes) + n_ups)
        N = sum(h * w for h, w in sizes)
        P = n_ups * ups_k + n_pre * pre_k
        lat = 0.7 * torch.randn(B, N, generator=g)
        prm = torch.full((B, P + PAD), float("nan"))
        prm[:, :P] = 0.4 * torch.randn(B, P, generator=g)
        _INPUTS[key] = (lat.to(dev), prm.to(dev))
    return _INPUTS[key]


def _ups(lat, prm, sizes, ups_k, n_ups, pre_k, n_pre, quantize, form, shared_latent=False, ws=None, out=None):
    """One ccmi_ups_forward_f32_form call on the current stream; lat [B, N] (shared_latent: row 0 for every
    frame, latent_stride 0), prm [B, stride].  ws: the workspace to use (else a NaN-filled one)."""
    import ccmi
    from ccmi.forward import _grid_arrays
    dev = lat.device
    L = len(sizes)
    H, W = sizes[0]
    nb = prm.shape[0]
    h, w = _grid_arrays(sizes)
    nws = ccmi.lib().ccmi_ups_workspace_bytes(L, h, w, nb)
    if ws is None:
        ws = torch.full((max(nws // 4, 1),), float("nan"), device=dev)
    if out is None:
        out = torch.full((nb, L, H, W), float("nan"), device=dev)
    a = ccmi.UpsArgs(latent=ccmi.ptr(lat), latent_stride=0 if shared_latent else lat.shape[1], n_grids=L, h=h, w=w,
                     gain=16.0, quantize=int(quantize), ups_k=ups_k, n_ups=n_ups, pre_k=pre_k, n_pre=n_pre,
                     params=ccmi.ptr(prm), param_stride=prm.shape[1], out=ccmi.ptr(out), out_stride=L * H * W,
                     workspace=ccmi.ptr(ws), workspace_bytes=nws, batch=nb)
    ccmi.check(ccmi.lib().ccmi_ups_forward_f32_form(C.byref(a), ccmi.stream_handle(dev), form))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("quantize,many", [(1, True), (0, False), (1, False), (0, True)],
                         ids=["q-nmax", "noq-n1", "q-n1", "noq-nmax"])
@pytest.mark.parametrize("H,W,n", CASES, ids=["%dx%d-%d" % c for c in CASES])
def test_dense_output_equals_per_level_form(H, W, n, quantize, many, gpu, ccmi_lib):
    """Three frames with their own filters (NaN between the parameter blocks), then one latent vector
    under the three filter sets; the workspace is NaN-filled before each call."""
    import ccmi
    sizes = _chain(H, W, n)
    nf = n - 1 if many else 1
    lat, prm = _inputs(sizes, 8, nf, 7, nf, gpu)
    for shared in (False, True):
        new = _ups(lat, prm, sizes, 8, nf, 7, nf, quantize, ccmi.UPS_FORM_DEFAULT, shared)
        old = _ups(lat, prm, sizes, 8, nf, 7, nf, quantize, ccmi.UPS_FORM_LEVELS, shared)
        assert not bool(torch.isnan(old).any())
        assert torch.equal(new, old), (sizes, shared, int((new != old).sum()),
                                       [int((new[:, c] != old[:, c]).sum()) for c in range(n)])


_FRAMES = {}


def _frame(H, W):
    if (H, W) not in _FRAMES:
        mp = fo.ModelParams.random(H, W, seed=500 + H + W)
        g = torch.Generator().manual_seed(500 + H)
        _FRAMES[(H, W)] = (mp, [0.5 * torch.randn(h, w, generator=g) for h, w in mp.sizes])
    return _FRAMES[(H, W)]


@pytest.mark.gpu
@pytest.mark.parametrize("yuv420", [True, False], ids=["420", "444"])
@pytest.mark.parametrize("H,W", [(37, 130), (70, 300)])
def test_decoded_frame_equals_per_level_form(H, W, yuv420, gpu, ccmi_lib):
    """ccmi_decode_forward_f32 with and without stages bit 5 (hop): the level-1 stack that the fused
    kernel reads is the same, so the frames are."""
    from ccmi import forward as F
    mp, lat = _frame(H, W)
    assert mp.n_grids == 7
    flat = torch.cat([x.reshape(-1) for x in lat]).to(gpu)
    args = (flat, mp.sizes, F.pack_ups(mp.ups_full(), mp.pre_full()).to(gpu), mp.ups_k, len(mp.ups_half), mp.pre_k,
            len(mp.pre_half), mp.layers, F.pack_syn(mp.syn).to(gpu), mp.gain, True, 8, yuv420)
    new = F.decode_forward(*args)
    old = F.decode_forward(*args, ups_levels=True)
    assert not bool(torch.isnan(new).any())
    assert torch.equal(new, old), int((new != old).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,n", [(70, 300, 7), (129, 257, 7), (23, 40, 5)])
def test_nan_workspace_leaves_no_nan(H, W, n, gpu, ccmi_lib):
    """Every level a step reads was written by the step before it: with the workspace NaN-filled
    before a default-form call, no output is NaN."""
    import ccmi
    sizes = _chain(H, W, n)
    lat, prm = _inputs(sizes, 8, n - 1, 7, n - 1, gpu)
    out = _ups(lat, prm, sizes, 8, n - 1, 7, n - 1, 1, ccmi.UPS_FORM_DEFAULT)
    assert int(torch.isnan(out).sum()) == 0


@pytest.mark.gpu
def test_two_calls_on_one_stream_without_sync(gpu, ccmi_lib):
    """Two default-form calls back to back on one stream, one workspace, different filters: each gives
    its own per-level result."""
    import ccmi
    sizes = _chain(70, 300, 7)
    lat, prm1 = _inputs(sizes, 8, 6, 7, 6, gpu)
    prm2 = torch.flip(prm1, dims=[0]).contiguous()
    ref1 = _ups(lat, prm1, sizes, 8, 6, 7, 6, 1, ccmi.UPS_FORM_LEVELS)
    ref2 = _ups(lat, prm2, sizes, 8, 6, 7, 6, 1, ccmi.UPS_FORM_LEVELS)
    assert not torch.equal(ref1, ref2)
    ws = torch.full((ref1.numel(),), float("nan"), device=gpu)  # more than the workspace needs
    out1, out2 = torch.full_like(ref1, float("nan")), torch.full_like(ref1, float("nan"))
    torch.cuda.synchronize()
    _ups(lat, prm1, sizes, 8, 6, 7, 6, 1, ccmi.UPS_FORM_DEFAULT, ws=ws, out=out1)
    _ups(lat, prm2, sizes, 8, 6, 7, 6, 1, ccmi.UPS_FORM_DEFAULT, ws=ws, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(out1, ref1) and torch.equal(out2, ref2)


@pytest.mark.gpu
def test_graph_replay_equals_eager(gpu, ccmi_lib):
    """A default-form step captured into a HIP graph and replayed into cleared outputs equals the eager
    outputs (nothing is allocated or set up in the launch path)."""
    import ccmi
    sizes = _chain(70, 300, 7)
    lat, prm = _inputs(sizes, 8, 6, 7, 6, gpu)
    eager = _ups(lat, prm, sizes, 8, 6, 7, 6, 1, ccmi.UPS_FORM_DEFAULT)
    ws = torch.full((eager.numel(),), float("nan"), device=gpu)
    out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _ups(lat, prm, sizes, 8, 6, 7, 6, 1, ccmi.UPS_FORM_DEFAULT, ws=ws, out=out)
    for _ in range(2):
        out.zero_()
        ws.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.gpu
@pytest.mark.parametrize("ups_k,pre_k", [(4, 3), (8, 5), (6, 7)])
def test_other_tap_counts_run_the_generic_kernel(ups_k, pre_k, gpu, ccmi_lib):
    """Tap counts other than 8 / 7 keep the generic level kernel in both forms: this checks the dispatch."""
    import ccmi
    sizes = _chain(37, 130, 5)
    lat, prm = _inputs(sizes, ups_k, 2, pre_k, 2, gpu)
    new = _ups(lat, prm, sizes, ups_k, 2, pre_k, 2, 1, ccmi.UPS_FORM_DEFAULT)
    old = _ups(lat, prm, sizes, ups_k, 2, pre_k, 2, 1, ccmi.UPS_FORM_LEVELS)
    assert not bool(torch.isnan(new).any())
    assert torch.equal(new, old)


def test_unknown_form_is_refused(ccmi_lib):
    import ccmi
    a = ccmi.UpsArgs()
    assert ccmi.lib().ccmi_ups_forward_f32_form(C.byref(a), None, 2) == ccmi.ERR_ARG
