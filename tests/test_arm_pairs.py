"""The pairs form of the path-A ARM (arm_fwd_pairs_kernel, ccmi_arm_forward_f32_form) against the
row form (arm_fwd_kernel): the same bits in rate, mu, scale and log_scale, on frames chosen for
where 8 x 64 tiles go wrong, and the contract of the packed-weight buffer (ordered on a stream,
stable under graph replay, never allocated inside a capture).

Bit equality needs no tolerance: both forms start every output unit at (a_j + b_j) and add the
products for i = 0 .. d-1 in order with fused multiply-adds; only the packing differs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

OUTS = ("mu", "scale", "log_scale", "rate")
ROWS, PAIRS = 1, 2
FILL = -7.0
PAD = 3  # out_stride - latents of a frame: the padding must stay untouched

# frame (h, w), grids
SHAPES = {
    "1x1": ((1, 1), 1),           # smallest case
    "9x65": ((9, 65), 3),         # one row / column past a tile, grids down to 3 x 17
    "23x40": ((23, 40), 7),       # ends in 1 x 1 grids
    "37x130": ((37, 130), 4),     # general multi-tile case
}


def _sizes(hw, n):
    h, w = hw
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def _count(d, nh):
    return nh * (d * d + d) + 2 * d + 2


def _inputs(dev, sizes, d, nh, batch, seed, pad=7):
    """Latents [batch, N] and parameters [batch, count + pad] (a stride larger than the count)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(h * w for h, w in sizes)
    lat = 0.4 * torch.randn(batch, n, generator=g)
    par = torch.randn(batch, _count(d, nh) + pad, generator=g) * (0.5 / d ** 0.5)
    return lat.to(dev), par.to(dev)


def _call(lib, form, lat, par, sizes, d, nh, quantize=1, want=OUTS, lat_stride=None, par_stride=None, batch=None,
          stream=None, outs=None):
    """One ccmi_arm_forward_f32_form call; returns (rc, outputs).  Outputs are pre-filled."""
    import ccmi
    from ccmi import forward as F
    n = sum(h * w for h, w in sizes)
    batch = lat.shape[0] if batch is None else batch
    if outs is None:
        outs = {k: torch.full((batch, n + PAD), FILL, device=lat.device) for k in want}
    h, w = F._grid_arrays(sizes)
    a = ccmi.ArmArgs(latent=ccmi.ptr(lat), latent_stride=n if lat_stride is None else lat_stride, n_grids=len(sizes),
                     h=h, w=w, gain=16.0, quantize=quantize, dim_arm=d, n_hidden=nh, params=ccmi.ptr(par),
                     param_stride=par.shape[1] if par_stride is None else par_stride,
                     mu=ccmi.ptr(outs.get("mu")), scale=ccmi.ptr(outs.get("scale")),
                     log_scale=ccmi.ptr(outs.get("log_scale")), rate=ccmi.ptr(outs.get("rate")),
                     out_stride=n + PAD, batch=batch)
    s = stream if stream is not None else torch.cuda.current_stream(lat.device)
    return lib.ccmi_arm_forward_f32_form(C.byref(a), s.cuda_stream, form), outs


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
        assert not torch.isnan(a[k]).any(), (what, k)


def _written(outs, n):
    for k, v in outs.items():
        assert bool((v[:, n:] == FILL).all()), f"{k}: padding written"
        assert bool((v[:, :n] != FILL).all()), f"{k}: a latent not written"


@pytest.mark.parametrize("nh", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [8, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pairs_equal_rows(ccmi_lib, gpu, shape, d, nh):
    """Batch 3, own weights per frame, param_stride larger than the parameter count, quantize 0
    and 1; the default form gives the pairs form's bits."""
    sizes = _sizes(*SHAPES[shape])
    n = sum(h * w for h, w in sizes)
    lat, par = _inputs(gpu, sizes, d, nh, 3, seed=100 * d + nh)
    for quantize in (1, 0):
        x = lat if quantize else torch.round(16.0 * lat)
        rc1, rows = _call(ccmi_lib, ROWS, x, par, sizes, d, nh, quantize)
        rc2, pairs = _call(ccmi_lib, PAIRS, x, par, sizes, d, nh, quantize)
        rc0, dflt = _call(ccmi_lib, 0, x, par, sizes, d, nh, quantize)
        torch.cuda.synchronize()
        assert (rc1, rc2, rc0) == (0, 0, 0)
        _written(rows, n)
        _same(pairs, rows, f"quantize {quantize}")
        _same(dflt, pairs, f"default form, quantize {quantize}")
    # the frames have their own weights: their outputs differ
    assert not torch.equal(rows["mu"][0], rows["mu"][1])


@pytest.mark.parametrize("shape", ["9x65", "37x130"])
def test_shared_latents_and_shared_weights(ccmi_lib, gpu, shape):
    """latent_stride 0 (one latent vector, three models) and param_stride 0 (one model)."""
    sizes = _sizes(*SHAPES[shape])
    lat, par = _inputs(gpu, sizes, 16, 2, 3, seed=7)
    for kw in (dict(lat_stride=0), dict(par_stride=0), dict(lat_stride=0, par_stride=0)):
        _, rows = _call(ccmi_lib, ROWS, lat, par, sizes, 16, 2, batch=3, **kw)
        rc, pairs = _call(ccmi_lib, PAIRS, lat, par, sizes, 16, 2, batch=3, **kw)
        torch.cuda.synchronize()
        assert rc == 0
        _same(pairs, rows, str(kw))
    assert torch.equal(pairs["rate"][0], pairs["rate"][2])  # everything shared: the frames agree


@pytest.mark.parametrize("skip", OUTS)
def test_each_output_optional(ccmi_lib, gpu, skip):
    sizes = _sizes(*SHAPES["23x40"])
    lat, par = _inputs(gpu, sizes, 8, 2, 3, seed=11)
    want = tuple(k for k in OUTS if k != skip)
    _, rows = _call(ccmi_lib, ROWS, lat, par, sizes, 8, 2, want=want)
    rc, pairs = _call(ccmi_lib, PAIRS, lat, par, sizes, 8, 2, want=want)
    torch.cuda.synchronize()
    assert rc == 0
    _same(pairs, rows)
    # a single output on its own, as the benchmark asks for the rate
    _, rows = _call(ccmi_lib, ROWS, lat, par, sizes, 8, 2, want=(skip,))
    _, pairs = _call(ccmi_lib, PAIRS, lat, par, sizes, 8, 2, want=(skip,))
    torch.cuda.synchronize()
    _same(pairs, rows)


def test_pairs_form_refused_where_absent(ccmi_lib, gpu):
    import ccmi
    sizes = _sizes(*SHAPES["9x65"])
    lat, par = _inputs(gpu, sizes, 24, 1, 1, seed=3)
    rc, _ = _call(ccmi_lib, PAIRS, lat, par, sizes, 24, 1)
    assert rc == ccmi.ERR_UNSUPPORTED and "pairs" in ccmi.last_error()
    rc0, dflt = _call(ccmi_lib, 0, lat, par, sizes, 24, 1)
    rc1, rows = _call(ccmi_lib, ROWS, lat, par, sizes, 24, 1)
    torch.cuda.synchronize()
    assert (rc0, rc1) == (0, 0)
    _same(dflt, rows)
    assert _call(ccmi_lib, 3, lat, par, sizes, 24, 1)[0] == ccmi.ERR_ARG


def test_two_calls_on_one_stream_are_ordered(ccmi_lib, gpu):
    """Different weights in two calls without a sync between them: the second call's pack may not
    overwrite the buffer before the first call's kernel has read it."""
    sizes = _sizes(*SHAPES["37x130"])
    lat, par1 = _inputs(gpu, sizes, 16, 2, 3, seed=21)
    _, par2 = _inputs(gpu, sizes, 16, 2, 3, seed=22)
    _, ref1 = _call(ccmi_lib, ROWS, lat, par1, sizes, 16, 2)
    _, ref2 = _call(ccmi_lib, ROWS, lat, par2, sizes, 16, 2)
    torch.cuda.synchronize()
    rc1, out1 = _call(ccmi_lib, PAIRS, lat, par1, sizes, 16, 2)
    rc2, out2 = _call(ccmi_lib, PAIRS, lat, par2, sizes, 16, 2)
    torch.cuda.synchronize()
    assert (rc1, rc2) == (0, 0)
    _same(out1, ref1, "first call")
    _same(out2, ref2, "second call")
    assert not torch.equal(ref1["mu"], ref2["mu"])


def test_graph_replays_equal_eager(ccmi_lib, gpu):
    """One eager call on the stream (which gives it its buffer), then the call captured in a
    graph and replayed twice into cleared outputs."""
    sizes = _sizes(*SHAPES["37x130"])
    lat, par = _inputs(gpu, sizes, 16, 2, 3, seed=31)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        rc, eager = _call(ccmi_lib, 0, lat, par, sizes, 16, 2, stream=s)
        s.synchronize()
        assert rc == 0
        eager = {k: v.clone() for k, v in eager.items()}
        outs = {k: torch.full_like(v, FILL) for k, v in eager.items()}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            rc, _ = _call(ccmi_lib, PAIRS, lat, par, sizes, 16, 2, stream=s, outs=outs)
    torch.cuda.synchronize()
    assert rc == 0  # the pairs form itself was captured: the stream had its buffer
    for _ in range(2):
        for v in outs.values():
            v.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        _same(outs, eager, "replay")


def test_first_call_inside_a_capture_takes_the_row_form(ccmi_lib, gpu):
    """No buffer may be allocated while the stream captures.  A batch whose packed weights need
    more than any earlier call of this process asked for finds no buffer of sufficient size: the
    pairs form is refused there, the default form runs the row form, and the replay is right."""
    import ccmi
    sizes = _sizes(*SHAPES["9x65"])
    batch = 400  # 400 x 864 floats of packed weights: far more than any other test's batch needs
    lat, par = _inputs(gpu, sizes, 16, 3, batch, seed=41)
    _, ref = _call(ccmi_lib, ROWS, lat, par, sizes, 16, 3)
    torch.cuda.synchronize()
    outs = {k: torch.full_like(v, FILL) for k, v in ref.items()}
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            rc2, _ = _call(ccmi_lib, PAIRS, lat, par, sizes, 16, 3, stream=s, outs=outs)
            msg = ccmi.last_error()
            rc0, _ = _call(ccmi_lib, 0, lat, par, sizes, 16, 3, stream=s, outs=outs)
    torch.cuda.synchronize()
    assert rc2 == ccmi.ERR_UNSUPPORTED and "captur" in msg
    assert rc0 == 0
    g.replay()
    torch.cuda.synchronize()
    _same(outs, ref, "replay of the captured row form")
    # outside a capture the same stream now gets its buffer, and the pairs form runs
    with torch.cuda.stream(s):
        rc, pairs = _call(ccmi_lib, PAIRS, lat, par, sizes, 16, 3, stream=s)
    torch.cuda.synchronize()
    assert rc == 0
    _same(pairs, ref, "after the capture")
