"""The path-A ARM's tile staging and stores (fwd_arm.hip: arm_tile_of, arm_stage_tile, arm_emit;
rows of the tile read through per-row buffer descriptors, outputs stored at a wave-uniform base plus
a 32-bit offset), on frames chosen for where the tile geometry goes wrong rather than for size:

  1x1      a tile wider and taller than the image, every grid
  3x5      the same with more than one latent; the second load of a row is wholly outside
  9x65     one row and one column past a tile: the second load cut by the image edge after 5 columns
  12x137   2 x 3 tiles: halos from the tile above and beside, second load cut after 9 - 4 columns
  17x200   3 x 4 tiles with an interior one, last tile 1 row x 8 columns

each with 7 grids (down to 1 x 1 .. 1 x 4), so a launch mixes all of the above.

Staging is checked bit for bit without the library on the other side: with n_hidden = 0, a batch of
dim_arm frames over one latent vector, frame i's mu row one-hot at i and everything else 0, mu of
frame i is the quantised latent at context offset i, zero outside the image; the expectation is
built here from the reference's offset table (forward_oracle.CTX_INDEX, arm.py:373-506).  The full
network is checked against the float64 reference of tests/arm_ref.py with its a-priori bounds.

Worst error / bound on an MI355X over all cases of test_full_network_within_bounds (the bounds are
not to be tightened to these):
  mu 0.279   log_scale 0.444   scale 0.325   rate 0.483   total rate 0.149
"""
import ctypes as C

import pytest
import torch

import arm_ref as R
import forward_oracle as fo

pytestmark = pytest.mark.gpu

ROWS, PAIRS = 1, 2
FORM_NAME = {ROWS: "rows", PAIRS: "pairs"}
FORMS = [(PAIRS, 8), (PAIRS, 16), (ROWS, 16), (ROWS, 24)]
FRAMES = [(1, 1), (3, 5), (9, 65), (12, 137), (17, 200)]
GRIDS = 7
FILL = -7.5    # no output of these tests is a half-integer
PAD = 3       # out_stride - latents of a frame, where a test does not choose its own
GAIN = 16.0

form_ids = [f"{FORM_NAME[f]}-{d}" for f, d in FORMS]
frame_ids = [f"{h}x{w}" for h, w in FRAMES]


def _sizes(hw, n=GRIDS):
    h, w = hw
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def _call(lib, form, lat, par, sizes, d, nh, quantize=1, want=R.OUTS, batch=None, lat_stride=None, par_stride=None,
          out_stride=None, alloc=None):
    """One ccmi_arm_forward_f32_form call into FILL-filled outputs [batch, out_stride] (or of the
    shape `alloc`, for a call that must be refused): (rc, outputs)."""
    import ccmi
    from ccmi import forward as F
    n = sum(h * w for h, w in sizes)
    batch = lat.shape[0] if batch is None else batch
    out_stride = n + PAD if out_stride is None else out_stride
    outs = {k: torch.full(alloc or (batch, out_stride), FILL, device=lat.device) for k in want}
    h, w = F._grid_arrays(sizes)
    a = ccmi.ArmArgs(latent=ccmi.ptr(lat), latent_stride=lat.shape[1] if lat_stride is None else lat_stride,
                     n_grids=len(sizes), h=h, w=w, gain=GAIN, quantize=quantize, dim_arm=d, n_hidden=nh,
                     params=ccmi.ptr(par), param_stride=par.shape[1] if par_stride is None else par_stride,
                     mu=ccmi.ptr(outs.get("mu")), scale=ccmi.ptr(outs.get("scale")),
                     log_scale=ccmi.ptr(outs.get("log_scale")), rate=ccmi.ptr(outs.get("rate")),
                     out_stride=out_stride, batch=batch)
    rc = lib.ccmi_arm_forward_f32_form(C.byref(a), torch.cuda.current_stream(lat.device).cuda_stream, form)
    torch.cuda.synchronize()
    return rc, outs


def _written(outs, n):
    for k, v in outs.items():
        assert bool((v[:, n:] == FILL).all()), f"{k}: written outside the frame's latents"
        assert bool((v[:, :n] != FILL).all()), f"{k}: a latent not written"


# ----------------------------------------------------------------------------- staging, bitwise


@pytest.mark.parametrize("hw", FRAMES, ids=frame_ids)
@pytest.mark.parametrize("form,d", FORMS, ids=form_ids)
def test_staging_is_the_shifted_latent(ccmi_lib, gpu, form, d, hw):
    sizes = _sizes(hw)
    n = sum(h * w for h, w in sizes)
    g = torch.Generator().manual_seed(1000 * hw[0] + hw[1])
    q = [torch.randint(-90, 91, s, generator=g).double() for s in sizes]           # no zeros needed: the pad is 0
    q = [x + (x == 0) * 7 for x in q]                                              # ... and a latent never is
    lat = torch.cat([((x + 0.6 * (torch.rand(x.shape, generator=g, dtype=torch.float64) - 0.5)) / GAIN).float().reshape(-1)
                     for x in q])
    assert torch.equal(torch.round(GAIN * lat).double(), torch.cat([x.reshape(-1) for x in q]))
    # frame i: W_out[0] one-hot at i, W_out[1] = 0, b_out = 0
    par = torch.zeros(d, 2 * d + 2)
    par[torch.arange(d), torch.arange(d)] = 1.0
    want = torch.zeros(d, n)
    for i, k in enumerate(fo.CTX_INDEX[d]):
        dy, dx = k // 9 - 4, k % 9 - 4
        cols = []
        for x in q:
            H, W = x.shape
            s = torch.zeros(H, W, dtype=torch.float64)
            ys, xs = slice(max(0, -dy), H), slice(max(0, -dx), min(W, W - dx))
            yd, xd = slice(max(0, -dy) + dy, H + dy), slice(max(0, -dx) + dx, min(W, W - dx) + dx)
            if ys.start < ys.stop and xs.start < xs.stop:
                s[ys, xs] = x[yd, xd]
            cols.append(s.reshape(-1))
        want[i] = torch.cat(cols).float()
    for quantize, x in ((1, lat), (0, torch.round(GAIN * lat))):
        rc, outs = _call(ccmi_lib, form, x.to(gpu)[None], par.to(gpu), sizes, d, 0, quantize, want=("mu", "log_scale"),
                         batch=d, lat_stride=0)
        assert rc == 0
        _written(outs, n)
        assert torch.equal(outs["mu"][:, :n].cpu(), want), (quantize, int((outs["mu"][:, :n].cpu() != want).sum()))
        assert bool((outs["log_scale"][:, :n] == 0).all())


# ----------------------------------------------------------------------------- full network


WORST = {}


@pytest.mark.parametrize("nh", [0, 2])
@pytest.mark.parametrize("hw", FRAMES, ids=frame_ids)
@pytest.mark.parametrize("form,d", FORMS, ids=form_ids)
def test_full_network_within_bounds(ccmi_lib, gpu, form, d, hw, nh):
    """Batch 3 (the mid, low and high regimes of tests/arm_ref.py), own latents and weights per
    frame, all four outputs, quantize 1 on the latents and 0 on the integer grids."""
    sizes = _sizes(hw)
    n = sum(h * w for h, w in sizes)
    frames = []
    for k, regime in enumerate(R.FRAMES):
        c = R.make_case(d, nh, sizes, 7000000 + 10000 * hw[0] + 10 * hw[1] + 1000000 * k + 100 * d + nh, regime)
        frames.append((c, R.reference(c["q"], c["arm"], d)))
    lat = torch.stack([R.flat(c["lat"]) for c, _ in frames]).to(gpu)
    q = torch.stack([R.flat(c["q"]).float() for c, _ in frames]).to(gpu)
    par = torch.stack([R.pack_arm(c["arm"], 7) for c, _ in frames]).to(gpu)   # NaN behind the parameters
    for quantize, x in ((1, lat), (0, q)):
        rc, outs = _call(ccmi_lib, form, x, par, sizes, d, nh, quantize)
        assert rc == 0
        _written(outs, n)
        for b, (c, ref) in enumerate(frames):
            r = R.check(ref, {k: v[b, :n].cpu().numpy() for k, v in outs.items()},
                        f"{FORM_NAME[form]} ({d}, {nh}) {hw} quantize {quantize} frame {c['regime']}")
            for k, v in r.items():
                WORST[k] = max(WORST.get(k, 0.0), v)
    print("\nworst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


# ----------------------------------------------------------------------------- strides, untouched memory


def _inputs(dev, sizes, d, nh, batch, seed, lat_pad=0):
    g = torch.Generator().manual_seed(seed)
    n = sum(h * w for h, w in sizes)
    lat = 0.4 * torch.randn(batch, n + lat_pad, generator=g)
    par = torch.randn(batch, nh * (d * d + d) + 2 * d + 2 + 5, generator=g) * (0.5 / d ** 0.5)
    return lat.to(dev), par.to(dev)


@pytest.mark.parametrize("only", R.OUTS)
@pytest.mark.parametrize("form,d", FORMS, ids=form_ids)
def test_strides_and_untouched_memory(ccmi_lib, gpu, form, d, only):
    """Each output requested on its own, with out_stride and latent_stride larger than the frame,
    latent_stride 0 and param_stride 0: what lies outside the n latents of a frame keeps its
    sentinel, and the values are those of the call with all four outputs."""
    sizes = _sizes((12, 137))
    n = sum(h * w for h, w in sizes)
    lat, par = _inputs(gpu, sizes, d, 2, 3, seed=500 + d, lat_pad=11)
    rc, full = _call(ccmi_lib, form, lat, par, sizes, d, 2, out_stride=n + 129)
    assert rc == 0
    _written(full, n)
    for kw in (dict(), dict(lat_stride=0), dict(par_stride=0), dict(lat_stride=0, par_stride=0)):
        rc, one = _call(ccmi_lib, form, lat, par, sizes, d, 2, want=(only,), batch=3, out_stride=n + 129, **kw)
        assert rc == 0 and list(one) == [only]
        _written(one, n)
        if not kw:
            assert torch.equal(one[only], full[only])
        if kw == dict(lat_stride=0, par_stride=0):  # everything shared: the frames agree, and with frame 0 above
            assert torch.equal(one[only][1], one[only][0]) and torch.equal(one[only][2], full[only][0])


# ----------------------------------------------------------------------------- refusals


@pytest.mark.parametrize("form,d", FORMS, ids=form_ids)
def test_out_of_range_launches_are_refused(ccmi_lib, gpu, form, d):
    """2^31 tiles or more (the tile lookup's constants are exact for 31-bit tile ids) and a frame
    of more than 2^30 latents (the stores' 32-bit byte offsets): CCMI_ERR_ARG, nothing launched."""
    import ccmi
    sizes = _sizes((9, 65), 3)
    lat, par = _inputs(gpu, sizes, d, 2, 1, seed=9)
    tiles = sum(-(-w // 64) * -(-h // 8) for h, w in sizes)
    rc, outs = _call(ccmi_lib, form, lat, par, sizes, d, 2, batch=(2 ** 31 - 1) // tiles + 1, lat_stride=0, par_stride=0,
                     alloc=(1, 4096))
    assert rc == ccmi.ERR_ARG and "tiles" in ccmi.last_error()
    assert all(bool((v == FILL).all()) for v in outs.values())
    rc, outs = _call(ccmi_lib, form, lat, par, sizes, d, 2, batch=(2 ** 31 - 1) // tiles, lat_stride=0, par_stride=0,
                     out_stride=1, alloc=(1, 4096))   # the largest batch passes that check (and fails the next)
    assert rc == ccmi.ERR_ARG and "stride" in ccmi.last_error()
    big = [(32768, 32768), (1, 1)]
    rc, outs = _call(ccmi_lib, form, lat, par, big, d, 2, batch=1, lat_stride=0, par_stride=0, out_stride=2 ** 30 + 8,
                     alloc=(1, 4096))
    assert rc == ccmi.ERR_ARG and "2^30" in ccmi.last_error()
    assert all(bool((v == FILL).all()) for v in outs.values())
