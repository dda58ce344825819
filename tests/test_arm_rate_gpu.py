"""The path-A ARM and rate (fwd_arm.hip, and the training step's rate form in train_arm.hip) against
the float64 reference of tests/arm_ref.py, on inputs that leave the rate and scale clamps
(tests/test_arm_ref.py asserts that on the reference): every (dim_arm, n_hidden) that
ccmi_arm_forward_f32 accepts, in the rows form, the pairs form and the default form, the drop-in
kernels ccmi_arm_context_f32 and ccmi_arm_mlp_f32, and the training form of the rate.

Every output stays within its a-priori per-latent bound and the total rate within its own (header
of tests/arm_ref.py); the bounds come from the reference, not from a kernel's outputs.

Worst error / bound on an MI355X (measured against the float64 reference; the bounds are not to be
tightened to these):
  kernel                                          mu     log_scale  scale  rate   total rate
  ccmi_arm_forward_f32_form, dim_arm 8  (3 forms)  0.313  0.407      0.336  0.464  0.081
                             dim_arm 16 (3 forms)  0.204  0.281      0.296  0.463  0.133
                             dim_arm 24 (rows)     0.119  0.256      0.196  0.474  0.185
                             dim_arm 32 (rows)     0.103  0.175      0.166  0.436  0.113
                             large q, rows, pairs  0.125  0.129      0.118  0.452  0.036
  ccmi_arm_mlp_f32                                 0.200  0.184      0.187
  training step's rate (train_arm.hip arm_rate)                                 0.474  0.027
  ccmi_arm_context_f32: equal to the oracle, element for element.
The rows, pairs and default forms give the same figures (the same bits), and so do quantize = 1
and 0.  The torch fp32 oracle reaches the same 0.474 per latent on the (24, 2) cases
(tests/test_arm_ref.py), as does the training form.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import arm_ref as R
import forward_oracle as fo

pytestmark = pytest.mark.gpu

ROWS, PAIRS = 1, 2
PAD = 3       # out_stride - latents of a frame
PPAD = 7      # param_stride - parameter count; the padding is NaN: reading it shows in the outputs
NAN = float("nan")


def _stack(frames, dev):
    """A batch from (case, ref) frames: latents [B, N], q [B, N] (float32), parameters [B, count + PPAD]."""
    lat = torch.stack([R.flat(c["lat"]) for c, _ in frames]).to(dev)
    q = torch.stack([R.flat(c["q"]).float() for c, _ in frames]).to(dev)
    par = torch.stack([R.pack_arm(c["arm"], PPAD) for c, _ in frames]).to(dev)
    return lat, q, par


def _arm_forward(lib, form, x, par, sizes, d, nh, quantize):
    """One ccmi_arm_forward_f32_form call into NaN-filled outputs of stride N + PAD."""
    import ccmi
    from ccmi import forward as F
    B, n = x.shape
    assert n == sum(h * w for h, w in sizes) and par.shape[1] == R.param_count(d, nh) + PPAD
    outs = {k: torch.full((B, n + PAD), NAN, device=x.device) for k in R.OUTS}
    h, w = F._grid_arrays(sizes)
    a = ccmi.ArmArgs(latent=ccmi.ptr(x), latent_stride=n, n_grids=len(sizes), h=h, w=w, gain=16.0, quantize=quantize,
                     dim_arm=d, n_hidden=nh, params=ccmi.ptr(par), param_stride=par.shape[1], mu=ccmi.ptr(outs["mu"]),
                     scale=ccmi.ptr(outs["scale"]), log_scale=ccmi.ptr(outs["log_scale"]), rate=ccmi.ptr(outs["rate"]),
                     out_stride=n + PAD, batch=B)
    rc = lib.ccmi_arm_forward_f32_form(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream, form)
    torch.cuda.synchronize()
    assert rc == 0, ccmi.last_error()
    for k, v in outs.items():
        assert bool(torch.isnan(v[:, n:]).all()), f"{k}: padding written"
        assert not bool(torch.isnan(v[:, :n]).any()), f"{k}: a latent not written (or NaN)"
    return {k: v[:, :n].cpu().numpy() for k, v in outs.items()}


def _check_batch(frames, got, what, worst):
    for b, (c, ref) in enumerate(frames):
        r = R.check(ref, {k: v[b] for k, v in got.items()}, f"{what} frame {c['regime']}")
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)


def _show(what, worst):
    print(f"\n{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


FORMS = [(ROWS, d, nh) for d, nh in R.ARMS] + [(f, d, nh) for f in (PAIRS, 0) for d, nh in R.ARMS if d in (8, 16)]
FORM_NAME = {ROWS: "rows", PAIRS: "pairs", 0: "default"}


@pytest.mark.parametrize("shape", list(R.SHAPES))
@pytest.mark.parametrize("form,d,nh", FORMS, ids=[f"{FORM_NAME[f]}-{d}-{nh}" for f, d, nh in FORMS])
def test_arm_forward_within_bounds(ccmi_lib, gpu, form, d, nh, shape):
    """Three frames (mid, low, high), own weights per frame, quantize = 1 on the latents and
    quantize = 0 on the integer grids."""
    frames = R.batch_case(d, nh, shape)
    lat, q, par = _stack(frames, gpu)
    sizes = R.sizes_of(shape)
    for quantize, x in ((1, lat), (0, q)):
        worst = {}
        got = _arm_forward(ccmi_lib, form, x, par, sizes, d, nh, quantize)
        _check_batch(frames, got, f"{FORM_NAME[form]} ({d}, {nh}) {shape} quantize {quantize}", worst)
        _show(f"arm_forward {FORM_NAME[form]} ({d}, {nh}) {shape} quantize {quantize}", worst)


def test_arm_forward_large_q(ccmi_lib, gpu):
    """|q| about 10^4: the pairs form's scaled ReLU holds activations times 2^-32, which is exact
    while no pre-activation exceeds 2^32."""
    c, ref = R.large_q_case()
    assert np.abs(ref["q"]).max() >= 5000 and ref["pre_max"] < 2.0 ** 32
    lat, q, par = _stack([(c, ref)], gpu)
    for form in (ROWS, PAIRS):
        for quantize, x in ((1, lat), (0, q)):
            worst = {}
            got = _arm_forward(ccmi_lib, form, x, par, c["sizes"], 16, 2, quantize)
            _check_batch([(c, ref)], got, f"large q {FORM_NAME[form]} quantize {quantize}", worst)
            _show(f"arm_forward large q {FORM_NAME[form]} quantize {quantize}", worst)


CTX_SHAPES = [(1, 1), (1, 70), (17, 1), (9, 65), (5, 51), (16, 16), (1, 257)]   # H * W = 255, 256, 257 among them


@pytest.mark.parametrize("hw", CTX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("d", [8, 16, 24, 32])
def test_arm_context_equals_oracle(ccmi_lib, gpu, d, hw):
    """ccmi_arm_context_f32 against forward_oracle.context, element for element, batch 2; the
    words behind the output stay untouched."""
    import ccmi
    H, W = hw
    g = torch.Generator().manual_seed(1000 * d + 10 * H + W)
    grid = torch.randint(-40, 41, (2, H, W), generator=g).float()
    n, tail = 2 * H * W * d, 64
    out = torch.full((n + tail,), NAN, device=gpu)
    dgrid = grid.to(gpu)
    rc = ccmi_lib.ccmi_arm_context_f32(ccmi.ptr(dgrid), 2, H, W, d, ccmi.ptr(out), ccmi.stream_handle(gpu))
    torch.cuda.synchronize()
    assert rc == 0, ccmi.last_error()
    assert bool(torch.isnan(out[n:]).all()), "written past the output"
    got = out[:n].cpu().view(2, H * W, d)
    for b in range(2):
        assert torch.equal(got[b], fo.context(grid[b], d)), (d, hw, b)


def _arm_mlp(lib, ctx, par, d, nh, want):
    """ccmi_arm_mlp_f32 with the outputs in `want`, NaN-filled with a tail behind them."""
    import ccmi
    m, tail = ctx.shape[0], 8
    outs = {k: torch.full((m + tail,), NAN, device=ctx.device) for k in want}
    rc = lib.ccmi_arm_mlp_f32(ccmi.ptr(ctx), m, d, nh, ccmi.ptr(par), ccmi.ptr(outs.get("mu")),
                              ccmi.ptr(outs.get("scale")), ccmi.ptr(outs.get("log_scale")),
                              ccmi.stream_handle(ctx.device))
    torch.cuda.synchronize()
    assert rc == 0, ccmi.last_error()
    for k, v in outs.items():
        assert bool(torch.isnan(v[m:]).all()), f"{k}: written past the output"
        assert not bool(torch.isnan(v[:m]).any()), f"{k}: a row not written (or NaN)"
    return {k: v[:m].cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("nh", R.MLP_HIDDEN)
@pytest.mark.parametrize("d", [8, 16, 24, 32])
def test_arm_mlp_within_bounds(ccmi_lib, gpu, d, nh):
    """ccmi_arm_mlp_f32 on the reference's contexts, M = 1, 255, 257 (one row, a row short of a
    workgroup, a row past one), mid / low / high frames, each output left out in turn."""
    worst = {}
    outs = ("mu", "scale", "log_scale")
    for m in R.MLP_GRIDS:
        for c, ref in R.mlp_case(d, nh, m):
            ctx = torch.from_numpy(ref["ctx"]).float().to(gpu)
            assert ctx.shape == (m, d)
            par = R.pack_arm(c["arm"], PPAD).to(gpu)
            full = _arm_mlp(ccmi_lib, ctx, par, d, nh, outs)
            for k, v in R.check(ref, full, f"mlp ({d}, {nh}) M={m} {c['regime']}").items():
                worst[k] = max(worst.get(k, 0.0), v)
            for skip in outs:
                part = _arm_mlp(ccmi_lib, ctx, par, d, nh, tuple(k for k in outs if k != skip))
                assert skip not in part
                for k, v in part.items():
                    assert np.array_equal(v, full[k]), (k, "without", skip)
    _show(f"arm_mlp ({d}, {nh})", worst)


@pytest.mark.parametrize("d,nh", R.TRAIN_ARMS)
def test_training_rate_form_within_bounds(ccmi_lib, gpu, d, nh):
    """The training step's rate (train_arm.hip arm_rate: expm1f, an IEEE division) through
    ccmi.autograd.TrainForward with the true_ste quantizer (forward: round) and no noise, on the
    mid and high frames at 37x130 with the smallest synthesis the step accepts: the same per-latent
    and total bounds as the eval form, so both forms meet one reference latent by latent."""
    from ccmi import train as T
    from ccmi.autograd import TrainForward
    (h, w), n_grids = R.SHAPES["37x130"]
    frames = [f for f in R.batch_case(d, nh, "37x130") if f[0]["regime"] in ("mid", "high")]
    assert len(frames) == 2
    arch = T.Arch(h, w, dim_arm=d, n_hidden=nh, layers=((1, 1, False, False), (3, 1, False, False)), n_grids=n_grids)
    assert arch.sizes == R.sizes_of("37x130")
    rest = T.init_params(arch)[R.param_count(d, nh):]
    par = torch.stack([torch.cat([R.pack_arm(c["arm"]), rest]) for c, _ in frames]).to(gpu)
    lat = torch.stack([R.flat(c["lat"]) for c, _ in frames]).to(gpu)
    raw, rate = TrainForward.apply(lat, par, {"arch": arch, "quantizer": "true_ste", "noise": None})
    torch.cuda.synchronize()
    assert raw.shape == (2, 3, h, w) and bool(torch.isfinite(raw).all())
    worst = {}
    _check_batch(frames, {"rate": rate.cpu().numpy()}, f"training rate ({d}, {nh})", worst)
    _show(f"training rate ({d}, {nh})", worst)
