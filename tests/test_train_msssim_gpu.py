"""ccmi_train_step_dist (train.hip + dist_msssim.hip): the overfit step with D = alpha MSE +
beta (1 - MS-SSIM) as its distortion, on 2 frames of 176 x 208 of the "hop" architecture of
tests/test_train_tiles_gpu.py, 4:4:4 (5 scales) and 4:2:0 (chroma 88 x 104: 4 scales).

The frames' targets are their own train-mode output plus 0.03 N(0, 1), so that every v_s is far from
the max (random networks against random images give v_s near 0).

  values     dist_out and loss_out[:, 1] of a forward_only call against the float64 restatement
             (tests/msssim_ref.py) on that call's raw_out: within msssim_ref.out_bound()
  loss       loss_out[:, 0] = D + lmbda rate / (H W), to 2 roundings of that expression
  gradients  grad_out of the _dist step against the grad_raw step fed the standalone call's gradient
             of raw_out; the bound is 4 x the largest entry-wise spread of three repeats of that
             grad_raw step (its float atomics), relative to each tensor's largest entry, floored at 2^-20
  unchanged  with dist = NULL, and through ccmi_train_step, rows and gradients stay within that spread

Measured on an MI355X: the spread of three grad_raw steps is 1.0e-7 .. 1.2e-7 of a tensor's largest
entry (three ccmi_train_step calls: 1.3e-7 .. 1.5e-7), so the bound is its floor 2^-20 = 9.5e-7; the
_dist step is off by 4.1e-8 (4:4:4) and 1.0e-7 (4:2:0), dist = NULL by 1.2e-7 .. 1.5e-7, its rows by
<= 7.9e-8; dist_out within 1.1e-5 (4:4:4, min v_s 0.72) and 1.6e-6 (4:2:0) of the restatement against
a bound of 8.8e-5, the MSE within 8.3e-11; 30 Adam steps take D from 0.97 .. 0.99 to 0.06 .. 0.13.
The file takes 4 s."""
import ctypes as C

import numpy as np
import pytest
import torch

import forward_oracle as fo
import msssim_ref as M
import train_oracle as to
import train_ref as R

pytestmark = pytest.mark.gpu

H, W, B = 176, 208, 2
FLOOR = 2.0 ** -20


def _frames(yuv420):
    """latents [B, N], params [B, P] of B random "hop" networks off the rate floor (as train_ref.frame)"""
    lats, prms = [], []
    for d in range(B):
        seed = 4000 + 10 * int(yuv420) + d
        mp = fo.ModelParams.random(H, W, seed=seed, dim_arm=16, n_hidden=2, layers=fo.parse_layers(R.HOP), n_grids=7)
        mp.arm[-1][1][1] += 4.0
        g = torch.Generator().manual_seed(1000 + seed)
        lat = [0.05 * torch.randn(h, w, generator=g) for h, w in mp.sizes]
        st = to.TrainState(mp, lat)
        lats.append(torch.cat([x.reshape(-1) for x in lat]))
        prms.append(torch.cat([x.detach().reshape(-1) for x in st.params()[mp.n_grids:]]).float())
    arch = dict(H=H, W=W, dim_arm=16, n_hidden=2, layers=tuple(fo.parse_layers(R.HOP)), n_grids=7, ups_k=8, pre_k=7)
    return arch, torch.stack(lats), torch.stack(prms)


def _case(yuv420):
    return M.Case("train", H, W, 4 if yuv420 else 5, layout="raw420" if yuv420 else "packed444", B=B, alpha=0.3, beta=0.7)


def _call(of, dist, noise, fn="dist", **kw):
    """one call with update = 0 on of's state: fields of ccmi_train_args by keyword (tensors -> pointers)"""
    from ccmi import train as T
    L = T._bind()
    a = of._args()
    a.quantizer, a.noise = T.Q_TYPES["softround"], T.NOISE_TYPES["kumaraswamy"]
    a.temperature, a.noise_param, a.lmbda = R.TEMP, R.NOISE_A, R.LMBDA
    a.step, a.seed, a.noise_in = 1, 0, noise.data_ptr()
    a.workspace, a.workspace_bytes = of.ws.data_ptr(), of.ws.numel()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    s = torch.cuda.current_stream().cuda_stream
    if fn == "plain":
        rc = L.ccmi_train_step(C.byref(a), s)
    else:
        rc = L.ccmi_train_step_dist(C.byref(a), None if dist is None else C.byref(dist), s)
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module", params=[False, True], ids=["444", "420"])
def setup(request, gpu):
    """the Overfitter, its noise, the forward's raw output and the targets made from it"""
    from ccmi import train as T
    from ccmi.metrics import Distortion
    yuv420 = request.param
    case = _case(yuv420)
    arch, lat, prm = _frames(yuv420)
    n = sum(h * w for h, w in case.sizes)
    D = Distortion(case.alpha, case.beta, n_scales=case.S)
    of = T.Overfitter(T.Arch(**arch), lat.to(gpu), prm.to(gpu), torch.zeros(B, n, device=gpu), yuv420=yuv420, distortion=D)
    g = torch.Generator().manual_seed(77)
    noise = to.kumaraswamy(torch.rand(B, of.N, generator=g), R.NOISE_A).float().to(gpu).contiguous()
    raw = torch.full((B, 3, H, W), float("nan"), device=gpu)
    assert _call(of, None, noise, forward_only=1, raw_out=raw) == 0
    assert bool(torch.isfinite(raw).all())
    rc = raw.cpu().reshape(B, -1)
    tg = torch.empty(B, n)
    o = 0
    for (h, w), (off, pitch, sub) in zip(case.sizes, case.planes):
        idx = M.plane_index(h, w, off, pitch, sub)
        tg[:, o:o + h * w] = (rc[:, idx].clamp(0, 1) + 0.03 * torch.randn(B, h * w, generator=g)).clamp(0.02, 0.98)
        o += h * w
    of.targets.copy_(tg.to(gpu))
    ref = M.reference(case, rc, tg)
    assert float(ref.v64.min()) > 0.5, ref.v64
    return dict(of=of, noise=noise, raw=raw, case=case, ref=ref, D=D, yuv420=yuv420, tg=tg)


def test_forward_only_values(setup):
    of, case, ref = setup["of"], setup["case"], setup["ref"]
    dist_out = torch.full((B, 4), float("nan"), device="cuda")
    loss = torch.full((B, 4), float("nan"), device="cuda")
    raw2 = torch.empty_like(setup["raw"])
    d = setup["D"].train_struct(setup["yuv420"], dist_out)
    assert _call(of, d, setup["noise"], forward_only=1, raw_out=raw2, loss_out=loss) == 0
    assert torch.equal(raw2, setup["raw"])
    eo = float((dist_out.cpu().double() - ref.out64).abs().max())
    em = float((loss[:, 1].cpu().double() - ref.out64[:, 2]).abs().max())
    print(f"\n{case.layout}: dist_out within {eo:.2e}, loss_out mse within {em:.2e} (bound {M.out_bound():.2e}); "
          f"D {dist_out[:, 0].tolist()} MS {dist_out[:, 1].tolist()} min v_s {float(dist_out[:, 3].min()):.3f}")
    assert eo <= M.out_bound() and em <= M.out_bound()
    assert float(loss[:, 3].abs().max()) == 0.0  # forward only: no gradient norm
    # loss = D + (lmbda / (H W)) rate, in float32: the product and the sum round once each (or fuse)
    lo, Dv, rate = (t.cpu().numpy() for t in (loss[:, 0], dist_out[:, 0], loss[:, 2]))
    lam = np.float32(np.float32(R.LMBDA) / np.float32(H * W))
    want = Dv.astype(np.float64) + np.float64(lam) * rate.astype(np.float64)
    assert np.all(np.abs(lo - want) <= 2 * 2.0 ** -24 * np.abs(want)), (lo, want)


def _tensors(of):
    """(name, slice) of the gradient row's tensors: each latent grid, then ARM, upsampling, synthesis"""
    from ccmi.quantize import Layout
    out, o = [], 0
    for i, (h, w) in enumerate(of.arch.sizes):
        out.append((f"latent {i}", slice(o, o + h * w)))
        o += h * w
    lay = Layout.of(of.arch)
    u0 = int(lay.ups_w[0])
    out += [("arm", slice(o, o + u0)), ("upsampling", slice(o + u0, o + lay.syn_off)), ("synthesis", slice(o + lay.syn_off, o + lay.P))]
    return out


def _rel(a, b, ref, tensors):
    """largest |a - b| per tensor over the tensor's largest |ref|"""
    return max(float((a[:, s] - b[:, s]).abs().max() / ref[:, s].abs().max()) for _, s in tensors)


def test_gradients_against_the_grad_raw_step(setup):
    from ccmi import metrics
    of, case = setup["of"], setup["case"]
    tensors = _tensors(of)
    assert tensors[-1][1].stop == of.N + of.P
    # the standalone call's gradient of raw_out, [B, 3, H, W] with 0 at the positions that are no sample
    tgt = of.targets
    _, graw = metrics.distortion(setup["raw"], tgt, setup["D"], yuv420=setup["yuv420"], grad=True)
    reps = []
    for _ in range(3):
        G = torch.full((B, of.N + of.P), float("nan"), device="cuda")
        assert _call(of, None, setup["noise"], grad_out=G, grad_raw=graw) == 0
        reps.append(G.double())
    st = torch.stack(reps)
    spread = _rel(st.max(0).values, st.min(0).values, reps[0], tensors)
    bound = max(4 * spread, FLOOR)
    G1 = torch.full((B, of.N + of.P), float("nan"), device="cuda")
    loss = torch.full((B, 4), float("nan"), device="cuda")
    d = setup["D"].train_struct(setup["yuv420"])
    assert _call(of, d, setup["noise"], grad_out=G1, loss_out=loss) == 0
    assert bool(torch.isfinite(G1).all()) and bool(torch.isfinite(loss).all())
    err = _rel(G1.double(), reps[0], reps[0], tensors)
    print(f"\n{case.layout}: spread of three grad_raw steps {spread:.2e}, bound {bound:.2e}, _dist step off by {err:.2e}; "
          f"largest entry {float(reps[0].abs().max()):.2e}")
    assert float(reps[0].abs().max()) > 0
    assert err <= bound
    # the row of the update = 0 step: D + lmbda rate / (H W) and the MSE of the forward_only call
    assert float((loss[:, 1].cpu().double() - setup["ref"].out64[:, 2]).abs().max()) <= M.out_bound()
    assert float((loss[:, 0].cpu().double() - setup["ref"].out64[:, 0]
                  - R.LMBDA / (H * W) * loss[:, 2].cpu().double()).abs().max()) <= M.out_bound()
    setup["spread"] = bound


def test_without_a_distortion_nothing_changes(setup):
    """dist = NULL and ccmi_train_step: the built-in MSE path, rows and gradients within the spread"""
    of = setup["of"]
    tensors = _tensors(of)
    runs = []
    for fn in ("plain", "plain", "plain", "dist"):
        G = torch.full((B, of.N + of.P), float("nan"), device="cuda")
        loss = torch.full((B, 4), float("nan"), device="cuda")
        assert _call(of, None, setup["noise"], fn=fn, grad_out=G, loss_out=loss) == 0
        runs.append((G.double(), loss.double()))
    st = torch.stack([g for g, _ in runs[:3]])
    spread = _rel(st.max(0).values, st.min(0).values, runs[0][0], tensors)
    bound = max(4 * spread, FLOOR)
    err = _rel(runs[3][0], runs[0][0], runs[0][0], tensors)
    lerr = float(((runs[3][1] - runs[0][1]).abs() / runs[0][1].abs()).max())
    print(f"\n{setup['case'].layout}: spread of three ccmi_train_step calls {spread:.2e}, dist = NULL off by {err:.2e}, rows by {lerr:.2e}")
    assert err <= bound and lerr <= bound
    # the built-in MSE of the row is the stage's MSE of the same forward
    assert float((runs[0][1][:, 1].cpu() - setup["ref"].out64[:, 2]).abs().max()) <= M.out_bound()


def test_dist_with_grad_raw_is_refused(setup):
    import ccmi
    of = setup["of"]
    d = setup["D"].train_struct(setup["yuv420"])
    assert _call(of, d, setup["noise"], grad_raw=setup["raw"]) == ccmi.ERR_ARG
    assert "grad_raw" in ccmi.last_error()


@pytest.mark.parametrize("yuv420", [False, True], ids=["444", "420"])
def test_thirty_adam_steps_lower_the_distortion(yuv420, gpu):
    from ccmi import train as T
    from ccmi.metrics import Distortion
    case = _case(yuv420)
    g = torch.Generator().manual_seed(5)
    tg = torch.stack([torch.cat([M._plane(h, w, g).reshape(-1) for h, w in case.sizes]) for _ in range(B)]).float().to(gpu)
    arch = T.Arch(H, W)
    prm = torch.stack([T.init_params(arch, g) for _ in range(B)]).to(gpu)
    D = Distortion(0.0, 1.0, n_scales=case.S)
    of = T.Overfitter(arch, torch.zeros(B, arch.n_latents, device=gpu), prm, tg, yuv420=yuv420, distortion=D)
    first = of.validate(0.0).clone()
    d0 = of.dist.clone()
    for _ in range(30):
        of.step(lmbda=0.0)
    last = of.validate(0.0).clone()
    torch.cuda.synchronize()
    print(f"\n{case.layout}: D {d0[:, 0].tolist()} -> {of.dist[:, 0].tolist()}, MS {d0[:, 1].tolist()} -> {of.dist[:, 1].tolist()}")
    assert bool(torch.isfinite(last).all())
    assert bool((of.dist[:, 0] < d0[:, 0]).all()) and bool((last[:, 0] < first[:, 0]).all())
    assert torch.equal(last[:, 0], of.dist[:, 0])  # lmbda = 0: the loss is D


def test_quantize_model_scores_with_the_distortion(gpu, monkeypatch):
    """every loss of the returned table is metrics.distortion of that candidate plus the rate term:
    the rows the search hands to metrics.distortion are recorded and the chosen ones re-scored by the
    float64 restatement"""
    from ccmi import metrics, quantize
    from ccmi import train as T
    h, w, S, lmbda = 64, 96, 2, 1e-3
    case = M.Case("q", h, w, S, layout="packed420", alpha=0.3, beta=0.7)
    D = metrics.Distortion(case.alpha, case.beta, n_scales=S)
    arch = T.Arch(h, w)
    g = torch.Generator().manual_seed(9)
    tg = torch.cat([M._plane(hh, ww, g).reshape(-1) for hh, ww in case.sizes]).float().to(gpu)
    prm = T.init_params(arch, g).to(gpu)
    lat = (0.3 * torch.randn(arch.n_latents, generator=g)).to(gpu)
    seen = []
    real = metrics.distortion

    def spy(x, y, dist, **kw):
        r = real(x, y, dist, **kw)
        seen.append((x.cpu(), r.cpu()))
        return r

    monkeypatch.setattr(metrics, "distortion", spy)
    qm = quantize.quantize_model(arch, lat, prm, tg, lmbda, yuv420=True, distortion=D)
    assert seen and all(r.shape[1] == 4 for _, r in seen)
    rows = torch.cat([x for x, _ in seen])
    vals = torch.cat([r[:, 0] for _, r in seen]).double()
    n_syn, n_ups = len(qm.table["synthesis"]), len(qm.table["upsampling"])
    assert rows.shape[0] == n_syn + n_ups
    # the upsampling search is the last one: its chosen candidate is the model returned
    k = int(np.argmin([v for _, _, v in qm.table["upsampling"]]))
    assert abs(qm.table["upsampling"][k][2] - qm.loss) == 0
    got = float(vals[n_syn + k])
    assert abs(qm.loss - (got + lmbda * qm.nn_bits["upsampling"] / (h * w))) <= 1e-12
    ref = M.reference(case, rows[n_syn + k][None], tg.cpu()[None])
    assert abs(got - float(ref.out64[0, 0])) <= M.out_bound()
    # and the MSE-scored search is untouched by the option
    calls = len(seen)
    qm0 = quantize.quantize_model(arch, lat, prm, tg, lmbda, yuv420=True)
    assert len(seen) == calls and set(qm0.table) == set(qm.table)
