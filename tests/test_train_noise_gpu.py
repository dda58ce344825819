"""The quantisation noise that the training step draws inside t_quant (csrc/train.hip), draw by
draw against the float64 restatement of the same counter (tests/noise_ref.py, pinned on the CPU by
tests/test_noise_ref.py).  No statistics are asserted on device output.

The generator is observed through ccmi_train_step with forward_only = 1 and a network that hands
grid 0's y_hat through unchanged: two grids, ARM (8, 0) with zero weights, zero upsampling and refine
half kernels (refine is filter(x) + x), synthesis 16-1-linear-relu|3-1-linear-none with hidden unit
0 = +channel 0, unit 1 = -channel 0, output 0 = h0 - h1.  relu(y) - relu(-y) = y and every other
product is 0 x finite, so with zero latents and quantizer "none" raw_out[b, 0] is the noise of grid
0, bit for bit (test_observation_is_exact, with a handed-in tensor).  Frame 37 x 58 (2146 latents in
grid 0, not a multiple of the 256-thread block), batch 3.  The coarser grids' draws (i >= H W) are
covered by test_in_kernel_draw_feeds_the_step_as_the_tensor_does.

Bounds (derived in the header of tests/noise_ref.py, not from these figures): Kumaraswamy
|CDF(n) - u1| <= K(a) 2^-24 with K = 10.7, 16.6, 26.6 for a = 1, 1.5, 2; Gaussian
|n - reference| <= sigma 15 2^-24 (R + 1).

Worst error / bound on an MI355X, over the six counters of each case (seeds 0, 1, 2^63 + 5 at
step 1; steps 2, 10600, 2^23 + 3 at seed 0):
  case                  worst   per counter
  kumaraswamy a = 1     0.141   0.094 0.141 0.141 0.141 0.141 0.141   (1.5 of the 10.7 lattice steps)
  kumaraswamy a = 1.5   0.169   0.159 0.167 0.163 0.159 0.165 0.169   (2.8 of 16.6)
  kumaraswamy a = 2     0.095   0.093 0.095 0.088 0.087 0.091 0.087   (2.5 of 26.6)
  gaussian sigma = .25  0.128   0.110 0.124 0.117 0.110 0.127 0.128
  gaussian sigma = .1   0.146   0.126 0.143 0.119 0.130 0.146 0.143
The bounds are not to be tightened to these.  With b computed without its / a in a scratch copy of
the reference the first counter of a = 1.5 fails at 1.1e5 times the bound (a = 1 cannot tell: b is
1 either way); with u2 taken from r, the first counter of sigma = 0.25 at 1.7e6 times.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import noise_ref as R

pytestmark = pytest.mark.gpu

H, W, B = 37, 58, 3
H1, W1 = (H + 1) // 2, (W + 1) // 2
N0, N = H * W, H * W + H1 * W1
LAYERS = ((16, 1, False, True), (3, 1, False, False))
COUNTERS = [(0, 1), (1, 1), (2 ** 63 + 5, 1), (0, 2), (0, 10600), (0, 2 ** 23 + 3)]      # (seed, step)
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _uniforms(seed, step, batch, n):
    """(u1, u2) [batch, n] of the reference at (seed, step), read-only."""
    u1, u2 = R.draw_uniforms(seed, step, np.arange(batch)[:, None], np.arange(n)[None, :])
    u1.setflags(write=False)
    u2.setflags(write=False)
    return u1, u2


def _ref_noise(ntype, param, seed, step, batch, n):
    u1, u2 = _uniforms(seed, step, batch, n)
    x = R.kumaraswamy(u1, param) if ntype == "kumaraswamy" else R.gaussian(u1, u2, param)
    return torch.from_numpy(x.astype(np.float32))


def _observer(dev):
    """(arch, params [B, P]) of the observing network."""
    from ccmi import train as T
    arch = T.Arch(H, W, dim_arm=8, n_hidden=0, layers=LAYERS, n_grids=2)
    w0, w1 = torch.zeros(16, 2, 1, 1), torch.zeros(3, 16, 1, 1)
    w0[0, 0], w0[1, 0] = 1.0, -1.0
    w1[0, 0], w1[0, 1] = 1.0, -1.0
    p = T.pack_params([(torch.zeros(2, 8), torch.zeros(2))], [torch.zeros(4)], [torch.zeros(4)],
                      [(w0, torch.zeros(16)), (w1, torch.zeros(3))])
    return arch, p.repeat(B, 1).to(dev)


def _observe(dev, ntype, param, seed, step, stride=N, noise_in=None):
    """One forward-only ccmi_train_step on zero latents of the given stride: raw_out [B, 3, H W]
    as numpy float32."""
    import ccmi
    from ccmi import autograd as A, train as T
    L = T._bind()
    arch, prm = _observer(dev)
    lat = torch.zeros(B, stride, device=dev)
    a = A._args(arch, lat, prm, False)
    assert L.ccmi_train_param_count(C.byref(a)) == prm.shape[1]
    dummy = torch.zeros(1, device=dev)
    raw = torch.full((B, 3, N0), NAN, device=dev)
    rate = torch.full((B, N), NAN, device=dev)
    a.target, a.target_stride = dummy.data_ptr(), 0
    a.quantizer, a.noise = T.Q_TYPES["none"], T.NOISE_TYPES[ntype]
    a.temperature, a.noise_param = 0.3, float(param)
    a.seed, a.step, a.update = seed, step, 0
    a.noise_in = None if noise_in is None else noise_in.data_ptr()
    a.forward_only, a.raw_out, a.rate_out = 1, raw.data_ptr(), rate.data_ptr()
    ws = torch.empty(L.ccmi_train_workspace_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    rc = L.ccmi_train_step(C.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, ccmi.last_error()
    out = raw.cpu().numpy()
    assert not np.isnan(out).any(), "raw_out: a pixel not written (or NaN)"
    return out


def _same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


def _check_kumaraswamy(raw, a, seed, step):
    """Worst |CDF(n) - u1| / tol_u of one call; asserts the bound and the support."""
    n = raw[:, 0].astype(np.float64)
    assert np.all(raw[:, 1:] == 0.0)
    assert np.all((n >= -0.5) & (n <= 0.5)), (n.min(), n.max())
    u1 = _uniforms(seed, step, B, N)[0][:, :N0]
    err = np.abs(R.kumaraswamy_cdf(n, a) - u1) / R.kumaraswamy_tol_u(a)
    assert err.max() <= 1.0, (a, seed, step, np.unravel_index(err.argmax(), err.shape), float(err.max()))
    return float(err.max())


def _check_gaussian(raw, sigma, seed, step):
    n = raw[:, 0].astype(np.float64)
    assert np.all(raw[:, 1:] == 0.0)
    u1, u2 = (u[:, :N0] for u in _uniforms(seed, step, B, N))
    err = np.abs(n - R.gaussian(u1, u2, sigma)) / R.gaussian_tol(u1, sigma)
    assert err.max() <= 1.0, (sigma, seed, step, np.unravel_index(err.argmax(), err.shape), float(err.max()))
    return float(err.max())


def test_observation_is_exact(ccmi_lib, gpu):
    """The control: a handed-in tensor comes out of raw_out[:, 0] bit for bit, through a latent
    buffer wider than N (noise_in shares its stride)."""
    g = torch.Generator().manual_seed(0)
    for stride in (N, N + 5):
        noise = (torch.rand(B, stride, generator=g) - 0.5).clamp(-0.4999, 0.4999)
        raw = _observe(gpu, "none", 1.0, 0, 1, stride=stride, noise_in=noise.to(gpu))
        assert _same_bits(raw[:, 0], noise[:, :N0].numpy())
        assert np.all(raw[:, 1:] == 0.0)


@pytest.mark.parametrize("a", [1.0, 1.5, 2.0])
def test_kumaraswamy_draws(ccmi_lib, gpu, a):
    worst = [_check_kumaraswamy(_observe(gpu, "kumaraswamy", a, seed, step), a, seed, step) for seed, step in COUNTERS]
    print(f"\nkumaraswamy a = {a}: worst error / bound {max(worst):.3f} ({', '.join(f'{w:.3f}' for w in worst)})")


@pytest.mark.parametrize("sigma", [0.25, 0.1])
def test_gaussian_draws(ccmi_lib, gpu, sigma):
    worst = [_check_gaussian(_observe(gpu, "gaussian", sigma, seed, step), sigma, seed, step) for seed, step in COUNTERS]
    print(f"\ngaussian sigma = {sigma}: worst error / bound {max(worst):.3f} ({', '.join(f'{w:.3f}' for w in worst)})")


@pytest.mark.parametrize("ntype,param", [("kumaraswamy", 2.0), ("gaussian", 0.25)])
def test_keyed_by_index_not_by_address(ccmi_lib, gpu, ntype, param):
    ref = _observe(gpu, ntype, param, 1, 2)
    assert _same_bits(_observe(gpu, ntype, param, 1, 2, stride=N + 5), ref)


@pytest.mark.parametrize("ntype,param", [("kumaraswamy", 2.0), ("gaussian", 0.25)])
def test_a_function_of_its_key(ccmi_lib, gpu, ntype, param):
    first = _observe(gpu, ntype, param, 2 ** 63 + 5, 10600)
    assert _same_bits(_observe(gpu, ntype, param, 2 ** 63 + 5, 10600), first)
    assert not _same_bits(_observe(gpu, ntype, param, 2 ** 63 + 5, 10601), first)
    assert not _same_bits(_observe(gpu, ntype, param, 2 ** 63 + 4, 10600), first)


@pytest.mark.parametrize("top", [True, False], ids=["u1=1", "u1=2^-25"])
def test_edges_on_the_device(ccmi_lib, gpu, top):
    """r >> 40 = 2^24 - 1 (u1 = 1.0) and r >> 40 = 0 (u1 = 2^-25) placed at one latent of frame 1,
    step 3, by the seed: finite, Kumaraswamy inside its support, both within their bounds."""
    step, b, i = 3, 1, 1234
    r = ((2 ** 24 - 1) << 40 | 0x5A5A5A5A5A) if top else 0x0F1E2D3C4B
    seed = int(R.seed_for(r, step, b, i))
    u1 = _uniforms(seed, step, B, N)[0]
    assert u1[b, i] == (1.0 if top else 2.0 ** -25)
    for a in (1.0, 1.5, 2.0):
        raw = _observe(gpu, "kumaraswamy", a, seed, step)
        _check_kumaraswamy(raw, a, seed, step)
        v = float(raw[b, 0, i])
        assert np.isfinite(v) and -0.5 <= v <= 0.5
    for sigma in (0.25, 0.1):
        raw = _observe(gpu, "gaussian", sigma, seed, step)
        _check_gaussian(raw, sigma, seed, step)
        v = float(raw[b, 0, i])
        assert np.isfinite(v) and abs(v) <= 5.9 * sigma


# ----------------------------------------------------------------------------- the whole step
def _random_state(dev, batch=2):
    """A random default-architecture network and latents per frame at 37 x 58 (the set-up of
    test_train_gpu.py::_random_arch_vs_oracle): arch, latents, params, target, and the (name, size)
    of every tensor of a gradient row."""
    import forward_oracle as fo
    from ccmi import train as T
    lats, prms, tgts = [], [], []
    for f in range(batch):
        mp = fo.ModelParams.random(H, W, seed=40 + f)
        g = torch.Generator().manual_seed(1040 + f)
        lats.append(torch.cat([0.05 * torch.randn(h * w, generator=g) for h, w in mp.sizes]))
        prms.append(T.pack_params(mp.arm, mp.ups_half, mp.pre_half, mp.syn))
        tgts.append(torch.rand(3 * H * W, generator=g))
    arch = T.Arch(H, W, dim_arm=mp.dim_arm, n_hidden=mp.n_hidden, layers=tuple(mp.layers), n_grids=mp.n_grids)
    names = [(f"latent_grids.{k}", h * w) for k, (h, w) in enumerate(mp.sizes)]
    names += [(f"arm.{k}.{n}", t.numel()) for k, wb in enumerate(mp.arm) for n, t in zip("wb", wb)]
    names += [(f"ups.{k}", t.numel()) for k, t in enumerate(mp.ups_half)]
    names += [(f"pre.{k}", t.numel()) for k, t in enumerate(mp.pre_half)]
    names += [(f"syn.{k}.{n}", t.numel()) for k, wb in enumerate(mp.syn) for n, t in zip("wb", wb)]
    return arch, torch.stack(lats).to(dev), torch.stack(prms).to(dev), torch.stack(tgts).to(dev), names


def _overfitter(state, seed):
    from ccmi import train as T
    arch, lat, prm, tgt, _ = state
    return T.Overfitter(arch, lat.clone(), prm.clone(), tgt.clone(), yuv420=False, seed=seed)


@pytest.mark.parametrize("qtype,ntype,param", [("softround", "kumaraswamy", 2.0), ("softround", "gaussian", 0.25),
                                               ("none", "kumaraswamy", 1.0)])
def test_in_kernel_draw_feeds_the_step_as_the_tensor_does(ccmi_lib, gpu, qtype, ntype, param):
    """Loss, rate and every gradient of one step with the in-kernel noise (seed 7, step 1) against
    the same step given the reference's draws as a tensor: every grid carries noise, so this covers
    the draws at i >= H W too."""
    from test_train_gpu import _grad_close
    state = _random_state(gpu)
    names = state[4]
    out = []
    for noise in (None, _ref_noise(ntype, param, 7, 1, 2, state[0].n_latents).to(gpu)):
        of = _overfitter(state, 7)
        assert (of.N + of.P) == sum(n for _, n in names)
        g = torch.zeros(2, of.N + of.P, device=gpu)
        loss = of.step(qtype, ntype, 0.3, param, 1e-3, update=False, noise=noise, grad_out=g)
        torch.cuda.synchronize()
        out.append((loss.cpu().numpy().astype(np.float64), g.cpu().numpy()))
    (l_got, g_got), (l_ref, g_ref) = out
    assert np.all(np.isfinite(l_ref)) and np.all(l_ref[:, 2] > 0)
    for col in (0, 2):                                                  # loss, rate
        assert np.all(np.abs(l_got[:, col] - l_ref[:, col]) <= 1e-5 * np.abs(l_ref[:, col])), (col, l_got, l_ref)
    for b in range(2):
        o = 0
        for name, n in names:
            _grad_close(g_got[b, o:o + n], g_ref[b, o:o + n], f"frame {b} {name}")
            o += n


def _fresh_state(dev, batch=2):
    """Where every overfit starts: a freshly constructed encoder per frame (init_params), zero
    latents, a random target."""
    from ccmi import train as T
    arch = T.Arch(H, W)
    g = torch.Generator().manual_seed(5)
    prm = torch.stack([T.init_params(arch, torch.Generator().manual_seed(f)) for f in range(batch)])
    return arch, torch.zeros(batch, arch.n_latents, device=dev), prm.to(dev), torch.rand(batch, 3 * H * W, generator=g).to(dev), None


def test_overfitter_wires_step_and_seed(ccmi_lib, gpu):
    """Three updating steps with the in-kernel Kumaraswamy(2) noise (seed 11) end where three
    steps given the reference's draws of steps 1, 2, 3 end -- and not where step 1's draws given
    three times end, so the agreement is not one that a tolerance hides the noise in.

    The state is the freshly initialised encoder, not _random_state: Adam's first step is
    lr g / (|g| + eps), so entries with |g| ~ eps move by up to lr on a rounding error, and from
    _random_state that reaches 13 % of a frame's parameters (0.35 lr at most) after three steps --
    for the in-kernel noise and just as much (6 %, 0.21 lr) for the handed-in tensor moved by one
    float32 ulp, with every step's gradients within half of _grad_close's tolerance.  From the
    fresh state the in-kernel run has 0.08 % of a frame's parameters past 2e-3 lr (0.0023 lr at
    most), the one-ulp control none, the replay 99 % (3 lr)."""
    from test_train_gpu import _adam_close
    state = _fresh_state(gpu)
    n_lat, lr = state[0].n_latents, 1e-2

    def run(noise_of_step):
        of = _overfitter(state, 11)
        for t in (1, 2, 3):
            s = noise_of_step(t)
            noise = None if s is None else _ref_noise("kumaraswamy", 2.0, 11, s, 2, n_lat).to(gpu)
            of.step("softround", "kumaraswamy", 0.3, 2.0, 1e-3, lr=lr, noise=noise)
        torch.cuda.synchronize()
        assert of.t == 3
        return of.latents.cpu().numpy(), of.params.cpu().numpy()

    got, ref, replay = run(lambda t: None), run(lambda t: t), run(lambda t: 1)
    for b in range(2):
        _adam_close(got[0][b], ref[0][b], lr, f"frame {b} latents")
        _adam_close(got[1][b], ref[1][b], lr, f"frame {b} parameters")
        with pytest.raises(AssertionError):
            _adam_close(got[0][b], replay[0][b], lr, f"frame {b} latents, step 1's noise three times")
