"""GPU encoder overfit step (ccmi_train_step) against the reference and the CPU oracle.

* tests/golden/train_*.npz (reference modules, tools/gen_golden_train.py): loss, every
  parameter gradient, and the parameters after two clipped-Adam steps;
* oracle/train_oracle.py (torch autograd on CPU, pinned to the same goldens) for the
  paths the goldens cannot hold: quantisation noise (given to both as the same tensor),
  other quantizers, batches of frames with their own networks.
Tolerances (fp32, different summation order and expm1 ulps): loss and rate 1e-5
relative.  Gradients rtol 2e-3 with an absolute floor of 2e-4 x the largest gradient of
the tensor: the rate gradient has a 1 / P factor, and P = F(q+1/2) - F(q-1/2) cancels in
fp32 for latents far in the Laplace tails, where one ulp of expm1 is ~1e-3 of P.
Parameters after Adam: 2e-3 x lr absolute for all but 2 % of the entries, and at most
2 x lr for those (Adam moves a parameter by ~lr g / (|g| + eps): near-zero gradients make
that step ill-conditioned in any implementation).
"""
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
FILES = sorted(GOLDEN.glob("train_*.npz"))

pytestmark = pytest.mark.gpu


def _setup(z, gpu, batch=1):
    import train_oracle as to
    from ccmi import train as T
    st, target, meta = to.from_golden(z)
    mp = st.mp
    arch = T.Arch(H=mp.H, W=mp.W, dim_arm=mp.dim_arm, n_hidden=mp.n_hidden, layers=tuple(mp.layers),
                  n_grids=mp.n_grids, gain=mp.gain)
    params = T.pack_params(mp.arm, mp.ups_half, mp.pre_half, mp.syn)
    lat = torch.cat([x.reshape(-1) for x in st.lat]).detach()
    if meta["yuv420"]:
        tgt = torch.cat([target[c].reshape(-1) for c in "yuv"])
    else:
        tgt = target.reshape(-1)
    of = T.Overfitter(arch, lat.repeat(batch, 1).to(gpu), params.repeat(batch, 1).to(gpu),
                      tgt.repeat(batch, 1).to(gpu), yuv420=meta["yuv420"])
    return of, st, target, meta


def _flat_grads(st):
    return torch.cat([p.grad.reshape(-1) for p in st.params()]).numpy()


def _grad_close(got, ref, name, floor=None):
    tol = 2e-3 * np.abs(ref) + 1e-7 + 2e-4 * np.abs(ref).max()
    if floor is not None:
        tol = np.maximum(tol, floor)
    if "latent_grids" in name:
        # the rate term's 1 / P with P cancelling in fp32 deep in the Laplace tails (header):
        # at most 0.1 % of a latent grid's entries may reach 4x the tolerance
        err = np.abs(got - ref)
        assert np.mean(err > tol) <= 1e-3 and np.all(err <= 4 * tol), \
            (name, int((err > tol).sum()), float((err / tol).max()))
    else:
        assert np.all(np.abs(got - ref) <= tol), (name, got, ref, tol)


def _adam_close(got, ref, lr, name, g0=None):
    """Adam moves a parameter by ~lr g / |g| whatever |g|: an entry whose gradient is small
    next to the tensor's largest takes a step as sensitive to the float error of its gradient
    (bounded by the gradient test above: ~4e-5 of the tensor's largest at 128 x 192, the CPU
    restatement's own level) as the gradient is small.  Entries off by more than 2e-3 lr must
    be such entries (|g0| < 5 % of the tensor's largest) or at most 2 % of the tensor; even
    small-gradient entries may be at most 10 % of the tensor."""
    bad = np.abs(got - ref) > 1e-5 * np.abs(ref) + 2e-3 * lr
    if g0 is not None and bad.any():
        small = np.abs(g0) < 0.05 * np.abs(g0).max()
        assert bad.mean() <= 0.02 or (np.all(small[bad]) and bad.mean() <= 0.1), \
            f"{name}: {int(bad.sum())} of {bad.size} entries off, {int((bad & ~small).sum())} with a large gradient"
    else:
        assert bad.mean() <= 0.02, f"{name}: {int(bad.sum())} of {bad.size} entries off"
    assert np.all(np.abs(got - ref) <= 2 * lr + 1e-6), name


def _check_grads(got, st, names):
    o = 0
    for name, p in zip(names, st.params()):
        n = p.numel()
        _grad_close(got[o:o + n], p.grad.reshape(-1).numpy(), name)
        o += n


@pytest.mark.parametrize("f", FILES, ids=lambda f: f.stem)
def test_gpu_gradients_match_reference(f, gpu):
    _gradients_match_reference(f, gpu)


# the opt-in kernel forms the library ships next to the defaults (train_head.hip head_bwd_regs /
# train_sp.hip sp_bwd_persistent, read per launch): the register-form head backward
# (t_head_bwd_m) and the one-tile-per-workgroup 3x3 backward (t_sp_bwd<3>)
@pytest.mark.parametrize("env", [("CCMI_HEAD_BWD_REGS", "1"), ("CCMI_SP_BWD_PF", "0")], ids=lambda e: f"{e[0]}={e[1]}")
def test_gpu_gradients_opt_in_kernel_forms(env, gpu, monkeypatch):
    monkeypatch.setenv(*env)
    for f in FILES:
        _gradients_match_reference(f, gpu)


def _gradients_match_reference(f, gpu):
    import train_oracle as to
    z = np.load(f)
    of, st, target, meta = _setup(z, gpu)
    g = torch.zeros(1, of.N + of.P, device=gpu)
    loss = of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], update=False, grad_out=g)
    torch.cuda.synchronize()
    L, mse, rate, _ = loss[0].tolist()
    assert abs(L - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    assert abs(rate - float(z["rate_bit"])) <= 2e-5 * float(z["rate_bit"])
    # reference gradients (golden) in TrainState order
    names = to.golden_param_names(meta)
    got = g[0].cpu().numpy()
    o = 0
    for name, p in zip(names, st.params()):
        n = p.numel()
        _grad_close(got[o:o + n], z[f"g/{name}"].reshape(-1), name)
        o += n


@pytest.mark.parametrize("f", FILES, ids=lambda f: f.stem)
def test_forward_only_rate_read_right_after_the_call(f, gpu):
    """forward_only (the autograd forward) returns the ARM's rate, which is computed on the
    training side stream: values read right after the call, ordered only by the caller's
    stream, must be the final ones.  Against the diagnostic spin build (make -C cool-chic_amd
    spin; CCMI_LIB=.../libccmi_spin.so) a missing side-stream join reads stale values here."""
    from ccmi.autograd import TrainForward
    z = np.load(f)
    of, st, target, meta = _setup(z, gpu)
    cfg = dict(arch=of.arch, quantizer=meta["quantizer_type"], temperature=float(meta["temperature"]),
               yuv420=bool(meta["yuv420"]))
    raw, rate = TrainForward.apply(of.latents, of.params, cfg)
    got = float(rate.double().sum().item())  # stream-ordered read, no device synchronize before it
    assert abs(got - float(z["rate_bit"])) <= 2e-5 * float(z["rate_bit"]), (got, float(z["rate_bit"]))
    assert torch.isfinite(raw).all()


@pytest.mark.parametrize("f", [f for f in FILES if "g1/latent_grids.0.data" in np.load(f).files],
                         ids=lambda f: f.stem)
def test_gpu_gradients_at_step1_parameters_match_reference(f, gpu):
    """Goldens at a realistic size: the gradient at the reference's own step-1 parameters.
    (Chaining our own Adam steps there compares trajectories, not kernels: after one step the
    latents sit on the other side of clamp_min(P, 2^-16) / ReLU / scale-clamp switches for a
    few of the ~33 k latents, which moves individual ARM weight gradients by more than the
    float error; the two-step comparison stays on the small goldens below.)"""
    import train_oracle as to

    class _Npz(dict):  # the np.load interface from_golden / ModelParams.from_npz read
        @property
        def files(self):
            return list(self)

    z = _Npz(np.load(f))
    for k in list(z):
        if k.startswith("s1/"):
            z["p/" + k[3:]] = z[k]
    of, st, target, meta = _setup(z, gpu)
    g = torch.zeros(1, of.N + of.P, device=gpu)
    of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], update=False, grad_out=g)
    torch.cuda.synchronize()
    got = g[0].cpu().numpy()
    o = 0
    for name, p in zip(to.golden_param_names(meta), st.params()):
        n = p.numel()
        _grad_close(got[o:o + n], z[f"g1/{name}"].reshape(-1), "step-1 " + name)
        o += n


@pytest.mark.parametrize("f", [f for f in FILES if "g1/latent_grids.0.data" not in np.load(f).files],
                         ids=lambda f: f.stem)
def test_gpu_two_adam_steps_match_reference(f, gpu):
    import train_oracle as to
    z = np.load(f)
    of, st, target, meta = _setup(z, gpu)
    for s in (1, 2):
        of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], lr=meta["lr"], clip=0.1)
        torch.cuda.synchronize()
        lat = of.latents[0].cpu().numpy()
        prm = of.params[0].cpu().numpy()
        flat = np.concatenate([lat, prm])
        o = 0
        for name, p in zip(to.golden_param_names(meta), st.params()):
            n = p.numel()
            _adam_close(flat[o:o + n], z[f"s{s}/{name}"].reshape(-1), meta["lr"], f"step {s} {name}",
                        z[f"g/{name}"].reshape(-1))
            o += n


@pytest.mark.parametrize("f", [f for f in FILES if "g1/latent_grids.0.data" in np.load(f).files],
                         ids=lambda f: f.stem)
def test_gpu_two_adam_steps_at_128x192(f, gpu):
    """Two clipped-Adam steps on the realistic-size golden.  Step 1 is compared for every
    tensor.  Step 2 starts from OUR step-1 parameters, so it is compared only for the tensors
    whose gradient there already matches the reference's step-1 gradient (g1): on the others
    the trajectories split at a clamp / ReLU switch of a few latents (see the step-1 gradient
    test above), which is not a kernel error."""
    import train_oracle as to
    z = np.load(f)
    of, st, target, meta = _setup(z, gpu)
    names = to.golden_param_names(meta)
    sizes = [p.numel() for p in st.params()]
    of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], lr=meta["lr"], clip=0.1)
    g = torch.zeros(1, of.N + of.P, device=gpu)
    of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], update=False, grad_out=g)
    torch.cuda.synchronize()
    flat1 = np.concatenate([of.latents[0].cpu().numpy(), of.params[0].cpu().numpy()])
    g1 = g[0].cpu().numpy()
    match, o = {}, 0
    for name, n in zip(names, sizes):
        _adam_close(flat1[o:o + n], z[f"s1/{name}"].reshape(-1), meta["lr"], f"step 1 {name}", z[f"g/{name}"].reshape(-1))
        try:
            _grad_close(g1[o:o + n], z[f"g1/{name}"].reshape(-1), name)
            match[name] = True
        except AssertionError:
            match[name] = False
        o += n
    assert sum(match.values()) >= len(names) // 2, match
    of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], lr=meta["lr"], clip=0.1)
    torch.cuda.synchronize()
    flat2 = np.concatenate([of.latents[0].cpu().numpy(), of.params[0].cpu().numpy()])
    o = 0
    for name, n in zip(names, sizes):
        if match[name]:
            _adam_close(flat2[o:o + n], z[f"s2/{name}"].reshape(-1), meta["lr"], f"step 2 {name}",
                        z[f"g1/{name}"].reshape(-1))
        o += n


@pytest.mark.parametrize("qtype,ntype", [("softround", "kumaraswamy"), ("softround", "gaussian"), ("none", "kumaraswamy"),
                                         ("ste", "none"), ("true_ste", "none")])
def test_gpu_noise_and_quantizers_match_oracle(qtype, ntype, gpu):
    import train_oracle as to
    z = np.load(FILES[0])
    of, st, target, meta = _setup(z, gpu)
    g = torch.Generator().manual_seed(3)
    N = of.N
    if ntype == "kumaraswamy":
        noise = to.kumaraswamy(torch.rand(N, generator=g), 2.0)
    elif ntype == "gaussian":
        noise = 0.25 * torch.randn(N, generator=g)
    else:
        noise = torch.zeros(N)
    to.grads(st, target, qtype, 0.3, meta["lmbda"], meta["yuv420"], noise=noise)
    gout = torch.zeros(1, N + of.P, device=gpu)
    of.step(qtype, ntype, 0.3, 2.0, meta["lmbda"], update=False, noise=noise[None].to(gpu), grad_out=gout)
    torch.cuda.synchronize()
    _check_grads(gout[0].cpu().numpy(), st, to.golden_param_names(meta))


def _random_arch_vs_oracle(gpu, H, W, seed, K=8, Kp=7, yuv420=False, **kw):
    """Gradient of one softround + kumaraswamy step (the same noise tensor given to both) of a
    random network against the oracle's autograd, at an odd size so every pyramid level crops.
    kw: dim_arm / n_hidden / n_grids / layers for ModelParams.random and Arch."""
    import forward_oracle as fo
    import train_oracle as to
    from ccmi import train as T
    mp = fo.ModelParams.random(H, W, seed=seed, **kw)
    g = torch.Generator().manual_seed(1000 + seed)
    if (K, Kp) != (8, 7):
        mp.ups_half = [0.3 * torch.randn((K + 1) // 2, generator=g) for _ in mp.ups_half]
        mp.pre_half = [0.1 * torch.randn((Kp + 1) // 2, generator=g) for _ in mp.pre_half]
        mp.ups_k, mp.pre_k = K, Kp
    arch = T.Arch(H, W, dim_arm=mp.dim_arm, n_hidden=mp.n_hidden, layers=tuple(mp.layers), n_grids=mp.n_grids,
                  ups_k=K, pre_k=Kp)
    lat = [0.05 * torch.randn(h, w, generator=g) for h, w in mp.sizes]
    img = torch.rand(3, H, W, generator=g)
    if yuv420:
        target = {"y": img[0], "u": img[1, ::2, ::2], "v": img[2, ::2, ::2]}
        tflat = torch.cat([target[c].reshape(-1) for c in "yuv"])
    else:
        target, tflat = img, img.reshape(-1)
    st = to.TrainState(mp, lat)
    noise = to.kumaraswamy(torch.rand(arch.n_latents, generator=g), 2.0)
    keep = {}
    to.grads(st, target, "softround", 0.3, 1e-3, yuv420, noise=noise, keep=keep)
    # the ARM output biases' gradients are plain sums over the latents of dL/dmu and
    # dL/dlog_scale; on tiny frames those few terms can cancel (17 x 1: four terms of +-5e-3 sum
    # to 5e-5), so their absolute floor is 2e-4 x the sum of the terms' magnitudes rather than
    # of the (cancelled) result -- the same 2e-4-relative bar per term as every other tensor
    bias_floor = np.array([float(keep["mu"].grad.abs().sum()), float(keep["log_scale"].grad.abs().sum())])
    out_bias = 2 * (mp.n_hidden + 1) + mp.n_grids - 1  # index of the ARM output-layer bias in st.params()
    of = T.Overfitter(arch, torch.cat([x.reshape(-1) for x in lat])[None].to(gpu),
                      T.pack_params(mp.arm, mp.ups_half, mp.pre_half, mp.syn)[None].to(gpu),
                      tflat[None].to(gpu), yuv420=yuv420)
    gout = torch.zeros(1, of.N + of.P, device=gpu)
    of.step("softround", "kumaraswamy", 0.3, 2.0, 1e-3, update=False, noise=noise[None].to(gpu), grad_out=gout)
    torch.cuda.synchronize()
    got = gout[0].cpu().numpy()
    o = 0
    for i, p in enumerate(st.params()):
        n = p.numel()
        _grad_close(got[o:o + n], p.grad.reshape(-1).numpy(), f"{kw} K={K} Kp={Kp} tensor {i}" +
                    (" latent_grids" if i < mp.n_grids else ""), floor=2e-4 * bias_floor if i == out_bias else None)
        o += n


@pytest.mark.parametrize("K,Kp", [(4, 3), (4, 7), (6, 1), (6, 5), (6, 9), (8, 1), (8, 3), (8, 5), (8, 9)])
def test_gpu_gradients_other_kernel_sizes(K, Kp, gpu):
    """The upsampling backward for every kernel-size pair the training step accepts (the goldens
    hold the default 8 / 7 only): K = 8 runs the one-launch-per-level kernel (t_lvl_bwd), 4 / 6
    the separate refine / transposed-conv kernels."""
    _random_arch_vs_oracle(gpu, 45, 70, 10 * K + Kp, K, Kp)


@pytest.mark.parametrize("dim_arm,n_hidden", [(d, nh) for d in (8, 16, 24, 32) for nh in range(4)])
def test_gpu_gradients_arm_variants(dim_arm, n_hidden, gpu):
    """Every ARM the training step accepts (--dim_arm 8..32 x --n_hidden_layers_arm 0..3, the
    full product): the matrix-core ARM (dim 16) and the VALU ARM (8 / 24 / 32; 24 and 32 gather
    context row 4 above the tile).  The goldens hold (8, 2), (16, 2)."""
    _random_arch_vs_oracle(gpu, 37, 58, dim_arm + n_hidden, dim_arm=dim_arm, n_hidden=n_hidden)


@pytest.mark.parametrize("n_grids,layers,yuv420", [
    (2, "16-1-linear-relu|3-1-linear-none", False),
    (3, "16-1-linear-relu|3-1-linear-none", False),
    (4, "40-1-linear-relu|3-1-linear-none|3-3-residual-relu", True),
    (5, "64-1-linear-relu|3-1-linear-relu|3-3-residual-relu|3-3-residual-relu|3-3-residual-none", False),
    (6, "40-1-linear-relu|3-1-linear-none|3-3-residual-relu", False),
    (7, "24-1-linear-relu|3-1-linear-none|3-3-linear-relu|3-3-residual-none", True),
    (8, "24-1-linear-relu|3-1-linear-none|3-3-linear-relu|3-3-residual-none", False),
])
def test_gpu_gradients_synthesis_and_grid_variants(n_grids, layers, yuv420, gpu):
    """Latent-pyramid depth 2..8 (the 1x1 head's input width) and synthesis heads of 16..64
    channels followed by 0..3 3x3 layers, residual or not, with 444 and 420 targets (even frame
    size, as 420 needs; the coarser levels are odd and crop)."""
    import forward_oracle as fo
    _random_arch_vs_oracle(gpu, 42, 66, n_grids, n_grids=n_grids, layers=fo.parse_layers(layers), yuv420=yuv420)


@pytest.mark.parametrize("H,W", [(128, 192), (97, 161)])
def test_gpu_gradients_reference_default_decoder(H, W, gpu):
    """The reference's default decoder exactly (coolchic/utils/types.py:120-143: ARM 24,2, 7 grids,
    40-1-linear-relu|3-1-linear-none|3-3-residual-relu|3-3-residual-none) at sizes of several
    ARM tiles, 3x3-backward tiles and pyramid tiles per level: the VALU ARM t_arm<24, 2> with its
    4-rows-up contexts, and the next 3x3 layer applying the previous one's ReLU mask."""
    import forward_oracle as fo
    _random_arch_vs_oracle(gpu, H, W, 24, dim_arm=24, n_hidden=2, n_grids=7,
                           layers=fo.parse_layers("40-1-linear-relu|3-1-linear-none|3-3-residual-relu|3-3-residual-none"))


@pytest.mark.parametrize("H,W", [(33, 65), (17, 1), (1, 70), (2, 1), (81, 129)])
def test_gpu_gradients_border_tile_shapes(H, W, gpu):
    """Sizes whose last image row / column is the first of a 16 x 64 backward tile (H = 1 mod
    16, W = 1 mod 64) and 1-pixel image sides: the 3x3 backward's replicate-padding adjoint
    post-pass (t_sp_bwd<3>) then excludes ring slots and adds both edge terms of one pixel, and
    every pyramid level is 1 wide or 1 high.  The reference pads by replication
    (synthesis.py:264-277); the oracle's autograd differentiates exactly that."""
    _random_arch_vs_oracle(gpu, H, W, 7 * H + W)


def test_gpu_batch_of_frames_each_with_own_network(gpu):
    """Frames in a batch are independent: frame b's gradient equals a batch-of-1 run."""
    z = np.load(FILES[1])
    of, st, target, meta = _setup(z, gpu, batch=3)
    torch.manual_seed(0)
    of.params[1] += 0.01 * torch.randn_like(of.params[1])
    of.latents[2] += 0.05 * torch.randn_like(of.latents[2])
    g3 = torch.zeros(3, of.N + of.P, device=gpu)
    of.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], update=False, grad_out=g3)
    for b in range(3):
        of1, _, _, _ = _setup(z, gpu)
        of1.params.copy_(of.params[b:b + 1])
        of1.latents.copy_(of.latents[b:b + 1])
        g1 = torch.zeros(1, of.N + of.P, device=gpu)
        of1.step(meta["quantizer_type"], "none", meta["temperature"], 0.0, meta["lmbda"], update=False, grad_out=g1)
        torch.cuda.synchronize()
        a, r = g3[b].cpu().numpy(), g1[0].cpu().numpy()
        np.testing.assert_allclose(a, r, rtol=1e-4, atol=1e-6 * np.abs(r).max())


def test_gpu_overfit_reduces_loss(gpu):
    """A short c3x-like phase (softround + kumaraswamy noise from the in-kernel RNG, Adam
    1e-2) lowers the eval loss of a 64x96 frame."""
    import forward_oracle as fo
    from ccmi import train as T
    mp = fo.ModelParams.random(64, 96, seed=5)
    arch = T.Arch(64, 96)
    params = T.pack_params(mp.arm, mp.ups_half, mp.pre_half, mp.syn)
    g = torch.Generator().manual_seed(0)
    lat = 0.01 * torch.randn(1, arch.n_latents, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 64), torch.linspace(0, 1, 96), indexing="ij")
    img = torch.stack([0.5 + 0.3 * torch.sin(6 * xx + 3 * yy), 0.5 + 0.2 * torch.cos(5 * yy), 0.4 + 0.2 * xx])
    tgt = torch.cat([img[0].reshape(-1), img[1, ::2, ::2].reshape(-1), img[2, ::2, ::2].reshape(-1)])[None]
    of = T.Overfitter(arch, lat.to(gpu), params[None].to(gpu), tgt.to(gpu), yuv420=True, seed=1)
    first = of.step("softround", "kumaraswamy", 0.3, 2.0, 1e-3, lr=1e-2).clone()
    for _ in range(200):
        last = of.step("softround", "kumaraswamy", 0.3, 2.0, 1e-3, lr=1e-2)
    torch.cuda.synchronize()
    assert torch.isfinite(last).all()
    assert float(last[0, 0]) < 0.5 * float(first[0, 0])


def test_gpu_c3x_schedule_short(gpu):
    """The c3x schedule driver (warm-up candidates as one batch, then the three phases) at
    2 % of its iterations on two 48x64 frames: runs end to end, keeps one network per frame
    and improves on the initial loss."""
    from ccmi import train as T
    arch = T.Arch(48, 64)
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 48), torch.linspace(0, 1, 64), indexing="ij")
    imgs = []
    for k in range(2):
        img = torch.stack([0.5 + 0.3 * torch.sin((4 + k) * xx + 2 * yy), 0.5 + 0.1 * torch.cos(3 * yy), 0.5 + 0.1 * xx])
        img = (img + 0.01 * torch.randn(img.shape, generator=g)).clamp(0, 1)
        imgs.append(torch.cat([img[0].reshape(-1), img[1, ::2, ::2].reshape(-1), img[2, ::2, ::2].reshape(-1)]))
    tg = torch.stack(imgs).to(gpu)
    of0 = T.Overfitter(arch, torch.zeros(2, arch.n_latents, device=gpu),
                       torch.stack([T.init_params(arch, torch.Generator().manual_seed(0))] * 2).to(gpu), tg)
    init = of0.validate(1e-3)
    of, best = T.overfit(arch, tg, 1e-3, scale=0.02, seed=3)
    torch.cuda.synchronize()
    assert of.B == 2 and torch.isfinite(best).all()
    assert bool((best[:, 0] < init[:, 0]).all())


def _adam_pair(gpu, k):
    """A 2-frame batch (frames with different networks) after k - 1 clipped-Adam steps, so
    its moments are non-zero; returns the Overfitter and a deep copy of its state."""
    z = np.load(FILES[1])
    of, st, target, meta = _setup(z, gpu, batch=2)
    torch.manual_seed(0)
    of.params[1] += 0.01 * torch.randn_like(of.params[1])
    for _ in range(k - 1):
        of.step("ste", "none", 1e-4, 1.0, 1e-3, lr=1e-2)
    state = [x.clone() for x in (of.latents, of.params, of.m, of.v, of.steps)]
    return of, state, meta


def _restore(of, state, t):
    for dst, src in zip((of.latents, of.params, of.m, of.v, of.steps), state):
        dst.copy_(src)
    of.t = t


def test_gpu_per_frame_adam_steps_uniform_equals_scalar(gpu):
    """adam_steps = [k, k] (the per-frame bias-correction path, t_adam_bc) gives the update of
    the scalar step = k path: the same parameters, latents and moments."""
    k = 4
    of, state, meta = _adam_pair(gpu, k)
    of.step("ste", "none", 1e-4, 1.0, 1e-3, lr=1e-2)        # scalar path, step k
    scalar = [x.clone() for x in (of.latents, of.params, of.m, of.v)]
    _restore(of, state, k - 1)
    of.steps_uniform = False                                  # per-frame path, steps [k, k]
    of.step("ste", "none", 1e-4, 1.0, 1e-3, lr=1e-2)
    torch.cuda.synchronize()
    assert of.steps.tolist() == [k, k]
    for a, b, name in zip((of.latents, of.params, of.m, of.v), scalar, ("latents", "params", "m", "v")):
        # same formula in double on host and device, rounded once to fp32; the gradients of
        # two launches may differ in summation order (atomics), hence the ulp-level bound
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-8, msg=name)


def test_gpu_per_frame_adam_steps_diverging(gpu):
    """Frames of one batch at their own Adam steps [k1, k2] move as the scalar path moves them at
    k1 (frame 0) and at k2 (frame 1); a frame at step <= 0 keeps its parameters and moments."""
    k1, k2 = 2, 7
    of, state, meta = _adam_pair(gpu, 3)
    ref = {}
    for k in (k1, k2):
        _restore(of, state, k - 1)
        of.step("ste", "none", 1e-4, 1.0, 1e-3, lr=1e-2)
        ref[k] = [x.clone() for x in (of.latents, of.params, of.m, of.v)]
    _restore(of, state, 0)
    of.steps.copy_(torch.tensor([k1 - 1, k2 - 1], dtype=torch.int32))
    of.steps_uniform = False
    of.step("ste", "none", 1e-4, 1.0, 1e-3, lr=1e-2)
    torch.cuda.synchronize()
    assert of.steps.tolist() == [k1, k2]
    for b, k in ((0, k1), (1, k2)):
        for a, r, name in zip((of.latents, of.params, of.m, of.v), ref[k], ("latents", "params", "m", "v")):
            torch.testing.assert_close(a[b], r[b], rtol=1e-5, atol=1e-8, msg=f"frame {b} step {k} {name}")
    # the two bias corrections really differ: the frames did not both take one of them
    d1 = (ref[k1][1][0] - state[1][0]).abs().max()
    d2 = (ref[k2][1][0] - state[1][0]).abs().max()
    assert abs(float(d1) / float(d2) - 1) > 0.2
    # step <= 0: frozen frame (parameters, latents and Adam moments untouched)
    _restore(of, state, 0)
    of.steps.copy_(torch.tensor([-1, k2 - 1], dtype=torch.int32))
    of.steps_uniform = False
    of.step("ste", "none", 1e-4, 1.0, 1e-3, lr=1e-2)
    torch.cuda.synchronize()
    for a, s0, name in zip((of.latents, of.params, of.m, of.v), state, ("latents", "params", "m", "v")):
        assert torch.equal(a[0], s0[0]), f"frozen frame changed its {name}"
    torch.testing.assert_close(of.params[1], ref[k2][1][1], rtol=1e-5, atol=1e-8)


def test_gpu_run_phase_reload_uses_per_frame_steps(gpu):
    """A cosine phase with a short patience on a real Overfitter: frames whose loss stalls
    reload their best parameters AND Adam state (train.py:226-236), which sends the batch down
    the per-frame Adam-step path; the phase ends on every frame's best record."""
    from ccmi import train as T
    z = np.load(FILES[1])
    of, st, target, meta = _setup(z, gpu, batch=2)
    torch.manual_seed(1)
    of.params[1] += 0.01 * torch.randn_like(of.params[1])
    # lr 0.5: the loss blows up after a few steps, so the records stop and patience expires
    ph = T.Phase(lr=0.5, max_itr=40, freq_valid=2, patience=4, schedule_lr=True, end_lr=0.4,
                 quantizer_type="ste", quantizer_noise_type="none", softround_temperature=(1e-4, 1e-4))
    best = T.run_phase(of, ph, 1e-3)
    torch.cuda.synchronize()
    assert not of.steps_uniform, "no frame reloaded its optimizer state"
    assert torch.isfinite(best).all()
    assert of.phase_iterations == [40, 40]
    # the phase restores each frame's best record: validating now gives the recorded loss
    torch.testing.assert_close(of.validate(1e-3)[:, 0], best[:, 0], rtol=1e-5, atol=0)
