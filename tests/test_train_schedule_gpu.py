"""The training step's gradients (train.hip and its stage units train_*.hip) at every quantiser setting of the c3x schedule, against
the oracle in float64: tests/test_train_tiles_gpu.py holds them at the warm-up's setting only
(softround + kumaraswamy a = 2, T = 0.3), 800 of the preset's 14,000 iterations per image.

Per setting of tests/train_ref.py SCHEDULE and architecture (hop 33 x 65, default decoder 34 x 66 in
4:2:0), B = 8 frames cycling D = 4, the noise handed in as a tensor: loss rows to ROW_TOL, every
gradient entry of every frame to 16 e S_T, the norm to its bound -- the assertions of
test_train_tiles_gpu.py, whose code this file runs (_check_frames).  The frames' preconditions are
pinned on the CPU by tests/test_train_ref.py.

hardround: dq = 0, so the latent part of grad_out is 0.0 exactly in every frame; the parameter
gradients, the loss row and the norm are held to the true-ste references of the same frames (the
same forward, y = rint(x)).

ste at T = 1e-4, the setting of the schedule's last 2,500 iterations, in factors.  At this
temperature the float32 oracle of the whole step is 2^-5 from float64 on the latents (the float32
fraction, tests/quant_ref.py, times upstream gradients of mixed sign), so 16 e S_T does not apply
to them.  The step forms a latent's gradient as G = gq * dq with gq = dL/dy and dq = gain * d
(t_quant: dq[wi] = gain * d; t_latgrad_sumsq multiplies), and true_ste is the same step with
d = 1.  On frames whose latents are planted on the derivative's peak (train_ref lat_plant="half"),
two steps on the same Overfitter:
  (a) true_ste: every gradient to the frame's float64 oracle within 16 e S_T, as above;
  (b) ste, T = 1e-4: parameter gradients and loss rows to the same references and bounds (they do
      not depend on dq);
  (c) ste latents, entry by entry: |G[i] - g_true[i] d64[i]| <= 16 e S_T d64[i] + bound_d |g_true[i]|
      with g_true the float64 true_ste latent gradient (= gain * dL/dy, so g_true d64 =
      (g_true / gain) (gain d64): the gain is in g_true once and cancels out of the factors), d64
      and bound_d = 16 max(e32_d, 2^-22) max |d64| from quant_ref on the grid's own float32
      x = 16 * latent (exact).  At least half of each grid's entries have d64 > 1.
Latent-only mode (update="latent", the last 1,000 iterations): the step's kernels are the same and
only t_adam's range differs, so grad_out of such a step satisfies (b) and (c) too; its latent part
is compared with the update=False step's, see test_latent_only_step.

Worst error / bound on an MI355X (measured against the float64 oracle; the bounds are not to be
tightened to these); e as computed on that machine's CPU; hop / default decoder in 4:2:0:
  setting                                    e                  gradients      latents        norm
  warmup-a1   softround, kumaraswamy 1, 0.3  6.4e-6 / 3.1e-6    0.027 / 0.056  0.027 / 0.056  0.002 / 0.005
  main-start  softround, gaussian .25, 0.3   8.3e-6 / 5.2e-6    0.022 / 0.029  0.013 / 0.020  0.001 / 0.001
  main-mid    softround, gaussian .175, 0.2  5.2e-6 / 1.8e-6    0.092 / 0.183  0.092 / 0.183  0.004 / 0.003
  main-end    softround, gaussian .1, 0.1    7.7e-6 / 4.1e-6    0.049 / 0.068  0.049 / 0.068  0.001 / 0.031
  ste-warm    ste, 0.3                       2.7e-6 / 2.8e-6    0.053 / 0.060  0.030 / 0.036  0.001 / 0.005
  true-ste    true_ste                       1.4e-6 / 1.5e-6    0.085 / 0.392  0.037 / 0.392  0.006 / 0.009
  alone-end   softround_alone, 0.1           5.6e-6 / 3.7e-6    0.044 / 0.102  0.044 / 0.102  0.002 / 0.002
  noise-only  none, gaussian .25             3.1e-6 / 3.0e-6    0.035 / 0.019  0.035 / 0.016  0.004 / 0.002
  hardround   hardround                      1.4e-6 / 1.5e-6    0.085 / 0.334  0 (equal)      0.005 / 0.005
  ste-end     (a) true_ste, planted          5.1e-6 / 2.9e-6    0.028 / 0.071  0.018 / 0.042  0.001 / 0.003
              (b) ste 1e-4, parameters                          0.028 / 0.071
              (c) ste 1e-4, latents: |G - g_true d64| / bound   0.015 / 0.017  (largest d64 5000, 53 % above 1)
  latent-only (hop): (b) 0.028, (c) 0.015; the update=False repeats and the latent-only step differ in 13 entries
              over the six comparisons of 8 x 2927, by at most 4.8e-4 of 2 e S_T d64.
  loss rows: within 2.4e-7 relative everywhere (bounds 1e-5, 1e-5, 2e-5).
Two frames missed under their first seeds, 112-fold and 66-fold: a ReLU argument of the ARM at 1.1e-7
of its terms and one of the head at 1.1e-8, whose signs no float32 evaluation resolves
(tests/train_ref.py SCHEDULE_RESEED); no miss traced to the kernels.
Each case takes 0.1 .. 0.9 s on the GPU machine, the oracles of all cases together 6 s.
"""
import numpy as np
import pytest
import torch

import quant_ref as Q
import train_ref as R
from test_train_tiles_gpu import _check_frames, _check_grads, _check_rows, _overfitter

pytestmark = pytest.mark.gpu

B = 8
SETTINGS = [(s, c) for s in R.SCHEDULE for c in R.SCHEDULE_CASES]


def _ids(x):
    return x if isinstance(x, str) else x.name


@pytest.mark.parametrize("setting,case", SETTINGS, ids=_ids)
def test_step_at_each_setting(setting, case, gpu):
    frs = R.schedule_frames(setting, case)
    print()
    of, _, idx = _check_frames(frs, B, gpu, f"{setting.name} {case} B={B}",
                               (setting.qtype, setting.ntype, setting.T, setting.nparam))
    if setting.name == "hardround":
        # (_check_frames held the latent part to a bound of 0 already; said once more in plain words)
        gout = torch.full((B, of.N + of.P), float("nan"), device=gpu)
        of.step("hardround", "none", 1.0, 1.0, R.LMBDA, update=False, grad_out=gout)
        torch.cuda.synchronize()
        assert bool((gout[:, :of.N] == 0).all())


def _ste_end_refs(frs, e, gpu):
    """Per frame [D, N]: g_true, d64, and the bound of (c)."""
    g, d, b = [], [], []
    for f in frs:
        x = (f.lat * f.gain).numpy()
        gt = np.concatenate(f.g64[:f.n_grids])
        d64 = np.empty(f.N)
        bd = np.empty(f.N)
        o = 0
        for i in range(f.n_grids):
            n = f.sizes[i]
            _, dd, _, bound_d, _, e_d = Q.bounds(x[o:o + n], "ste", R.STE_END.T)
            assert np.mean(dd > 1) >= 0.5, (i, n, float(np.mean(dd > 1)))     # (c) is not vacuous
            d64[o:o + n], bd[o:o + n] = dd, bound_d
            o += n
        assert o == f.N
        s = np.repeat(R.grad_bounds(f, e)[:f.n_grids], f.sizes[:f.n_grids])
        g.append(gt)
        d.append(d64)
        b.append(s * d64 + bd * np.abs(gt))
    t = lambda a: torch.tensor(np.stack(a), device=gpu)
    return t(g), t(d), t(b)


def _check_ste_end(frs, e, idx, gout, loss, what):
    """(b) and (c) of the header for a grad_out of the ste step at T = 1e-4."""
    N = frs[0].N
    _check_rows(loss, [f.row64 for f in frs], idx, what)
    _check_grads(frs, e, idx, gout, loss, what + " parameters", norm=False, columns=slice(N, None))
    g, d, b = _ste_end_refs(frs, e, gout.device)
    err = (gout[:, :N].double() - (g * d)[idx]).abs()
    ratio = err / b[idx]
    print(f"{what} latents: worst |G - g_true d64| / bound {float(ratio.max()):.3f}; largest d64 {float(d.max()):.1f}, "
          f"entries with d64 > 1: {float((d > 1).double().mean()):.2f}")
    assert float(ratio.max()) <= 1.0, (what, float(ratio.max()), int(ratio.argmax()))


@pytest.mark.parametrize("case", R.SCHEDULE_CASES)
def test_ste_at_1e_4_in_factors(case, gpu):
    frs = R.schedule_frames(R.STE_END, case)
    e = max(f.e32 for f in frs)
    print()
    what = f"ste-end {case} B={B}"
    of3 = _check_frames(frs, B, gpu, what + " (a) true_ste", ("true_ste", "none", 1.0, 1.0))       # (a)
    of, noise, idx = of3
    gout = torch.full((B, of.N + of.P), float("nan"), device=gpu)
    loss = of.step("ste", "none", R.STE_END.T, 1.0, R.LMBDA, update=False, noise=noise, grad_out=gout)
    torch.cuda.synchronize()
    _check_ste_end(frs, e, idx, gout, loss, what + " (b, c) ste 1e-4")


def test_latent_only_step(gpu):
    """One ste step at T = 1e-4 with update="latent" on a fresh Overfitter: its grad_out (written
    before t_adam moves the latents) is held to (b) and (c), the latents move and the parameters
    do not.  Its latent part against three repeats of the update=False step: float atomics reach
    the latent gradients (on an MI355X the repeats agree bit for bit in most frames and differ by
    a rounding of an entry in some), so the comparison is not bitwise.  Another order of the same
    float32 sum is another float32 evaluation of it, and two of those are within 2 e of the
    tensor's largest entry of each other, e the float32 oracle's own distance from float64:
    |G_latent_only[i] - G_repeat[i]| <= 2 e S_T d64[i] against every repeat, and the repeats among
    themselves.  Measured: 13 entries differ, by at most 4.8e-4 of that bound."""
    case = "hop"
    frs = R.schedule_frames(R.STE_END, case)
    e = max(f.e32 for f in frs)
    of, noise, idx = _overfitter(frs, B, gpu)
    reps = []
    for _ in range(3):
        g = torch.full((B, of.N + of.P), float("nan"), device=gpu)
        of.step("ste", "none", R.STE_END.T, 1.0, R.LMBDA, update=False, noise=noise, grad_out=g)
        reps.append(g[:, :of.N].clone())
    lat0, params0 = of.latents.clone(), of.params.clone()
    gl = torch.full((B, of.N + of.P), float("nan"), device=gpu)
    loss = of.step("ste", "none", R.STE_END.T, 1.0, R.LMBDA, lr=1e-4, update="latent", noise=noise, grad_out=gl).clone()
    torch.cuda.synchronize()
    print()
    _check_ste_end(frs, e, idx, gl, loss, f"ste-end {case} latent-only")
    assert not torch.equal(of.latents, lat0) and torch.equal(of.params, params0)    # latents moved, nothing else
    _, d, _ = _ste_end_refs(frs, e, gpu)
    s_t = torch.tensor(np.stack([np.repeat(f.S[:f.n_grids], f.sizes[:f.n_grids]) for f in frs]), device=gpu)
    bound = (2 * e * s_t * d)[idx]
    worst, differ = 0.0, 0
    for a, b in [(gl[:, :of.N], r) for r in reps] + [(reps[0], reps[1]), (reps[0], reps[2]), (reps[1], reps[2])]:
        diff = (a.double() - b.double()).abs()
        differ += int((diff > 0).sum())
        worst = max(worst, float((diff / bound).max()))
    print(f"latent-only against update=False and the repeats among themselves: {differ} entries differ, "
          f"largest difference / (2 e S_T d64) {worst:.2e}")
    assert worst <= 1.0
