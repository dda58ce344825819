"""The training step's gradients (train.hip and its stage units train_*.hip) off the rate floor, with every persistent kernel on
its second and later work units: against the oracle in float64 (tests/train_ref.py; the frames'
preconditions and the cases' workgroup arithmetic are pinned on the CPU by tests/test_train_ref.py).

Each frame of a batch has its own network, latents, target and noise tensor; D distinct frames are
cycled as b % D.  Every row's loss and mse are held to 1e-5 relative and its rate to 2e-5 (the
project's figures), every gradient entry of every frame to 16 e S_T and the gradient norm
(loss[:, 3]) to its own bound (header of tests/train_ref.py), e the largest e32 of the case's frames.

  a  one workgroup per frame: B = 2048 frames of 33 x 65 (34 x 66 in 420); the ARM, the 3x3 backward
     and the head backward each loop over all of a frame's units (31 tiles, 6 tiles, 17 chunks on
     1, 1 and <= 2 workgroups at 256 CUs; >= 3 iterations asserted from the device's CU count)
  b  uneven split: B = CUs // 2 frames of 81 x 129; some workgroups take one iteration more
  c  one large frame, 300 x 450: the second pass of t_latgrad_sumsq and t_loss, 810 ARM tiles on 256
     workgroups
  d  loss rows of step(update=False) and validate() at B = 1025 and 2048 (t_finish as a grid)

Worst error / bound on an MI355X (measured against the float64 oracle; the bounds are not to be
tightened to these); e as computed on that machine's CPU:
  case                          B     e        gradients (worst tensor)  latents  norm
  hop                           2048  4.5e-6   0.057                     0.048    0.005
  hop, CCMI_HEAD_BWD_REGS=1     2048  4.5e-6   0.054                     0.040    0.005
  default decoder, 420          2048  6.1e-6   0.048                     0.048    0.002
  full-width head, 5 grids      2048  1.7e-6   0.145                     0.145    0.003
  head only, 2 grids, K6 Kp5    2048  2.9e-6   0.020                     0.012    0.001
  the other 15 ARMs             2048  1.9e-6 .. 8.5e-6  0.028 .. 0.179 (24, 1)  0.015 .. 0.147 (8, 3)  0.001 .. 0.011
  uneven, hop                   128   3.1e-6   0.035                     0.030    0.003
  uneven, default decoder       128   5.3e-6   0.068                     0.025    0.001
  large, hop                    1     6.4e-6   0.007                     0.007    0.000
  large, head only              1     8.0e-6   0.013                     0.004    0.000
  loss rows, every case and B = 1025 / 2048: loss, mse and rate within 2e-7 relative (bounds 1e-5,
  1e-5, 2e-5).
The large hop frame under its first seed missed the bound 14-fold at one pixel's latents: a ReLU
argument of 2.2e-8 there, whose sign no float32 evaluation resolves (tests/train_ref.py RESEED).
Each case takes 0.1 .. 1 s on the GPU machine, the oracles of all cases together 12 s.
"""
import numpy as np
import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

ROW_TOL = (1e-5, 1e-5, 2e-5)   # loss, mse, rate: relative


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _overfitter(frs, B, gpu):
    """B frames cycling the D frames of frs; returns (Overfitter, noise [B, N], frame index [B])."""
    from ccmi import train as T
    idx = torch.arange(B, device=gpu) % len(frs)
    stack = lambda k: torch.stack([getattr(f, k) for f in frs]).to(gpu)[idx].contiguous()
    of = T.Overfitter(T.Arch(**frs[0].arch), stack("lat"), stack("params"), stack("target"), yuv420=frs[0].yuv420)
    assert (of.N, of.P) == (frs[0].N, frs[0].P)
    return of, stack("noise"), idx


def _check_rows(loss, ref_rows, idx, what):
    """loss [B, 4] against the D reference rows (loss, mse, rate), cycled by idx."""
    assert bool(torch.isfinite(loss).all()), f"{what}: a loss row is not finite"
    ref = torch.tensor(ref_rows, dtype=torch.float64, device=loss.device)[idx]
    rel = (loss[:, :3].double() - ref).abs() / ref.abs()
    worst = rel.max(dim=0).values.tolist()
    print(f"\n{what}: worst relative error loss {worst[0]:.2e} mse {worst[1]:.2e} rate {worst[2]:.2e}")
    for k, (w, tol) in enumerate(zip(worst, ROW_TOL)):
        assert w <= tol, (what, "loss mse rate".split()[k], w, int(rel[:, k].argmax()))
    return worst


WARMUP = ("softround", "kumaraswamy", R.TEMP, R.NOISE_A)   # quantiser, noise, temperature, noise parameter


def _ratio(err, bnd):
    """err / bnd entry by entry; where the bound is 0 (a gradient that is zero by definition) the
    error has to be 0 too."""
    return torch.where(bnd > 0, err / bnd, torch.where(err == 0, 0.0, float("inf")).to(err.dtype))


def _check_grads(frs, e, idx, gout, loss, what, norm=True, columns=None):
    """gout [B, N + P] (and loss[:, 3], the norm) against the frames' float64 references, every
    entry of every frame on the device: [D, N + P] references and bounds, cycled by idx.
    columns: a slice of the row to check (all of it by default).  Returns the worst ratio per
    tensor."""
    gpu = gout.device
    ref = torch.tensor(np.stack([np.concatenate(f.g64) for f in frs]), device=gpu)
    bnd = torch.tensor(np.stack([np.repeat(R.grad_bounds(f, e), f.sizes) for f in frs]), device=gpu)
    assert bool(torch.isfinite(gout).all()), f"{what}: a gradient entry is not finite (or not written)"
    ratio = _ratio((gout.double() - ref[idx]).abs(), bnd[idx])
    lo, hi, _ = (columns or slice(None)).indices(gout.shape[1])
    per, o = [], 0
    for n in frs[0].sizes:
        per.append(float(ratio[:, o:o + n].max()) if lo <= o and o + n <= hi else 0.0)
        o += n
    nr = 0.0
    if norm:
        nrm = [R.norm_bound(f, e) for f in frs]
        nref = torch.tensor([r for r, _ in nrm], dtype=torch.float64, device=gpu)[idx]
        nbnd = torch.tensor([b for _, b in nrm], dtype=torch.float64, device=gpu)[idx]
        nratio = (loss[:, 3].double() - nref).abs() / nbnd
        nr = float(nratio.max())
    worst_t = int(np.argmax(per))
    print(f"{what}: e {e:.2e}, worst gradient error / bound {max(per):.3f} (tensor {worst_t} of {len(per)}), "
          f"latents {max(per[:frs[0].n_grids]):.3f}, norm {nr:.3f}")
    assert max(per) <= 1.0, (what, "tensor", worst_t, per)
    if norm:
        assert nr <= 1.0, (what, "gradient norm", nr, int(nratio.argmax()))
    return per


def _check_frames(frs, B, gpu, what, setting=WARMUP, of=None):
    """One step(update=False) of B frames cycling frs at a quantiser setting, noise handed in:
    loss rows, every gradient entry and the norm against the frames' references.  of: an
    (Overfitter, noise, idx) of these frames to reuse.  Returns it."""
    e = max(f.e32 for f in frs)
    assert e <= R.E32_MAX
    of, noise, idx = of or _overfitter(frs, B, gpu)
    gout = torch.full((B, of.N + of.P), float("nan"), device=gpu)
    loss = of.step(*setting, R.LMBDA, update=False, noise=noise, grad_out=gout)
    torch.cuda.synchronize()
    _check_rows(loss, [f.row64 for f in frs], idx, what)
    _check_grads(frs, e, idx, gout, loss, what)
    return of, noise, idx


def _check_case(case, gpu):
    B = R.batch_of(case, _cus(gpu))
    _check_frames(R.case_frames(case), B, gpu, f"{case.name} B={B}")


def _cases(group):
    return [c for c in R.CASES if c.group == group]


@pytest.mark.parametrize("case", _cases("a"), ids=lambda c: c.name)
def test_one_workgroup_per_frame(case, gpu, monkeypatch):
    it = R.case_iterations(case, _cus(gpu))
    assert all(v >= 3 for v in it.values()), (it, "this device gives a frame too many workgroups for the case")
    if case.env:
        monkeypatch.setenv(*case.env)
    _check_case(case, gpu)


@pytest.mark.parametrize("case", _cases("b"), ids=lambda c: c.name)
def test_uneven_split(case, gpu):
    cus = _cus(gpu)
    it = R.case_iterations(case, cus)
    assert it["arm"] >= 3 and it["sp"] >= 2 and it["head"] >= 2, it
    _check_case(case, gpu)


@pytest.mark.parametrize("case", _cases("c"), ids=lambda c: c.name)
def test_one_large_frame(case, gpu):
    u = R.units(case.H, case.W, **case.arch)
    assert u.latgrad_passes == 2 and u.loss_passes == 2
    assert R.case_iterations(case, _cus(gpu))["arm"] >= 2
    _check_case(case, gpu)


@pytest.mark.parametrize("B", [1025, 2048])
def test_loss_rows_of_batches_above_1024(B, gpu):
    """step(update=False) and validate() write their loss rows with t_finish, one thread per frame:
    past 1024 frames that needs more than one block."""
    frs = R.case_frames("hop")
    of, noise, idx = _overfitter(frs, B, gpu)
    of.loss.fill_(float("nan"))
    loss = of.step("softround", "kumaraswamy", R.TEMP, R.NOISE_A, R.LMBDA, update=False, noise=noise)
    torch.cuda.synchronize()
    _check_rows(loss, [f.row64 for f in frs], idx, f"step(update=False) B={B}")
    of.loss.fill_(float("nan"))
    val = of.validate(R.LMBDA)
    torch.cuda.synchronize()
    _check_rows(val, [f.eval64 for f in frs], idx, f"validate() B={B}")
