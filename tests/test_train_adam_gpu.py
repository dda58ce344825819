"""The training step's clipped Adam (train.hip t_adam, t_adam_bc) against a float64 restatement
(tests/train_ref.py adam64), entry by entry: three frames of different gradient norms, two warm-up
steps so that m and v are non-zero, then ONE updating step with grad_out given.  adam64 is fed the
device's own gradient row and its own loss[:, 3], so the comparison isolates the update: latents,
parameters, m and v must come out within K 2^-24 of the magnitude of each expression's terms
(K counted rounding by rounding in the header of tests/train_ref.py); what the step must not touch
(a frozen frame, the parameters of a latent-only step) stays bit for bit.

Worst error / bound on an MI355X (the bounds are not to be tightened to these):
  case                              m      v      p
  step 3, clip 0.1 (active)         0.722  0.815  0.881
  step 3, clip 100 (coefficient 1)  0.593  0.490  0.881
  step 3, clip 0                    0.593  0.490  0.881
  step 1, clip 0.1                  0.722  0.815  0.891
  latent-only, step 3               0.722  0.815  0.807
  per-frame steps 2, 7 and frozen   0.722  0.815  0.907
"""
import numpy as np
import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

LR = 1e-2
STEP = ("softround", "kumaraswamy", R.TEMP, R.NOISE_A, R.LMBDA)


@pytest.fixture(scope="module")
def warm(gpu):
    """(Overfitter, noise, saved state) of the three frames after two clipped steps."""
    from ccmi import train as T
    frs = R.case_frames("hop")[:3]
    stack = lambda k: torch.stack([getattr(f, k) for f in frs]).to(gpu)
    of = T.Overfitter(T.Arch(**frs[0].arch), stack("lat"), stack("params"), stack("target"), yuv420=False)
    noise = stack("noise")
    for _ in range(2):
        of.step(*STEP, lr=LR, clip=0.1, noise=noise)
    torch.cuda.synchronize()
    assert of.t == 2 and of.steps.tolist() == [2, 2, 2]
    assert float((of.m != 0).float().mean()) > 0.9 and float((of.v > 0).float().mean()) > 0.9
    state = [x.clone() for x in (of.latents, of.params, of.m, of.v)]
    return of, noise, state


def _restore(of, state, t, steps=None):
    for dst, src in zip((of.latents, of.params, of.m, of.v), state):
        dst.copy_(src)
    of.t = t
    of.steps.copy_(torch.tensor(steps if steps is not None else [t] * of.B, dtype=torch.int32))
    of.steps_uniform = steps is None


def _rows(of):
    """(p, m, v) as float32 arrays [B, N + P], p = latents then parameters."""
    p = torch.cat([of.latents, of.params], dim=1)
    return [x.cpu().numpy().copy() for x in (p, of.m, of.v)]


def _step_and_check(of, noise, clip, ts, what, update=True, per_frame=False):
    """One updating step from the restored state; frame b at Adam step ts[b] (<= 0: frozen)."""
    B, N = of.B, of.N
    p0, m0, v0 = _rows(of)
    G = torch.full((B, of.N + of.P), float("nan"), device=of.latents.device)
    loss = of.step(*STEP, lr=LR, clip=clip, update=update, noise=noise, grad_out=G).clone()
    torch.cuda.synchronize()
    G, norm = G.cpu().numpy(), loss[:, 3].cpu().numpy()
    assert np.isfinite(G).all() and np.isfinite(norm).all()
    p1, m1, v1 = _rows(of)
    worst = {}
    for b in range(B):
        if ts[b] <= 0:
            for name, a0, a1 in (("p", p0, p1), ("m", m0, m1), ("v", v0, v1)):
                assert np.array_equal(a0[b], a1[b]), f"{what}: frozen frame {b} changed its {name}"
            continue
        r = R.adam64(G[b], m0[b], v0[b], p0[b], norm[b], clip, LR, ts[b])
        n = N if update == "latent" else N + of.P
        for name, got, ref, tol in zip("mvp", (m1, v1, p1), (r.m, r.v, r.p), R.adam_bounds(r, per_frame)):
            ratio = float((np.abs(got[b, :n] - ref[:n]) / tol[:n]).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ratio <= 1.0, (what, "frame", b, name, ratio)
        if update == "latent":
            for name, a0, a1 in (("parameters", p0, p1), ("m", m0, m1), ("v", v0, v1)):
                assert np.array_equal(a0[b, N:], a1[b, N:]), f"{what}: latent-only step changed the {name} of frame {b}"
        assert np.any(p1[b, :N] != p0[b, :N]), f"{what}: frame {b} did not move"
    print(f"\n{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return norm


def test_frames_have_different_norms(warm, gpu):
    of, noise, state = warm
    _restore(of, state, 2)
    norm = of.step(*STEP, update=False, noise=noise)[:, 3].tolist()
    assert min(abs(a - b) / a for a, b in ((norm[0], norm[1]), (norm[0], norm[2]), (norm[1], norm[2]))) > 0.01, norm


@pytest.mark.parametrize("clip", [0.1, 100.0, 0.0])
def test_adam_step_3(clip, warm, gpu):
    of, noise, state = warm
    _restore(of, state, 2)
    norm = _step_and_check(of, noise, clip, [3, 3, 3], f"step 3 clip {clip}")
    if clip == 0.1:
        assert (norm > clip).all(), norm          # the clip is active in every frame
        assert all(float(R.clip_coef(clip, x)) < 1 for x in norm)
    if clip == 100.0:
        assert all(float(R.clip_coef(clip, x)) == 1.0 for x in norm)


def test_adam_step_1(warm, gpu):
    """Bias corrections of the first step (1 - beta^1), on non-zero moments."""
    of, noise, state = warm
    _restore(of, state, 0)
    _step_and_check(of, noise, 0.1, [1, 1, 1], "step 1 clip 0.1")


def test_adam_latent_only(warm, gpu):
    of, noise, state = warm
    _restore(of, state, 2)
    _step_and_check(of, noise, 0.1, [3, 3, 3], "latent-only step 3", update="latent")


def test_adam_per_frame_steps_and_a_frozen_frame(warm, gpu):
    """Frames at their own Adam steps (t_adam_bc forms the bias corrections on the device); a frame
    whose step is <= 0 after the step's own increment stays as it is."""
    of, noise, state = warm
    _restore(of, state, 2, steps=[1, 6, -1])
    _step_and_check(of, noise, 0.1, [2, 7, 0], "per-frame steps [2, 7, frozen]", per_frame=True)
    assert of.steps.tolist() == [2, 7, 0]
