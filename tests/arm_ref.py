"""Float64 reference of the path-A ARM and rate, the inputs that take it off the rate clamp, and
a-priori error bounds for a float32 evaluation.  A helper: no tests in it.  tests/test_arm_ref.py
pins it on the CPU (goldens, the fp32 oracle, planted errors), tests/test_arm_rate_gpu.py compares
the HIP kernels with it.

Reference (`reference`): context (forward_oracle.context), residual MLP, mu, log_scale,
scale = exp(clamp(log_scale - 4, -4.6, 5)), p = F(q + .5) - F(q - .5) with the reference's
_laplace_cdf (forward_oracle.laplace_cdf), rate = -log2(max(p, 2^-16)), all in float64 on the
float32 weights as they are.  At the floor p = 2^-16 is the difference of two values near 0 or 1
that carry 1e-16 each: 1e-11 relative, against the 2.4e-7 * 2^16 = 1.6e-2 bits the fp32 form is
allowed there.

Bounds, per latent, for any fp32 evaluation of the same formulas, u = 2^-24:
  hidden layer   e_out_j = (d + 2) u (|a_j| + |b_j| + sum_i |w_ji| |a_i|) + sum_i (|W| + I)_ji e_in_i
                 the running bound of a sum of d + 2 terms rounded d + 2 times, in any order, with
                 or without fma; ReLU is 1-Lipschitz; e_in = 0 for the (integer) contexts
  output layer   the same with d + 1 and without the residual: e_mu, e_ls
  scale          e_scale = scale (e_ls + 2^-20); the clamp is 1-Lipschitz, and 2^-20 covers the
                 rounding of x log2(e) for |x| <= 5 (3e-7), one ulp of v_exp_f32 and the float32
                 value of -4.6 (1e-7 off)
  rate           tol_rate = 1e-4 + 2.4e-7 2^rate + 1.5 (e_mu + e_scale |q - mu| / scale) / (scale ln 2)
                 the first two terms and the 1.5 are those of tests/test_forward.py (the fp32
                 cancellation of p: two CDF values, one ulp of 1 each, over p ln 2); the
                 propagated part comes from e_mu and e_scale, not from a kernel's outputs
  total rate     |sum err| <= 1e-5 sum + 1e-3 (tests/test_forward.py)

Inputs (`make_case`): integer grids q ~ rint(sigma_q randn), latents float32((q + u) / 16) with
|u| <= 0.3 (rint(16 lat) == q, no ties), a random float32 ARM whose output layer is rescaled in
float64 on the case's own activations so that mu has standard deviation sigma_q / 2 and median 0
and log_scale the regime's standard deviation and median.  Regimes (sigma_q, median, sd):
  mid  (3, 4.5, 3)    rates spread over 0 .. 16 bits
  low  (3, -0.6, 2)   log_scale - 4 centred on the lower scale clamp, -4.6
  high (40, 9, 2)     centred on the upper one, 5
A GPU case (`batch_case`) is a batch of three frames, mid, low and high, each with its own latents
and its own weights."""
import functools

import numpy as np
import torch

import forward_oracle as fo

U = 2.0 ** -24
P_MIN = 2.0 ** -16
LN2 = float(np.log(2.0))
OUTS = ("mu", "log_scale", "scale", "rate")

# regime -> (sigma_q, median of log_scale, its standard deviation)
REGIMES = {"mid": (3.0, 4.5, 3.0), "low": (3.0, -0.6, 2.0), "high": (40.0, 9.0, 2.0)}
FRAMES = ("mid", "low", "high")

# frame (h, w), grids: the shapes of tests/test_arm_pairs.py, for the 8 x 64 tile with its 4-row,
# 4-column halo
SHAPES = {
    "1x1": ((1, 1), 1),
    "9x65": ((9, 65), 3),
    "23x40": ((23, 40), 7),
    "37x130": ((37, 130), 4),
}
ARMS = [(d, nh) for d in (8, 16, 24, 32) for nh in (0, 1, 2, 3)]      # what ccmi_arm_forward_f32 accepts
TRAIN_ARMS = [(8, 0), (16, 2), (24, 2), (32, 3)]                     # the training-form cases, at 37x130
MLP_HIDDEN = (0, 1, 2, 3, 4)                                          # what ccmi_arm_mlp_f32 accepts
MLP_GRIDS = {1: (1, 1), 255: (5, 51), 257: (1, 257)}                  # M -> the grid the contexts come from


def sizes_of(shape):
    (h, w), n = SHAPES[shape]
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def param_count(d, nh):
    return nh * (d * d + d) + 2 * d + 2


# ----------------------------------------------------------------------------- reference


def _f64(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float64) if not torch.is_tensor(x) else x.double()


def mlp(ctx, arm):
    """Residual MLP in float64 on contexts [N, d] with the running fp32 error bound alongside.
    Returns mu, log_scale, e_mu, e_ls (all [N]) and the largest |pre-activation|."""
    x = _f64(ctx)
    e = torch.zeros_like(x)
    pre_max = 0.0
    for W, b in arm[:-1]:
        W, b = W.double(), b.double()
        d = W.shape[1]
        z = x @ W.T + b + x
        mag = x.abs() @ W.abs().T + b.abs() + x.abs()
        e = (d + 2) * U * mag + e @ W.abs().T + e
        pre_max = max(pre_max, float(z.abs().max()))
        x = torch.relu(z)
    W, b = arm[-1][0].double(), arm[-1][1].double()
    d = W.shape[1]
    out = x @ W.T + b
    e_out = (d + 1) * U * (x.abs() @ W.abs().T + b.abs()) + e @ W.abs().T
    return out[:, 0], out[:, 1], e_out[:, 0], e_out[:, 1], pre_max


def scale_of(log_scale, lo=-4.6, hi=5.0):
    return torch.exp(torch.clamp(log_scale - 4.0, min=lo, max=hi))


def rate_of(q, mu, scale):
    p = fo.laplace_cdf(q + 0.5, mu, scale) - fo.laplace_cdf(q - 0.5, mu, scale)
    return -torch.log2(torch.clamp_min(p, P_MIN))


def bounds(q, mu, log_scale, scale, rate, e_mu, e_ls):
    """The per-latent bounds of the header from the reference's values."""
    e_scale = scale * (e_ls + 2.0 ** -20)
    tol_rate = 1e-4 + 2.4e-7 * torch.exp2(rate) + 1.5 * (e_mu + e_scale * (q - mu).abs() / scale) / (scale * LN2)
    return {"mu": e_mu, "log_scale": e_ls, "scale": e_scale, "rate": tol_rate}


def reference(q_grids, arm, dim_arm):
    """q_grids: integer latent grids [H_i, W_i]; arm: [(W, b), ...] float32 as the state_dict holds
    them.  Returns a dict of float64 numpy arrays over the flat latents: q, ctx [N, d], mu, log_scale,
    scale, rate, the bounds e_mu, e_ls, e_scale, tol_rate, and pre_max (largest |pre-activation|
    of a hidden layer)."""
    qs = [_f64(g) for g in q_grids]
    ctx = torch.cat([fo.context(g, dim_arm) for g in qs], dim=0)
    q = torch.cat([g.reshape(-1) for g in qs])
    mu, ls, e_mu, e_ls, pre_max = mlp(ctx, arm)
    scale = scale_of(ls)
    rate = rate_of(q, mu, scale)
    b = bounds(q, mu, ls, scale, rate, e_mu, e_ls)
    r = {"q": q, "ctx": ctx, "mu": mu, "log_scale": ls, "scale": scale, "rate": rate, "e_mu": b["mu"],
         "e_ls": b["log_scale"], "e_scale": b["scale"], "tol_rate": b["rate"]}
    r = {k: v.numpy() for k, v in r.items()}
    r["pre_max"] = pre_max
    return r


BOUND = {"mu": "e_mu", "log_scale": "e_ls", "scale": "e_scale", "rate": "tol_rate"}


def ratios(ref, got):
    """Worst error / bound per output of `got` (name -> array over the latents); for a rate also
    "total": |sum err| / (1e-5 sum + 1e-3).  A zero bound allows a zero error only."""
    out = {}
    for k, v in got.items():
        err = np.abs(np.asarray(v, np.float64) - ref[k])
        bnd = ref[BOUND[k]]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
        out[k] = float(np.max(np.where(np.isnan(r), np.inf, r)))
        if k == "rate":
            s = float(ref["rate"].sum())
            t = abs(float(np.asarray(v, np.float64).sum()) - s) / (1e-5 * s + 1e-3)
            out["total"] = t if np.isfinite(t) else np.inf
    return out


def check(ref, got, what=""):
    """Every output within its per-latent bound, the total rate within its own.  Returns the ratios."""
    r = ratios(ref, got)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return r


# ----------------------------------------------------------------------------- inputs


def make_case(dim_arm, n_hidden, sizes, seed, regime, sigma_q=None):
    """One frame: dict(q = integer grids (float64), lat = float32 latents with rint(16 lat) == q,
    arm = [(W, b), ...] float32, sizes, dim_arm, n_hidden, regime)."""
    sq, med, sd = REGIMES[regime]
    sq = float(sigma_q) if sigma_q is not None else sq
    d = dim_arm
    g = torch.Generator().manual_seed(seed)
    q = [torch.round(sq * torch.randn(h, w, generator=g, dtype=torch.float64)) for h, w in sizes]
    lat = [((x + 0.6 * (torch.rand(x.shape, generator=g, dtype=torch.float64) - 0.5)) / 16.0).float() for x in q]
    for x, y in zip(q, lat):
        assert torch.equal(torch.round(16.0 * y).double(), x)
    arm = [((0.5 * torch.randn(d, d, generator=g, dtype=torch.float64) / d).float(),
            (0.5 * torch.randn(d, generator=g, dtype=torch.float64)).float()) for _ in range(n_hidden)]
    # the output layer, rescaled on the case's own last hidden activations
    x = torch.cat([fo.context(t, d) for t in q], dim=0)
    for W, b in arm:
        x = torch.relu(x @ W.double().T + b.double() + x)
    w = torch.randn(2, d, generator=g, dtype=torch.float64)
    want_sd = torch.tensor([0.5 * sq, sd], dtype=torch.float64)
    want_med = torch.tensor([0.0, med], dtype=torch.float64)
    n = x.shape[0]
    have_sd = (x @ w.T).std(dim=0) if n >= 9 else torch.full((2,), sq * d ** 0.5, dtype=torch.float64)
    w = (w * (want_sd / have_sd)[:, None]).float()
    t = x @ w.double().T
    b = (want_med - (t.median(dim=0).values if n >= 9 else torch.zeros(2, dtype=torch.float64))).float()
    arm.append((w, b))
    return {"q": q, "lat": lat, "arm": arm, "sizes": list(sizes), "dim_arm": d, "n_hidden": n_hidden,
            "regime": regime}


_SEED_KEYS = ("1x1", "9x65", "23x40", "37x130", "1", "255", "257", "large")
# cases whose first seed missed a coverage condition of tests/test_arm_ref.py (771 latents pooled:
# the first seed of (8, 1) at M = 257 left 0.422 of them at the floor, 0.40 is allowed)
_RESEED = {(8, 1, "257"): 5}


def _seed(d, nh, key, k):
    """Frame k of the case `key` (a shape, an M of the MLP cases, or the large-q case)."""
    return 100000 * (1 + _SEED_KEYS.index(key)) + 1000 * d + 10 * nh + k + _RESEED.get((d, nh, key), 0)


@functools.lru_cache(maxsize=None)
def batch_case(d, nh, shape):
    """The three frames (mid, low, high) of a GPU case and their references: [(case, ref)] * 3."""
    out = []
    for k, regime in enumerate(FRAMES):
        c = make_case(d, nh, sizes_of(shape), _seed(d, nh, shape, k), regime)
        out.append((c, reference(c["q"], c["arm"], d)))
    return out


@functools.lru_cache(maxsize=None)
def mlp_case(d, nh, m):
    """As batch_case on the single grid MLP_GRIDS[m] (M = m contexts), for ccmi_arm_mlp_f32."""
    out = []
    for k, regime in enumerate(FRAMES):
        c = make_case(d, nh, [MLP_GRIDS[m]], _seed(d, nh, str(m), k), regime)
        out.append((c, reference(c["q"], c["arm"], d)))
    return out


@functools.lru_cache(maxsize=None)
def large_q_case():
    """(16, 2) at 37x130, the high regime with sigma_q = 2000: |q| reaches about 10^4, which the
    pairs form's scaled ReLU carries times 2^-32."""
    c = make_case(16, 2, sizes_of("37x130"), _seed(16, 2, "large", 0), "high", sigma_q=2000.0)
    return c, reference(c["q"], c["arm"], 16)


def flat(grids):
    return torch.cat([g.reshape(-1) for g in grids])


def pack_arm(arm, pad=0, fill=float("nan")):
    """[(W, b), ...] -> flat float32 in ccmi_arm_args.params order, plus `pad` values of `fill`."""
    p = torch.cat([t.reshape(-1).float() for wb in arm for t in wb])
    return torch.cat([p, torch.full((pad,), fill)]) if pad else p


# ----------------------------------------------------------------------------- coverage


def coverage(frames):
    """Shares the coverage conditions speak of, from the references of a (mid, low, high) batch."""
    mid, low, high = (r for _, r in frames)
    rate = np.concatenate([r["rate"] for _, r in frames])
    share = lambda m: float(np.mean(m))  # noqa: E731
    return {
        "mid_floor": share(mid["rate"] >= 16.0),
        "low_cross": share(low["log_scale"] - 4.0 < -4.6),
        "high_cross": share(high["log_scale"] - 4.0 > 5.0),
        "r0_1": share(rate < 1.0), "r1_4": share((rate >= 1.0) & (rate < 4.0)),
        "r4_8": share((rate >= 4.0) & (rate < 8.0)), "r8_16": share((rate >= 8.0) & (rate < 16.0)),
        "floor": share(rate >= 16.0),
    }
