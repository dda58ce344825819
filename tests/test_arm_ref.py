"""Pins tests/arm_ref.py on the CPU, so that a wrong reference cannot hide a wrong kernel: the
float64 reference against the goldens of the reference implementation, the torch fp32 oracle
inside the a-priori bounds on every generated case, the coverage conditions of every case the GPU
tests (tests/test_arm_rate_gpu.py) use, and five planted errors the bounds must reject.

Shares of the bounds the torch fp32 oracle reaches over all cases (16 ARMs x 4 shapes x 3 frames,
the MLP cases, the large-q case): mu 0.36, log_scale 0.24, scale 0.19, rate 0.47, total 0.47."""
import numpy as np
import pytest
import torch

import arm_ref as R
import forward_oracle as fo

GOLDEN = fo.golden_files()
assert GOLDEN, "tests/golden/forward_*.npz missing"


@pytest.mark.parametrize("path", GOLDEN, ids=[p.stem for p in GOLDEN])
def test_reference_matches_golden(path):
    """mu, scale, log_scale and rate of the reference implementation (fp32) lie within the bounds
    around the float64 reference."""
    z = np.load(path)
    mp = fo.ModelParams.from_npz(z)
    ref = R.reference([z[f"q{i}"] for i in range(mp.n_grids)], mp.arm, mp.dim_arm)
    r = R.check(ref, {k: z[k] for k in R.OUTS}, path.stem)
    print(path.stem, {k: round(v, 3) for k, v in r.items()})


def _fp32_oracle(c):
    q = [x.float() for x in c["q"]]
    ctx = torch.cat([fo.context(x, c["dim_arm"]) for x in q])
    mu, sc, ls = fo.arm_mlp(ctx, c["arm"])
    r = fo.rate(R.flat(q), mu, sc)
    return {"mu": mu.numpy(), "log_scale": ls.numpy(), "scale": sc.numpy(), "rate": r.numpy()}


def _frames(d, nh):
    """Every frame the GPU tests run for this ARM (dim_arm, n_hidden), as (name, case, ref)."""
    for shape in R.SHAPES:
        if nh <= 3:
            for c, ref in R.batch_case(d, nh, shape):
                yield f"{shape} {c['regime']}", c, ref
    for m in R.MLP_GRIDS:
        for c, ref in R.mlp_case(d, nh, m):
            yield f"M={m} {c['regime']}", c, ref
    if (d, nh) == (16, 2):
        yield ("large q",) + R.large_q_case()


@pytest.mark.parametrize("nh", R.MLP_HIDDEN)
@pytest.mark.parametrize("d", [8, 16, 24, 32])
def test_fp32_oracle_within_bounds(d, nh):
    worst = {}
    for name, c, ref in _frames(d, nh):
        for x, y in zip(c["q"], c["lat"]):   # rint(16 lat) == q, no ties
            assert y.dtype == torch.float32 and float((16.0 * y.double() - x).abs().max()) <= 0.31
        for k, v in R.check(ref, _fp32_oracle(c), f"({d}, {nh}) {name}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"({d}, {nh}) fp32 oracle, worst error / bound:", {k: round(v, 3) for k, v in worst.items()})


def _coverage_ok(frames, what):
    c = R.coverage(frames)
    assert c["mid_floor"] <= 0.30, (what, c)
    assert 0.3 <= c["low_cross"] <= 0.7, (what, c)
    assert 0.3 <= c["high_cross"] <= 0.7, (what, c)
    assert c["r0_1"] >= 0.03 and c["r1_4"] >= 0.05 and c["r4_8"] >= 0.15 and c["r8_16"] >= 0.20, (what, c)
    assert c["floor"] <= 0.40, (what, c)


@pytest.mark.parametrize("nh", R.MLP_HIDDEN)
@pytest.mark.parametrize("d", [8, 16, 24, 32])
def test_gpu_cases_leave_the_clamps(d, nh):
    """The coverage conditions, on the reference alone, for every three-frame case of the GPU
    tests but the 1x1 shape (a single latent): the mid frame off the rate floor, the low and high
    frames astride their scale clamp, every rate range populated.  (The large-q case is a high
    frame alone, there for the scaled ReLU: nearly all of its latents sit on the floor.)"""
    if nh <= 3:
        for shape in R.SHAPES:
            if shape != "1x1":
                _coverage_ok(R.batch_case(d, nh, shape), (d, nh, shape))
    for m in R.MLP_GRIDS:
        if m != 1:
            _coverage_ok(R.mlp_case(d, nh, m), (d, nh, m))


def test_large_q_case_fits_the_scaled_relu():
    c, ref = R.large_q_case()
    assert np.abs(ref["q"]).max() >= 5000
    assert ref["pre_max"] < 2.0 ** 32


# ----------------------------------------------------------------------------- planted errors


def _context_with(q, index):
    H, W = q.shape
    qp = torch.nn.functional.pad(q, (4, 4, 4, 4))
    return torch.stack([qp[k // 9:k // 9 + H, k % 9:k % 9 + W].reshape(-1) for k in index], dim=1)


def _planted(name, c, ref):
    """Outputs computed in float64 like the reference, with one error planted."""
    t = {k: torch.from_numpy(ref[k]) for k in ("q", "mu", "log_scale", "scale")}
    q, mu, ls, scale = t["q"], t["mu"], t["log_scale"], t["scale"]
    if name == "half_swapped":
        p = fo.laplace_cdf(q - 0.5, mu, scale) - fo.laplace_cdf(q + 0.5, mu, scale)
        return {"rate": -torch.log2(torch.clamp_min(p, R.P_MIN))}
    if name == "lower_clamp_4.5":
        s = R.scale_of(ls, lo=-4.5)
        return {"scale": s, "rate": R.rate_of(q, mu, s)}
    if name == "upper_clamp_4":
        s = R.scale_of(ls, hi=4.0)
        return {"scale": s, "rate": R.rate_of(q, mu, s)}
    if name == "context_column":
        index = list(fo.CTX_INDEX[c["dim_arm"]])
        index[0] -= 1   # the first context pixel, one column to the left
        ctx = torch.cat([_context_with(g, index) for g in c["q"]])
        mu, ls = R.mlp(ctx, c["arm"])[:2]
        s = R.scale_of(ls)
        return {"mu": mu, "log_scale": ls, "scale": s, "rate": R.rate_of(q, mu, s)}
    if name == "mu_of_previous":
        mu = torch.roll(mu, 1)
        return {"mu": mu, "rate": R.rate_of(q, mu, scale)}
    raise KeyError(name)


@pytest.mark.parametrize("name,broken", [("half_swapped", "rate"), ("lower_clamp_4.5", "scale"),
                                         ("upper_clamp_4", "scale"), ("context_column", "mu"),
                                         ("mu_of_previous", "mu")])
def test_bounds_reject_planted_error(name, broken):
    """Each error breaks a bound on the mid frame of the (16, 2) 37x130 case: the output it
    touches first, and the rate."""
    c, ref = R.batch_case(16, 2, "37x130")[0]
    assert c["regime"] == "mid"
    got = {k: v.numpy() for k, v in _planted(name, c, ref).items()}
    r = R.ratios(ref, got)
    print(name, {k: float(f"{v:.3g}") for k, v in r.items()})
    assert r[broken] > 1.0 and r["rate"] > 1.0, r
    with pytest.raises(AssertionError):
        R.check(ref, got)
