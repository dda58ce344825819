"""ccmi_quantize_f32 (t_quant of train.hip at gain 1: the kernel whose dq multiplies every latent
gradient of the training step) against its float64 restatement, tests/quant_ref.py: every
quantiser type at the temperatures of the c3x schedule (0.3, 0.2, 0.1, and 1e-4 for ste and
softround_alone), on input sets that hold the ties of rintf, the neighbours of the integers and
halves, the derivative's peak and tails at the temperature, and magnitudes up to 2^24.

Bounds (header of tests/quant_ref.py): |d - d64| <= 16 max(e32_d, 2^-22) max |d64| and
|y - y64| <= 16 max(e32_y, 2^-22) max(1, |y64|) at every entry, e32 the restatement's own float32
distance on the set; for none, true_ste and hardround d is equal and y within one rounding, and
y = rint(x) of the three hard-rounding types is equal bit for bit, the sign of zero included.

Worst error / bound on an MI355X over the input sets (the bounds are not to be tightened to these),
with the restatement's own e32_d / e32_y there (largest over the sets; 2^-22 = 2.4e-7 is the floor):
  type, T                          e32_d            e32_y            d      y
  softround_alone 0.3 / 0.2 / 0.1  1.4e-7 .. 1.7e-7 9.5e-8 .. 1.2e-7 0.044  0.030
  softround_alone 1e-4             1.2e-7           8.3e-8           0.019  0.021
  softround 0.3 / 0.2 / 0.1        2.3e-6 .. 3.1e-6 3.4e-7 .. 9.6e-7 0.109  0.092   (minus2^23: e32_d 6.5 .. 5500)
  ste 0.3 / 0.2 / 0.1              1.4e-7 .. 1.7e-7 0 (y equal)      0.044  equal
  ste 1e-4                         1.2e-7           0                0.019  equal
  none, true_ste, hardround        d equal, y equal (none with noise: one rounding, 0.016 of the bound)
  lengths 255 / 256 / 257          softround 0.062 (d), 0.104 (y); ste 0.030 (d)
  mirror quantize(), 0.1, sigma .1 4.3e-6           4.7e-7           0.063  0.062
Where the ratio is 0.062 = 1 / 16 the kernel's worst entry is exactly as far from float64 as numpy's
float32 evaluation is.  The 31 tests take 2.5 s together.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import quant_ref as Q

pytestmark = pytest.mark.gpu

TEMPS = (0.3, 0.2, 0.1)
MATRIX = [(q, T) for q in Q.QTYPES for T in TEMPS] + [("ste", 1e-4), ("softround_alone", 1e-4)]


@pytest.fixture(scope="module")
def quant(gpu):
    from ccmi import check
    from ccmi.train import Q_TYPES, _bind
    L = _bind()
    L.ccmi_quantize_f32.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
    L.ccmi_quantize_f32.restype = C.c_int

    def run(x, qtype, T, noise=None, y=None, dy=None, n=None, want_dy=True):
        """x, noise: float32 arrays; returns (y, dy) as float32 arrays (dy None if not asked for).
        y / dy: device canvases to write into (n entries of them)."""
        xg = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)
        ng = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(gpu)
        n = xg.numel() if n is None else n
        yg = torch.full_like(xg, float("nan")) if y is None else y
        dg = (torch.full_like(xg, float("nan")) if dy is None else dy) if want_dy else None
        check(L.ccmi_quantize_f32(xg.data_ptr(), n, Q_TYPES[qtype], float(T), None if ng is None else ng.data_ptr(),
                                  yg.data_ptr(), None if dg is None else dg.data_ptr(),
                                  torch.cuda.current_stream(gpu).cuda_stream))
        torch.cuda.synchronize()
        return yg.cpu().numpy(), None if dg is None else dg.cpu().numpy()
    return run


def _check(qtype, T, name, x, n, y, d):
    """(y, d) of the kernel against the restatement on one set; returns the error / bound ratios."""
    y64, d64, by, bd, e_y, e_d = Q.bounds(x, qtype, T, n)
    what = (qtype, T, name, "noise" if n is not None else "no noise")
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(d)), what
    ry = float((np.abs(y - y64) / by).max())
    rd = float(np.abs(d - d64).max()) / bd if bd > 0 else 0.0
    print(f"  {name:10s} {'noise' if n is not None else '-':5s} e32_y {e_y:.2e} e32_d {e_d:.2e}  "
          f"error / bound: y {ry:.3f} d {rd:.3f}")
    assert ry <= 1.0, (what, "y", ry, int((np.abs(y - y64) / by).argmax()))
    if bd > 0:
        assert rd <= 1.0, (what, "d", rd, int(np.abs(d - d64).argmax()))
    if qtype in Q.TRIVIAL:
        assert np.array_equal(d, d64.astype(np.float32)), what
        assert np.all(np.abs(y - y64) <= 2.0 ** -24 * np.abs(y64)), what     # one rounding (none: x + n)
    if qtype in Q.HARD:
        assert np.array_equal(y, y64.astype(np.float32)) and np.array_equal(np.signbit(y), np.signbit(y64)), what
    return ry, rd


@pytest.mark.parametrize("qtype,T", MATRIX)
def test_quantize_matches_the_float64_restatement(qtype, T, quant):
    print(f"\n{qtype} T = {T}")
    for name, (x, n) in Q.sets_for(qtype, T).items():
        # noise as a tensor where the type adds it, and none for every type
        for noise in ((n, None) if qtype in ("none", "softround") else (None,)):
            y, d = quant(x, qtype, T, noise)
            _check(qtype, T, name, x, noise, y, d)
    if qtype not in ("none", "softround"):
        # a noise tensor given to a type that adds none changes nothing
        x, n = Q.input_sets(T)["randn3"]
        a, b = quant(x, qtype, T, None), quant(x, qtype, T, n)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("qtype", Q.QTYPES)
def test_the_derivative_is_optional(qtype, quant):
    """dy = NULL: the same y, bit for bit."""
    x, n = Q.input_sets(0.2)["randn3"]
    noise = n if qtype in ("none", "softround") else None
    y, d = quant(x, qtype, 0.2, noise)
    y0, d0 = quant(x, qtype, 0.2, noise, want_dy=False)
    assert d0 is None and d is not None
    assert np.array_equal(y.view(np.uint32), y0.view(np.uint32))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_nothing_is_written_past_n(n, quant, gpu):
    """One workgroup is 256 threads: n on either side of it, into canvases of a sentinel."""
    x, nz = Q.input_sets(0.1)["randn3"]
    x, nz = x[:1024], nz[:1024]
    sent = -12345.0
    for qtype in ("softround", "ste"):
        y = torch.full((1024,), sent, device=gpu)
        dy = torch.full((1024,), sent, device=gpu)
        yh, dh = quant(x, qtype, 0.1, nz, y=y, dy=dy, n=n)
        assert np.all(yh[n:] == sent) and np.all(dh[n:] == sent), (qtype, n)
        ya, da = quant(x[:n], qtype, 0.1, nz[:n])
        assert np.array_equal(yh[:n], ya) and np.array_equal(dh[:n], da), (qtype, n)
        if n > 1:   # (a set of one value has no scale of its own: max |d64| is that value's)
            _check(qtype, 0.1, f"n={n}", x[:n], nz[:n] if qtype == "softround" else None, yh[:n], dh[:n])


def test_mirror_quantize_at_the_end_of_the_main_phase(gpu):
    """coolchic.enc.component.core.quantizer.quantize (the autograd function over the same kernel) at
    T = 0.1, softround + gaussian noise of sigma 0.1: value and x.grad to the bounds above, the
    noise drawn again from the same torch generator state."""
    from coolchic.enc.component.core.quantizer import draw_noise, quantize
    T, sigma = 0.1, 0.1
    x = torch.from_numpy(Q.input_sets(T)["randn3"][0]).to(gpu)
    xg = x.clone().requires_grad_(True)
    torch.manual_seed(7)
    y = quantize(xg, "gaussian", "softround", torch.tensor(T), torch.tensor(sigma))
    y.sum().backward()
    torch.manual_seed(7)
    nz = draw_noise(x, "gaussian", torch.tensor(sigma))
    assert 0.05 < float(nz.std()) < 0.2
    print()
    _check("softround", T, "mirror", x.cpu().numpy(), nz.cpu().numpy(), y.detach().cpu().numpy(), xg.grad.cpu().numpy())
