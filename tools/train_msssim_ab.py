"""What the MS-SSIM stage costs inside the overfit step, and the standalone call's time.

One process, 8 frames of 512 x 768 (4:2:0, hop architecture), alternating legs in an order rotated
from round to round, medians of 9 timings of 10 steps each (device events), the whole comparison twice:
  a  ccmi_train_step of the library built from the parent commit (--base PATH, required)
  b  ccmi_train_step of this library
  c  ccmi_train_step_dist with alpha_mse = 0, beta_ms = 1
  d  the composed route: forward_only (raw_out), the float32 restatement (tests/msssim_ref.py) with
     autograd as torch operations on the GPU, then the grad_raw step
Then ccmi_msssim_f32 on --frames frames of 720p (default 960), one shared target: value alone, value
and gradient.  python tools/train_msssim_ab.py --base tools/ablib/libccmi_base.so [--out FILE] [--order bacd]"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in ("cool-chic_amd", "oracle", "tests"):
    sys.path.insert(0, str(ROOT / p))

from ccmi import metrics as M  # noqa: E402
from ccmi import train as T  # noqa: E402
import msssim_ref as R  # noqa: E402

H, W, B, STEPS, ROUNDS = 512, 768, 8, 10, 9


def make(dev, distortion=None):
    import forward_oracle as fo
    arch = T.Arch(H, W)
    rows = []
    for b in range(B):
        mp = fo.ModelParams.random(H, W, seed=b)
        rows.append(T.pack_params(mp.arm, mp.ups_half, mp.pre_half, mp.syn))
    g = torch.Generator().manual_seed(0)
    lat = 0.01 * torch.randn(B, arch.n_latents, generator=g)
    tgt = torch.rand(B, H * W + 2 * (H // 2) * (W // 2), generator=g)
    return T.Overfitter(arch, lat.to(dev), torch.stack(rows).to(dev), tgt.to(dev), yuv420=True, seed=1, distortion=distortion)


def args_of(of, **kw):
    """ccmi_train_args of one updating step, as Overfitter.step fills them"""
    of.t += 1
    a = of._args()
    a.adam_m, a.adam_v = of.m.data_ptr(), of.v.data_ptr()
    a.quantizer, a.noise = T.Q_TYPES["softround"], T.NOISE_TYPES["kumaraswamy"]
    a.temperature, a.noise_param, a.lmbda = 0.3, 2.0, 1e-3
    a.lr, a.beta1, a.beta2, a.eps, a.clip = 1e-2, 0.9, 0.999, 1e-8, 0.1
    a.step, a.seed, a.update = of.t, 1, 1
    a.loss_out = of.loss.data_ptr()
    a.workspace, a.workspace_bytes = of.ws.data_ptr(), of.ws.numel()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=960)
    ap.add_argument("--order", default="abcd", help="the order of the legs in the first round; each later round starts one leg "
                    "further (the leg after d measured 5 %% slower in a fixed order, whichever leg it was)")
    o = ap.parse_args()
    dev = torch.device("cuda:0")
    new = T._bind()
    base = C.CDLL(str((ROOT / o.base).resolve()))
    base.ccmi_train_step.argtypes = [C.POINTER(T.TrainArgs), C.c_void_p]
    base.ccmi_train_step.restype = C.c_int
    assert not hasattr(base, "ccmi_train_step_dist"), "--base must be the parent commit's library"
    stream = torch.cuda.current_stream(dev).cuda_stream
    D = M.Distortion(0.0, 1.0, n_scales=5)
    ofs = {k: make(dev, D if k in "cd" else None) for k in "abcd"}
    dstruct = D.train_struct(True, ofs["c"].dist)
    raw = torch.empty(B, 3, H, W, device=dev)
    sizes = M.plane_sizes(H, W, True)

    def leg_a():
        assert base.ccmi_train_step(C.byref(args_of(ofs["a"])), stream) == 0

    def leg_b():
        assert new.ccmi_train_step(C.byref(args_of(ofs["b"])), stream) == 0

    def leg_c():
        assert new.ccmi_train_step_dist(C.byref(args_of(ofs["c"])), C.byref(dstruct), stream) == 0

    def leg_d():
        of = ofs["d"]
        a = args_of(of, forward_only=1, raw_out=raw, update=0)
        of.t -= 1
        assert new.ccmi_train_step(C.byref(a), stream) == 0
        x = raw.detach().requires_grad_(True)
        Xs = [x[:, 0], x[:, 1, ::2, ::2][:, :H // 2, :W // 2], x[:, 2, ::2, ::2][:, :H // 2, :W // 2]]
        Ys, p = [], 0
        for h, w in sizes:
            Ys.append(of.targets[:, p:p + h * w].view(B, h, w))
            p += h * w
        out, _ = R.evaluate(Xs, Ys, 5, D.scale_weights(), D.plane_weights(True), 0.0, 1.0)
        g, = torch.autograd.grad(out[:, 0].sum(), x)
        assert new.ccmi_train_step(C.byref(args_of(of, grad_raw=g.contiguous())), stream) == 0

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
    legs = {k: legs[k] for k in o.order}
    lines = [f"train_msssim_ab: {B} frames of {H} x {W}, 4:2:0, {STEPS} steps per timing, medians of {ROUNDS}, "
             f"order {o.order}, device {torch.cuda.get_device_name(dev)}"]
    for f in legs.values():  # warm up every leg
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for run in range(2):
        ms = {k: [] for k in legs}
        for r in range(ROUNDS):
            keys = list(legs)
            keys = keys[r % len(keys):] + keys[:r % len(keys)]  # rotated: every leg takes every place in a round
            for k in keys:
                f = legs[k]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(STEPS):
                    f()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / STEPS)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, name in (("a", "parent ccmi_train_step"), ("b", "this ccmi_train_step"), ("c", "ccmi_train_step_dist beta 1"),
                        ("d", "forward_only + torch MS-SSIM + grad_raw step")):
            lines.append(f"run {run} leg {k} {name:46s} median {med[k]:.3f} ms/step  min {min(ms[k]):.3f} max {max(ms[k]):.3f}")
        lines.append(f"run {run} stage cost c - b = {med['c'] - med['b']:.3f} ms/step; b inside a's spread: "
                     f"{min(ms['a']) <= med['b'] <= max(ms['a'])}; c < d: {med['c'] < med['d']}")
    lines.append(f"D of leg c after its steps: {ofs['c'].dist[:, 0].tolist()}")
    del ofs, raw
    torch.cuda.empty_cache()

    # standalone: frames of 720p against one target
    n, h, w = o.frames, 720, 1280
    y = torch.rand(3 * h * w, device=dev)
    x = (y.view(1, 3, h, w) + 0.03 * torch.randn(n, 3, h, w, device=dev)).contiguous()
    g = torch.empty_like(x)
    d5 = M.Distortion(0.3, 0.7, n_scales=5)
    for name, grad in (("value", False), ("value and gradient", g)):
        t = []
        for i in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            M.distortion(x, y, d5, grad=grad)  # includes the workspace allocation (cached after the first call)
            e1.record()
            torch.cuda.synchronize()
            if i:
                t.append(e0.elapsed_time(e1))
        lines.append(f"standalone {n} frames of {w} x {h} 4:4:4, 5 scales, {name}: median {statistics.median(t):.2f} ms "
                     f"(min {min(t):.2f} max {max(t):.2f}) = {statistics.median(t) / n * 1e3:.1f} us per frame")
    text = "\n".join(lines)
    print(text)
    if o.out:
        Path(o.out).parent.mkdir(parents=True, exist_ok=True)
        Path(o.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
