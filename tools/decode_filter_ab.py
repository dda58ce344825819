"""A/B of the filter stage of the decoder's output stage (LatentStore.render_model(blur=..., solarize=...):
a per-frame Gaussian blur and a per-frame solarize after the colour ops, the GaussianBlur /
RandomSolarize steps of the self-supervised recipes) against the path it replaces, on one GPU, in one
process, legs alternating, in the form of tools/decode_colour_ab.py and on its workload: the bench's
`bitexact_decode` set (the 15 committed class-E 1280x720 streams x 64 = 960 frames) held in an int16
LatentStore, RandomResizedCrop regions resampled to 224 x 224, decode.colour_jitter(n, 0.4, 0.4, 0.4,
0.1), RGB, ImageNet mean / std, bfloat16 -- plus decode.gaussian_blur(n, 23, p=0.5) and
decode.random_solarize(n, p=0.2) (all seeded).
  N   store.render_model(roi=..., size=(224, 224), colour_ops=..., blur=..., solarize=..., mean=...,
      std=..., dtype=bfloat16)
  C   the composed path: the same call without a filter in float32 (mean 0, std 1), then as torch
      operations: the blurred frames gathered, reflect-padded and put through one grouped convolution
      per axis with their own 23 taps ([m x 3] groups), clamped and scattered back; solarize on the
      frames that have a threshold; then * scale + bias and the cast to bfloat16.
  P   N without blur and solarize (the call of the colour row): what the filter stage adds.
Warm-up rounds of all legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a
device synchronise.  Reported per leg: median and range of the time per call and of the tail's device
time (decode.last_timing()), the peak of torch's allocated bytes above what was allocated before the
leg (store and workspaces are the caller's, allocated before) and the tail groups.  N against C: the
share of bf16 elements that differ and by how many bf16 steps (N follows the contract's float32 order,
torch's convolution its own: counted, not asserted).

--mode regress: the call without a filter -- render_model(roi=..., size=(224, 224), colour_ops=...)
through the C ABI (ccmi_latents_render_col) of two libraries in one process, alternating, under the
rule of profiles/decode_split_ab.txt: the new library's median of block medians must lie inside the
parent's own spread of block medians, and the outputs must be equal in every element.

Run each mode twice; the report is appended to --out."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decode_colour_ab as col_ab  # noqa: E402
import decode_resample_ab as rs_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H
KSIZE = 23


def workload(n):
    rects = rs_ab.rrc_rects(n, np.random.default_rng(17))
    ops = decode.colour_jitter(n, 0.4, 0.4, 0.4, 0.1, generator=torch.Generator().manual_seed(29))
    blur = decode.gaussian_blur(n, KSIZE, p=0.5, generator=torch.Generator().manual_seed(31))
    sol = decode.random_solarize(n, 0.5, 0.2, generator=torch.Generator().manual_seed(37))
    return rects, ops, blur, sol


def torch_filter(x, blur, sol):
    """blur and solarize of every frame of x [n, 3, h, w] (float32), as torch operations."""
    dev = x.device
    js = [j for j, t in enumerate(blur) if t is not None]
    if js:
        r = KSIZE // 2
        idx = torch.tensor(js, device=dev)
        half = torch.from_numpy(np.stack([blur[j] for j in js])).to(dev)           # [m, r + 1]
        full = torch.cat([half[:, 1:].flip(1), half], dim=1)                        # [m, k]
        wgt = full.repeat_interleave(3, dim=0)                                      # [3 m, k]
        sub = x.index_select(0, idx)
        m, _, h, w = sub.shape
        sub = sub.reshape(1, 3 * m, h, w)
        sub = torch.nn.functional.conv2d(torch.nn.functional.pad(sub, (r, r, 0, 0), mode="reflect"),
                                         wgt.view(3 * m, 1, 1, KSIZE), groups=3 * m)
        sub = torch.nn.functional.conv2d(torch.nn.functional.pad(sub, (0, 0, r, r), mode="reflect"),
                                         wgt.view(3 * m, 1, KSIZE, 1), groups=3 * m)
        x.index_copy_(0, idx, sub.reshape(m, 3, h, w).clamp_(0, 1))
    js = [j for j, t in enumerate(sol) if t is not None and t <= 1.0]
    if js:
        idx = torch.tensor(js, device=dev)
        th = torch.tensor([float(sol[j]) for j in js], device=dev).view(-1, 1, 1, 1)
        sub = x.index_select(0, idx)
        x.index_copy_(0, idx, torch.where(sub >= th, 1.0 - sub, sub))
    return x


def bf16_steps(a, b):
    """|a - b| in bf16 steps: the distance of the two bit patterns on the monotonic integer line"""
    def line(t):
        v = t.view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(v >= 0x8000, 0x8000 - v, v)
    return (line(a) - line(b)).abs()


def mode_filter(a, streams):
    n = len(streams)
    rects, ops, blur, sol = workload(n)
    store = decode.LatentStore(streams, dtype=torch.int16)
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    need_p = store.render_model_workspace_bytes(roi=rects, size=OUT, colour_ops=ops)
    need_n = store.render_model_workspace_bytes(roi=rects, size=OUT, colour_ops=ops, blur=blur, solarize=sol)
    ws = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")
    fmt = dict(mean=MEAN, std=STD, dtype=torch.bfloat16)

    def leg_new():
        out = store.render_model(roi=rects, size=OUT, colour_ops=ops, blur=blur, solarize=sol, workspace=ws, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_plain():
        out = store.render_model(roi=rects, size=OUT, colour_ops=ops, workspace=ws, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_composed():
        x = store.render_model(roi=rects, size=OUT, colour_ops=ops, dtype=torch.float32, workspace=ws)
        groups, tail = decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]
        x = torch_filter(x, blur, sol)
        return (x * scale + bias).to(torch.bfloat16), groups, tail

    legs = {"N": leg_new, "C": leg_composed, "P": leg_plain}
    rec = {k: {"wall": [], "tail": [], "peak": []} for k in legs}
    last, groups = {}, {}
    for it in range(a.warmup + a.reps):
        for k, fn in legs.items():
            last[k] = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            last[k], groups[k], tail = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                rec[k]["wall"].append(1e3 * dt)
                rec[k]["tail"].append(tail)
                rec[k]["peak"].append(torch.cuda.max_memory_allocated() - base)
    names = {"N": "N  render_model(size=, colour_ops=, blur=, solarize=)       ",
             "C": "C  render_model(size=, colour_ops=, float32) + torch ops    ",
             "P": "P  render_model(size=, colour_ops=), no filter (unchanged)  "}
    nb, ns = sum(t is not None for t in blur), sum(t is not None for t in sol)
    staged = sum(b is not None or s is not None for b, s in zip(blur, sol))
    lines = ["filter stage A/B: LatentStore.render_model(size=..., colour_ops=..., blur=..., solarize=...) against the same call "
             "without a filter in float32 + the blur and solarize as torch operations, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; RandomResizedCrop regions -> "
             f"{OUT[0]}x{OUT[1]}; colour_jitter(0.4, 0.4, 0.4, 0.1); gaussian_blur({KSIZE}, p=0.5): {nb} frames; "
             f"random_solarize(p=0.2): {ns} frames; {staged} frames take the stage; bf16 RGB normalised; median [min .. max] of "
             f"{a.reps} repetitions after {a.warmup} warm-up rounds; workspace (caller-owned, not in the peaks): "
             f"{need_n / 2**20:.1f} MiB with the filter, {need_p / 2**20:.1f} MiB without ({need_n - need_p} bytes more)"]
    for k in legs:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    steps = bf16_steps(last["N"], last["C"])
    diff, total = int((steps != 0).sum()), steps.numel()
    hist = ", ".join(f"{k} step{'s' if k > 1 else ''}: {int((steps == k).sum())}" for k in (1, 2, 3))
    lines.append(f"  N against C: {diff} of {total} bf16 elements differ ({100.0 * diff / total:.3f} %); {hist}; more than 3: "
                 f"{int((steps > 3).sum())}; largest {int(steps.max())} steps")
    keep = [j for j, (b, s) in enumerate(zip(blur, sol)) if b is None and s is None]
    same = bool((last["N"][keep].view(torch.int16) == last["P"][keep].view(torch.int16)).all())
    lines.append(f"  the {len(keep)} frames that do not take the stage: N equal to P in every element: {same}")
    store.close()
    return lines


class RawStoreCol(col_ab.RawStoreRs):
    """col_ab.RawStoreRs with the colour row's call: the resampling render with colour ops, ccmi_latents_render_col."""

    def __init__(self, path, streams, rects, dtype, ops):
        super().__init__(path, streams, rects, dtype)
        P, I, Z = C.c_void_p, C.c_int, C.c_size_t
        L, n = self.L, self.n
        L.ccmi_latents_render_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
        L.ccmi_latents_render_col.argtypes = [P, P, I, P, P, P, P, P, P, P, I, I, P, Z, P]
        self.col, self.keep_col = decode._colour(ops, n)
        geom, need = (rs_ab.Geom * n)(), C.c_size_t(0)
        self.ok(L.ccmi_latents_render_col_plan(self.h, None, n, self.rects, 0, 0, C.byref(self.fmt), C.byref(self.rs), None,
                                               C.byref(self.col), geom, None, None, C.byref(need)))
        self.need = need.value
        self.ws = None
        self.ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")

    def render(self):
        self.ok(self.L.ccmi_latents_render_col(self.h, None, self.n, self.rects, self.op, self.cap, C.byref(self.fmt),
                                               C.byref(self.rs), None, C.byref(self.col), 0, 0, self.ws.data_ptr(),
                                               self.ws.numel(), self.stream))


def mode_regress(a, streams):
    if not a.parent or not Path(a.parent).exists():
        sys.exit("decode_filter_ab: --mode regress needs --parent, a libccmi.so built from the parent commit")
    import ccmi
    n = len(streams)
    rects, ops, _, _ = workload(n)
    dtype = torch.bfloat16
    libs = {"parent": RawStoreCol(a.parent, streams, rects, dtype, ops), "new": RawStoreCol(ccmi.LIB_PATH, streams, rects, dtype, ops)}
    blocks = 3
    reps = blocks * a.reps
    rec = {k: [] for k in libs}
    for it in range(a.warmup + reps):
        for k, s in libs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.render()
            torch.cuda.synchronize()
            if it >= a.warmup:
                rec[k].append(1e3 * (time.perf_counter() - t0))
    same = bool((libs["parent"].out.view(torch.int16) == libs["new"].out.view(torch.int16)).all())
    med = {k: [statistics.median(v[b * a.reps:(b + 1) * a.reps]) for b in range(blocks)] for k, v in rec.items()}
    ref, spread = min(med["parent"]), max(med["parent"]) - min(med["parent"])
    new = statistics.median(med["new"])
    lines = ["regression check: the call without a filter, render_model(size=, colour_ops=) through ccmi_latents_render_col, parent "
             "library against this tree's, one process, alternating",
             f"device: {torch.cuda.get_device_name(0)}; {n} class-E frames, RandomResizedCrop regions -> {OUT[0]}x{OUT[1]}, "
             f"colour_jitter(0.4, 0.4, 0.4, 0.1), RGB, ImageNet mean / std, bfloat16, NCHW; {blocks} blocks of {a.reps} alternating "
             f"repetitions after {a.warmup} warm-up rounds; wall ms per call; workspace parent {libs['parent'].need} bytes, new "
             f"{libs['new'].need} bytes",
             "  parent block medians " + ", ".join(f"{v:.3f}" for v in med["parent"]) + f"  (reference {ref:.3f}, spread {spread:.3f})",
             "  new block medians    " + ", ".join(f"{v:.3f}" for v in med["new"]) +
             f"  (median {new:.3f}; limit {ref + spread:.3f})  {'ok' if new <= ref + spread else 'OUTSIDE the allowance'}",
             f"  all repetitions: parent {rs_ab._fmt_stat(rec['parent'])}  new {rs_ab._fmt_stat(rec['new'])}",
             f"  outputs equal in every element: {same}"]
    for s in libs.values():
        s.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("filter", "regress"), default="filter")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_filter_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_filter_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_filter_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = (mode_filter if a.mode == "filter" else mode_regress)(a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
