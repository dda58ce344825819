"""A/B of the tone stage of the decoder's output stage (LatentStore.render_model(tone_ops=...): per-frame
lists of brightness, colour, contrast, sharpness, posterize, solarize, autocontrast and equalize, the
photometric half of RandAugment's op table) against the path it replaces, on one GPU, in one process, legs
alternating, in the form of tools/decode_filter_ab.py and on its frames: the bench's `bitexact_decode` set
(the 15 committed class-E 1280x720 streams x 64 = 960 frames) held in an int16 LatentStore,
RandomResizedCrop windows as the base matrices of decode.rand_augment(n, num_ops=2, magnitude=9) (seeded),
warped to 224 x 224, RGB, ImageNet mean / std, bfloat16.
  N   store.render_model(affine=..., size=(224, 224), tone_ops=..., mean=..., std=..., dtype=bfloat16)
  C   the composed path: the same call without tone ops in float32 (mean 0, std 1), then the same ops as
      torch operations, op position by op position, the frames that share an op gathered, put through
      one batched operation and scattered back; then * scale + bias and the cast to bfloat16.
  P   N without tone ops (the call of the warp row): what the tone stage adds.
Warm-up rounds of all legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a
device synchronise.  Reported per leg: median and range of the time per call and of the tail's device
time (decode.last_timing()), the peak of torch's allocated bytes above what was allocated before the
leg (store and workspaces are the caller's, allocated before) and the tail groups.  N against C: the
share of bf16 elements that differ and by how many bf16 steps (N follows the contract's float32 order
and fixed-point mean, torch its own: counted, not asserted).

--mode regress: the unchanged call, tools/decode_filter_ab.py's regression check (render_model(size=,
colour_ops=) through ccmi_latents_render_col of the parent's library and this tree's, alternating; the new
median of block medians inside the parent's own spread, outputs equal in every element).

Run each mode twice; the report is appended to --out."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decode_filter_ab as flt_ab  # noqa: E402
import decode_resample_ab as rs_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H


def workload(n):
    rects = rs_ab.rrc_rects(n, np.random.default_rng(17))
    base = np.array([[[w / OUT[1], 0.0, x], [0.0, h / OUT[0], y]] for x, y, w, h in rects])
    return decode.rand_augment(n, num_ops=2, magnitude=9, generator=torch.Generator().manual_seed(41), size=OUT, base=base)


def _grey(x):
    return 0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]


def _torch_op(op, sub, v):
    """one op on the frames sub [m, 3, h, w] with their values v [m, 1, 1, 1]"""
    m, _, h, w = sub.shape
    if op == "brightness":
        return (v * sub).clamp_(0, 1)
    if op == "saturation":
        return (v * sub + (1.0 - v) * _grey(sub)).clamp_(0, 1)
    if op == "contrast":
        return (v * sub + (1.0 - v) * _grey(sub).clamp(0, 1).mean((1, 2, 3), keepdim=True)).clamp_(0, 1)
    if op == "solarize":
        return torch.where(sub >= v, 1.0 - sub, sub)
    if op == "posterize":
        L = torch.exp2(v)
        return (sub.clamp(0, 1) * L).floor_().clamp_(min=0).minimum(L - 1.0) / L
    if op == "autocontrast":
        c = sub.clamp(0, 1)
        lo, hi = c.amin((2, 3), keepdim=True), c.amax((2, 3), keepdim=True)
        eq = hi == lo
        scale = torch.where(eq, torch.ones_like(hi), 1.0 / (hi - lo).clamp_(min=1e-30))
        return torch.where(eq, sub, ((sub - lo) * scale).clamp_(0, 1))
    if op == "equalize":
        q = (sub.clamp(0, 1) * 255.0).round_().long().view(3 * m, h * w)
        hist = torch.zeros(3 * m, 256, dtype=torch.int64, device=sub.device).scatter_add_(1, q, torch.ones_like(q))
        last = 255 - (hist.flip(1) > 0).int().argmax(1, keepdim=True)
        step = (h * w - hist.gather(1, last)) // 255
        lut = ((hist.cumsum(1) - hist + step // 2) // step.clamp(min=1)).clamp_(0, 255)
        lut = torch.where(step == 0, torch.arange(256, device=sub.device).expand_as(lut), lut)
        return (lut.gather(1, q).float() / 255.0).view(m, 3, h, w)
    assert op == "sharpness", op
    k = torch.full((3 * m, 1, 3, 3), 1.0 / 13.0, device=sub.device)
    k[:, :, 1, 1] = 5.0 / 13.0
    b = sub.clone()
    b[:, :, 1:-1, 1:-1] = torch.nn.functional.conv2d(sub.reshape(1, 3 * m, h, w), k, groups=3 * m).view(m, 3, h - 2, w - 2)
    return (v * sub + (1.0 - v) * b).clamp_(0, 1)


def torch_tone(x, tones):
    """the tone lists of every frame of x [n, 3, h, w] (float32), as torch operations"""
    for p in range(max(len(t) for t in tones)):
        by_op = {}
        for j, t in enumerate(tones):
            if p < len(t):
                by_op.setdefault(t[p][0], []).append((j, 0.0 if t[p][1] is None else float(t[p][1])))
        for op, frames in by_op.items():
            idx = torch.tensor([j for j, _ in frames], device=x.device)
            v = torch.tensor([f for _, f in frames], device=x.device).view(-1, 1, 1, 1)
            x.index_copy_(0, idx, _torch_op(op, x.index_select(0, idx), v))
    return x


def mode_tone(a, streams):
    n = len(streams)
    mats, tones = workload(n)
    store = decode.LatentStore(streams, dtype=torch.int16)
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    geo = dict(affine=mats, size=OUT, fill=0.0)
    need_p = store.render_model_workspace_bytes(**geo)
    need_n = store.render_model_workspace_bytes(tone_ops=tones, **geo)
    ws = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")
    fmt = dict(mean=MEAN, std=STD, dtype=torch.bfloat16)

    def leg_new():
        out = store.render_model(tone_ops=tones, workspace=ws, **geo, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_plain():
        out = store.render_model(workspace=ws, **geo, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_composed():
        x = store.render_model(dtype=torch.float32, workspace=ws, **geo)
        groups, tail = decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]
        x = torch_tone(x, tones)
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
    names = {"N": "N  render_model(affine=, size=, tone_ops=)                  ",
             "C": "C  render_model(affine=, size=, float32) + torch ops        ",
             "P": "P  render_model(affine=, size=), no tone ops (unchanged)    "}
    staged = sum(len(t) > 0 for t in tones)
    count = {}
    for t in tones:
        for op, _ in t:
            count[op] = count.get(op, 0) + 1
    lines = ["tone stage A/B: LatentStore.render_model(affine=..., size=..., tone_ops=...) against the same call without tone ops in "
             "float32 + the ops as torch operations, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; RandomResizedCrop windows x "
             f"rand_augment(num_ops=2, magnitude=9) -> {OUT[0]}x{OUT[1]}; {staged} frames take the stage ("
             + ", ".join(f"{k} {v}" for k, v in sorted(count.items())) + f"); bf16 RGB normalised; median [min .. max] of "
             f"{a.reps} repetitions after {a.warmup} warm-up rounds; workspace (caller-owned, not in the peaks): "
             f"{need_n / 2**20:.1f} MiB with tone ops, {need_p / 2**20:.1f} MiB without ({need_n - need_p} bytes more)"]
    for k in legs:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    steps = flt_ab.bf16_steps(last["N"], last["C"])
    diff, total = int((steps != 0).sum()), steps.numel()
    hist = ", ".join(f"{k} step{'s' if k > 1 else ''}: {int((steps == k).sum())}" for k in (1, 2, 3))
    lines.append(f"  N against C: {diff} of {total} bf16 elements differ ({100.0 * diff / total:.3f} %); {hist}; more than 3: "
                 f"{int((steps > 3).sum())}; largest {int(steps.max())} steps")
    keep = [j for j, t in enumerate(tones) if not t]
    same = bool((last["N"][keep].view(torch.int16) == last["P"][keep].view(torch.int16)).all())
    lines.append(f"  the {len(keep)} frames that do not take the stage: N equal to P in every element: {same}")
    store.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("tone", "regress"), default="tone")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_tone_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_tone_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_tone_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = (mode_tone if a.mode == "tone" else flt_ab.mode_regress)(a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
