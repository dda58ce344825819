"""A/B of the formatted output (LatentStore.render_model: crop, RGB, normalise, bf16 in the
decoder's output kernel) against the path it replaces, composed from torch operations, on one
GPU, in one process, alternating, on the bench's `bitexact_decode` set (the 15 committed class-E
1280x720 streams x 64 = 960 frames) held in a LatentStore; 256 x 256 regions at seeded random
even origins, RGB, ImageNet mean / std, bfloat16, NCHW:
  M   store.render_model(roi=..., mean=..., std=..., dtype=torch.bfloat16)
  C   store.render(roi=..., dtype=torch.float32, stack=True), then on the device: the chroma
      planes repeated x2, the three planes stacked, the YUV -> RGB matrix, clamp, * scale + bias
      and the cast to bfloat16 -- the contract of ccmi.h, one torch operation per step.

Warm-up rounds of both legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended
by a device synchronise.  Reported per leg: the median and the range of the whole time, of the
decoder tail inside it (decode.last_timing(), HIP events), and the peak of torch's allocated
bytes above what was allocated before the leg (the store and the render workspace, which the
caller owns and every leg shares: what remains is the outputs and the intermediates).  The
last results of the two legs are compared (the torch operations round as the kernel does
wherever torch's kernels divide and do not contract; the count of differing elements is
reported, not asserted).

--mode plain measures store.render(roi=..., dtype=torch.float32, stack=True) alone, for any
libccmi (e.g. one built from the parent commit and named by CCMI_LIB): the existing path next to
its parent.  Run each mode twice; the spread between two runs of one library is the margin.  The
report is appended to --out."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ccmi import decode, encode  # noqa: E402

SIDE = 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
YUV2RGB = ((-0.000007154783816076815, 1.4019975662231445, -179.45477266423404),
           (-0.3441331386566162, -0.7141380310058594, 135.45870971679688),
           (1.7720025777816772, 0.00001542569043522235, -226.8183044444304))


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def composed(store, rois, consts, ws):
    a, b, o, scale, bias = consts
    d = store.render(roi=rois, dtype=torch.float32, stack=True, workspace=ws)
    tail = decode.last_timing()["ups_syn_out"]
    u = d["u"].repeat_interleave(2, 1).repeat_interleave(2, 2)
    v = d["v"].repeat_interleave(2, 1).repeat_interleave(2, 2)
    p = torch.stack((d["y"], u, v), 1)
    q = (((p[:, 0:1] + a * p[:, 1:2]) + b * p[:, 2:3]) + o).clamp_(0.0, 1.0)
    return (q * scale + bias).to(torch.bfloat16), tail


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("model", "plain"), default="model")
    ap.add_argument("--label", default="", help="names the library of a --mode plain run")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_model_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_model_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_model_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    desc = encode.parse(streams[0]).desc
    H, W, n = desc.h, desc.w, len(streams)
    rng = np.random.default_rng(17)
    rois = [(2 * int(rng.integers(0, (W - SIDE) // 2 + 1)), 2 * int(rng.integers(0, (H - SIDE) // 2 + 1)), SIDE, SIDE)
            for _ in range(n)]
    store = decode.LatentStore(streams, dtype=torch.int16)
    del streams
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)  # noqa: E731
    consts = (f32([m[0] for m in YUV2RGB]), f32([m[1] for m in YUV2RGB]),
              f32([float(np.float32(m[2] / 255.0)) for m in YUV2RGB]),
              f32([float(np.float32(1.0 / s)) for s in STD]), f32([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)]))

    # one caller-owned render workspace for every leg (the plans of M, C and P report one size),
    # allocated before the legs: the peak then shows the outputs and the intermediates
    need = store.render_geometry(roi=rois, dtype=torch.float32)[1]
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")

    def leg_model():
        out = store.render_model(roi=rois, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws)
        return out, decode.last_timing()["ups_syn_out"]

    def leg_plain():
        out = store.render(roi=rois, dtype=torch.float32, stack=True, workspace=ws)
        return out, decode.last_timing()["ups_syn_out"]

    legs = {"M": leg_model, "C": lambda: composed(store, rois, consts, ws)} if a.mode == "model" else {"P": leg_plain}
    rec = {k: {"wall_ms": [], "tail_ms": [], "peak_bytes": []} for k in legs}
    last = {}
    for it in range(a.warmup + a.reps):
        for k, fn in legs.items():
            last[k] = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            last[k], tail = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                rec[k]["wall_ms"].append(1e3 * dt)
                rec[k]["tail_ms"].append(tail)
                rec[k]["peak_bytes"].append(torch.cuda.max_memory_allocated() - base)
    names = {"M": "M  render_model (bf16 RGB, normalised)   ", "C": "C  render(float32) + torch operations     ",
             "P": "P  render(float32, stack=True)            "}
    head = ("formatted output A/B: LatentStore.render_model against render(float32) + torch operations, alternating"
            if a.mode == "model" else f"plain render(float32, stack=True), library: {a.label or decode.lib()._name}")
    lines = [head, f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}, {SIDE}x{SIDE} "
                   f"regions at random even origins; median [min .. max] of {a.reps} repetitions after {a.warmup} warm-up rounds; "
                   f"render workspace {need / 2**20:.1f} MiB (caller-owned, not in the peaks)"]
    for k in legs:
        e = {s: _stat(v) for s, v in rec[k].items()}

        def f(s, e=e):
            return f"{e[s]['median']:8.2f} [{e[s]['min']:8.2f} .. {e[s]['max']:8.2f}]"
        lines.append(f"  {names[k]} total {f('wall_ms')} ms  tail {f('tail_ms')} ms  peak allocated "
                     f"{e['peak_bytes']['median'] / 2**20:8.1f} MiB")
    if a.mode == "model":
        m, c = last["M"], last["C"]
        diff = int((m.view(torch.int16) != c.view(torch.int16)).sum())
        worst = float((m.float() - c.float()).abs().max())
        lines.append(f"  M against C: {diff} of {m.numel()} bf16 elements differ, largest difference {worst:.3g}")
    lines.append("")
    text = "\n".join(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)
    store.close()


if __name__ == "__main__":
    main()
