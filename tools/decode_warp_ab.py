"""A/B of the warping output stage (LatentStore.render_model(affine=...): RandomAffine-style rotated
and scaled views, every output pixel a bilinear sample through the frame's own matrix in the
decoder's output stage, one batched tail) against the path it replaces, on one GPU, in one process,
legs alternating, on the bench's `bitexact_decode` set (the 15 committed class-E 1280x720 streams x
64 = 960 frames) held in an int16 LatentStore.  Matrices (seeded): rotation U(-30, 30) degrees,
scale U(0.5, 1.5), centre uniform in the frame; output 224 x 224, RGB, ImageNet mean / std,
bfloat16, pad "fill" with 0.
  N   store.render_model(affine=..., size=(224, 224), mean=..., std=..., dtype=bfloat16)
  C   the composed path: the same windows (LatentStore.warp_plan) rendered as float32 RGB,
      store.render_model(roi=windows, dtype=float32) once per distinct window size, then per group
      torch.nn.functional.grid_sample(bilinear, zeros, align_corners=False) with the grid in the
      window's coordinates, * scale + bias and the cast to bfloat16, written into one
      [n, 3, 224, 224] tensor.
Warm-up rounds of both legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by
a device synchronise.  Reported per leg: median and range of the time per call and of the tail's
device time (decode.last_timing(), summed over the leg's render calls), the peak of torch's
allocated bytes above what was allocated before the leg (store and render workspaces are the
caller's, allocated before), the workspaces, and the batched tail groups / per-frame tails the leg
launched.  The two results are compared: N follows the contract's float32 order, torch's
grid_sample its own, so they differ in rounding (counted, not asserted).

--mode regress: the unchanged call, store.render_model(256 x 256 regions, no size), through the
C ABI of two libraries in one process, alternating, under the rule of profiles/decode_split_ab.txt:
tools/decode_resample_ab.py's check, run from here so that its report lands in this tool's file.

Run each mode twice; the report is appended to --out."""
import argparse
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decode_resample_ab as rs_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = (224, 224)
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H


def random_affines(n, rng):
    return np.stack([decode.affine_matrix(OUT, (rng.uniform(0, W), rng.uniform(0, H)), math.radians(rng.uniform(-30, 30)),
                                          rng.uniform(0.5, 1.5)) for _ in range(n)])


def mode_warp(a, streams):
    n = len(streams)
    rng = np.random.default_rng(23)
    mats = random_affines(n, rng)
    store = decode.LatentStore(streams, dtype=torch.int16)
    wins = [p["window"] for p in store.warp_plan(None, mats, OUT)]
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    by_size = {}
    for j, r in enumerate(wins):
        by_size.setdefault((r[3], r[2]), []).append(j)
    need_n = store.render_model_workspace_bytes(affine=mats, size=OUT)
    need_c = max(store.render_model_workspace_bytes(index=js, roi=[wins[j] for j in js]) for js in by_size.values())
    ws_n = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")
    ws_c = torch.empty(max(need_c, 256), dtype=torch.uint8, device="cuda")
    # the composed leg's grids, in each window's normalised coordinates (built once, outside the timing)
    m = torch.from_numpy(mats).cuda().double()
    cx = (torch.arange(OUT[1], device="cuda", dtype=torch.float64) + 0.5).view(1, 1, -1)
    cy = (torch.arange(OUT[0], device="cuda", dtype=torch.float64) + 0.5).view(1, -1, 1)
    xs = m[:, 0, 0].view(-1, 1, 1) * cx + m[:, 0, 1].view(-1, 1, 1) * cy + m[:, 0, 2].view(-1, 1, 1)
    ys = m[:, 1, 0].view(-1, 1, 1) * cx + m[:, 1, 1].view(-1, 1, 1) * cy + m[:, 1, 2].view(-1, 1, 1)
    wt = torch.tensor(wins, device="cuda", dtype=torch.float64)
    grid = torch.stack([2 * (xs - wt[:, 0].view(-1, 1, 1)) / wt[:, 2].view(-1, 1, 1) - 1,
                        2 * (ys - wt[:, 1].view(-1, 1, 1)) / wt[:, 3].view(-1, 1, 1) - 1], dim=-1).float()
    groups_idx = {k: torch.tensor(js, device="cuda") for k, js in by_size.items()}

    def leg_new():
        out = store.render_model(affine=mats, size=OUT, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws_n)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_composed():
        out = torch.empty(n, 3, *OUT, dtype=torch.bfloat16, device="cuda")
        groups, tail = [0, 0], 0.0
        for k, js in by_size.items():
            x = store.render_model(index=js, roi=[wins[j] for j in js], dtype=torch.float32, workspace=ws_c)
            g = decode.last_tail_groups()
            groups[0] += g[0]
            groups[1] += g[1]
            tail += decode.last_timing()["ups_syn_out"]
            y = torch.nn.functional.grid_sample(x, grid[groups_idx[k]], mode="bilinear", padding_mode="zeros",
                                                align_corners=False)
            out[groups_idx[k]] = (y * scale + bias).to(torch.bfloat16)
        return out, tuple(groups), tail

    legs = {"N": leg_new, "C": leg_composed}
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
    area = [r[2] * r[3] / (W * H) for r in wins]
    names = {"N": "N  render_model(affine=, size=(224, 224))   ", "C": "C  render_model(float32) + grid_sample      "}
    lines = ["warping output stage A/B: LatentStore.render_model(affine=...) against render_model(float32, roi=window) per window "
             "size + torch grid_sample, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; rotation +-30 deg, scale 0.5 .. 1.5, "
             f"random centres (windows {min(area):.3f} .. {max(area):.3f} of the frame, mean {sum(area) / n:.3f}; {len(by_size)} "
             f"distinct sizes) -> {OUT[0]}x{OUT[1]} bf16 RGB normalised, pad fill 0; median [min .. max] of {a.reps} repetitions "
             f"after {a.warmup} warm-up rounds; workspaces (caller-owned, not in the peaks): N {need_n / 2**20:.0f} MiB, "
             f"C {need_c / 2**20:.0f} MiB"]
    for k in legs:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    mm, c = last["N"].float(), last["C"].float()
    diff = int((last["N"].view(torch.int16) != last["C"].view(torch.int16)).sum())
    lines.append(f"  N against C: {diff} of {mm.numel()} bf16 elements differ ({100.0 * diff / mm.numel():.3f} %), largest difference "
                 f"{float((mm - c).abs().max()):.3g} (normalised values; one bf16 step near 2 is 0.0156)")
    store.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("warp", "regress"), default="warp")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--dtype", choices=("bfloat16", "float32", "float16"), default="bfloat16",
                    help="--mode regress: the element type of the rendered tensor")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_warp_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_warp_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_warp_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = (mode_warp if a.mode == "warp" else rs_ab.mode_regress)(a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
