"""A/B of the perspective warp of the output stage (LatentStore.render_model(perspective=...): every
output pixel a bilinear sample at the position the frame's 3 x 3 homography gives, one batched tail) in
the form of tools/decode_warp_ab.py: one GPU, one process, legs alternating, on the bench's
`bitexact_decode` set (the 15 committed class-E 1280x720 streams x 64 = 960 frames) held in an int16
LatentStore.  Bases (seeded): RandomResizedCrop regions as 2 x 3 matrices of the 224 x 224 output;
homographies: decode.random_perspective(distortion_scale=0.5, p=1, base=bases).  Output 224 x 224, RGB,
ImageNet mean / std, bfloat16, pad "fill" with 0.
  P   store.render_model(perspective=..., size=(224, 224), mean=..., std=..., dtype=bfloat16)
  A   the same call with affine=bases: the price of the projective position (and of its larger windows)
  C   the composed path: the windows of P (LatentStore.warp_plan(perspective=...)) rendered as float32
      RGB, store.render_model(roi=windows, dtype=float32) once per distinct window size, then per group
      torch.nn.functional.grid_sample(bilinear, zeros, align_corners=False) on the projective grid in the
      window's coordinates, * scale + bias and the cast to bfloat16, into one [n, 3, 224, 224] tensor.
Warm-up rounds of all legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a
device synchronise.  Reported per leg: median and range of the time per call and of the tail's device
time, the peak of torch's allocated bytes above what was allocated before the leg, the workspaces and the
tail groups.  P is compared with C: P follows the contract's float32 order, torch its own, so they
differ in rounding (the share of bf16 elements and by how many steps are counted, not asserted).

d. with --parent (a libccmi.so built from the parent commit): the unchanged calls, render_model(size=)
on the RandomResizedCrop regions and render_model(affine=) on rotations, through the C ABI of both
libraries in one process, alternating in three blocks (tools/decode_cubic_ab.py's leg d): equal in every
element, and the new block medians against the parent's own spread.

Run it twice; the report is appended to --out."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decode_cubic_ab as cubic_ab  # noqa: E402
import decode_resample_ab as rs_ab  # noqa: E402
import decode_warp_ab as warp_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H


def leg_persp(a, store, n):
    rng = np.random.default_rng(17)
    rects = rs_ab.rrc_rects(n, rng)
    bases = np.array([[[w / OUT[1], 0, x], [0, h / OUT[0], y]] for x, y, w, h in rects], dtype=np.float32)
    mats = decode.random_perspective(n, OUT, distortion_scale=0.5, p=1.0, base=bases, generator=29)
    wins = [p["window"] for p in store.warp_plan(None, None, OUT, perspective=mats)]
    awins = [p["window"] for p in store.warp_plan(None, bases, OUT)]
    scale, bias = cubic_ab._norm()
    by_size = {}
    for j, r in enumerate(wins):
        by_size.setdefault((r[3], r[2]), []).append(j)
    need_p = store.render_model_workspace_bytes(perspective=mats, size=OUT)
    need_a = store.render_model_workspace_bytes(affine=bases, size=OUT)
    need_c = max(store.render_model_workspace_bytes(index=js, roi=[wins[j] for j in js]) for js in by_size.values())
    ws_n = torch.empty(max(need_p, need_a, 256), dtype=torch.uint8, device="cuda")
    ws_c = torch.empty(max(need_c, 256), dtype=torch.uint8, device="cuda")
    # the composed leg's grids, in each window's normalised coordinates (built once, outside the timing)
    m = torch.from_numpy(mats).cuda().double()
    cx = (torch.arange(OUT[1], device="cuda", dtype=torch.float64) + 0.5).view(1, 1, -1)
    cy = (torch.arange(OUT[0], device="cuda", dtype=torch.float64) + 0.5).view(1, -1, 1)
    row = [m[:, r, 0].view(-1, 1, 1) * cx + m[:, r, 1].view(-1, 1, 1) * cy + m[:, r, 2].view(-1, 1, 1) for r in range(3)]
    xs, ys = row[0] / row[2], row[1] / row[2]
    wt = torch.tensor(wins, device="cuda", dtype=torch.float64)
    grid = torch.stack([2 * (xs - wt[:, 0].view(-1, 1, 1)) / wt[:, 2].view(-1, 1, 1) - 1,
                        2 * (ys - wt[:, 1].view(-1, 1, 1)) / wt[:, 3].view(-1, 1, 1) - 1], dim=-1).float()
    groups_idx = {k: torch.tensor(js, device="cuda") for k, js in by_size.items()}

    def fused(**geo):
        def leg():
            out = store.render_model(size=OUT, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws_n, **geo)
            return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]
        return leg

    def composed():
        out = torch.empty(n, 3, *OUT, dtype=torch.bfloat16, device="cuda")
        groups, tail = [0, 0], 0.0
        for k, js in by_size.items():
            x = store.render_model(index=js, roi=[wins[j] for j in js], dtype=torch.float32, workspace=ws_c)
            g = decode.last_tail_groups()
            groups[0] += g[0]
            groups[1] += g[1]
            tail += decode.last_timing()["ups_syn_out"]
            y = torch.nn.functional.grid_sample(x, grid[groups_idx[k]], mode="bilinear", padding_mode="zeros", align_corners=False)
            out[groups_idx[k]] = (y * scale + bias).to(torch.bfloat16)
        return out, tuple(groups), tail

    names = {"P": "P  render_model(perspective=, size=(224, 224))", "A": "A  render_model(affine=bases, size=(224, 224))",
             "C": "C  render_model(float32) + grid_sample         "}
    rec, last, groups = cubic_ab._time_legs(a, {"P": fused(perspective=mats), "A": fused(affine=bases), "C": composed})
    area, aarea = [r[2] * r[3] / (W * H) for r in wins], [r[2] * r[3] / (W * H) for r in awins]
    wn = (m[:, 2, 0].abs() * OUT[1] + m[:, 2, 1].abs() * OUT[0])
    lines = [f"a. RandomResizedCrop bases x random_perspective(0.5, p=1) (windows {min(area):.3f} .. {max(area):.3f} of the frame, mean "
             f"{sum(area) / n:.3f}, {len(by_size)} distinct sizes; the bases' own windows mean {sum(aarea) / n:.3f}; |m20| out_w + |m21| out_h "
             f"up to {float(wn.max()):.2f}) -> {OUT[0]}x{OUT[1]} bf16 RGB normalised, pad fill 0; workspaces (caller-owned, not in the "
             f"peaks): P {need_p / 2**20:.0f} MiB, A {need_a / 2**20:.0f} MiB, C {need_c / 2**20:.0f} MiB"]
    for k in names:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    p, c = last["P"], last["C"]
    steps = cubic_ab._bf16_steps(p, c)
    tot = p.numel()
    differ = tot - int((steps == 0).sum())
    lines.append(f"  P against C: {differ} of {tot} bf16 elements differ ({100.0 * differ / tot:.3f} %): by 1 step {int((steps == 1).sum())}, "
                 f"by 2 {int((steps == 2).sum())}, by more {int((steps > 2).sum())} (largest {int(steps.max())} steps, "
                 f"{float((p.float() - c.float()).abs().max()):.3g} in normalised values; one bf16 step near 2 is 0.0156)")
    return lines, rects


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default="", help="leg d: a libccmi.so built from the parent commit (without it the leg is left out)")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_persp_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_persp_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_persp_ab: at least 7 repetitions")
    if a.parent and not Path(a.parent).exists():
        sys.exit("decode_persp_ab: --parent does not exist")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    n = len(streams)
    lines = ["perspective warp A/B: LatentStore.render_model(perspective=...) against the same call with affine= on the same bases and "
             "against the composed torch path, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H} in an int16 store; median "
             f"[min .. max] of {a.reps} repetitions after {a.warmup} warm-up rounds"]
    store = decode.LatentStore(streams, dtype=torch.int16)
    la, rects = leg_persp(a, store, n)
    store.close()
    del store
    torch.cuda.empty_cache()
    lines += la
    if a.parent:
        lines += cubic_ab.leg_d(a, streams, rects, warp_ab.random_affines(n, np.random.default_rng(23)))
    else:
        lines.append("d. left out (no --parent)")
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
