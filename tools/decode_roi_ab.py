"""A/B of the bit-exact decoder's whole-frame and region decodes on one GPU, in one process,
alternating, on the bench's `bitexact_decode` set (the 15 committed class-E 1280x720 streams
x 64) and on the class-B set (5 committed 1920x1080 streams x 64):
  W   decode.decode_batch_tensors(streams)                     whole frames
  R   decode.decode_batch_tensors(streams, roi=..., stack=True) 256 x 256 regions at seeded
      random even origins, T the same at the top-left corner, B at the bottom-right corner.

Per set: warm-up calls of every leg, then `--reps` (>= 7) alternating wall-clock repetitions;
every call ends in a stream synchronise inside the library.  Reported: the median and the
range of the whole-call time and of the `arm_cabac` and `ups_syn_out` stage times of
decode.last_timing() (HIP events), the measured region / whole ratios, and beside them what
the plan predicts: for the tail the samples the windows hold at every pyramid level and at
the synthesis output over the frame's, for the ARM the largest arm_rows[0] / h_0 of the
batch (the slowest layer-0 chain sets a batch's arm_cabac, so one region near the bottom edge
is enough to cost what the whole frame costs).  The last repetition's regions are compared
with the crops of the whole-frame result, which is checked against the reference md5s.

--mode whole measures leg W alone (any libccmi, e.g. one built from the parent commit and
named by CCMI_LIB) for the parent-against-new comparison.  The report is appended to --out."""
import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ccmi import decode, encode  # noqa: E402

MD5 = json.loads((ROOT / "tests/golden/ref_md5.json").read_text())
SIDE = 256


def level_windows(desc, rect):
    """[(y0, y1, x0, x1) per pyramid level] a region needs (the recurrence of DESIGN.md, "Region decode")."""
    L = desc.n_grids
    hs, ws = [desc.h], [desc.w]
    for _ in range(1, L):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    n_sp = sum((k - 1) // 2 for k in desc.syn_ks[: desc.n_syn_layers])
    taps = desc.ups_k // 2
    pad = taps // 2
    x, y, w, h = rect
    win = [(max(0, y - n_sp), min(hs[0], y + h + n_sp), max(0, x - n_sp), min(ws[0], x + w + n_sp))]

    def lo(a):
        return max(0, (a >> 1) - pad + (a & 1))

    def hi(b, n):
        return min(n, ((b - 1) >> 1) + ((b - 1) & 1) - pad + taps)
    for k in range(1, L):
        y0, y1, x0, x1 = win[-1]
        win.append((lo(y0), hi(y1, hs[k]), lo(x0), hi(x1, ws[k])))
    return win, hs, ws


def predicted_tail(descs, rects):
    """int32 samples the tail writes for the regions over what it writes for the frames:
    level k's stack has L - k channels (k = 0 .. L - 2), the synthesis output 3."""
    part = full = 0
    for d, r in zip(descs, rects):
        win, hs, ws = level_windows(d, r)
        for k in range(d.n_grids - 1):
            y0, y1, x0, x1 = win[k]
            part += (d.n_grids - k) * (y1 - y0) * (x1 - x0)
            full += (d.n_grids - k) * hs[k] * ws[k]
        part += 3 * r[2] * r[3]
        full += 3 * d.h * d.w
    return part / full


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_set(cls, copies, reps, warmup, mode):
    files = sorted((ROOT / "tests/golden/cool").glob(f"{cls}-*.cool"))
    job = [f for _ in range(copies) for f in files]
    streams = [f.read_bytes() for f in job]
    descs = [encode.parse(f.read_bytes()).desc for f in files] * copies
    H, W = descs[0].h, descs[0].w
    n = len(job)
    legs = {"W": (lambda: decode.decode_batch_tensors(streams), None)}
    if mode == "roi":
        rng = np.random.default_rng(17)
        rois = {"R": [(2 * int(rng.integers(0, (W - SIDE) // 2 + 1)), 2 * int(rng.integers(0, (H - SIDE) // 2 + 1)), SIDE, SIDE)
                      for _ in range(n)],
                "T": [(0, 0, SIDE, SIDE)] * n,
                "B": [(W - SIDE, H - SIDE, SIDE, SIDE)] * n}
        for k, r in rois.items():
            legs[k] = ((lambda r=r: decode.decode_batch_tensors(streams, roi=r, stack=True)), r)
    rec = {k: {"wall_ms": [], "arm_cabac_ms": [], "ups_syn_out_ms": []} for k in legs}
    last = {}
    for it in range(warmup + reps):
        for k, (fn, _) in legs.items():
            last[k] = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            dt = time.perf_counter() - t0
            tm = decode.last_timing()
            if it >= warmup:
                rec[k]["wall_ms"].append(1e3 * dt)
                rec[k]["arm_cabac_ms"].append(tm["arm_cabac"])
                rec[k]["ups_syn_out_ms"].append(tm["ups_syn_out"])
    whole = last["W"]
    nf = len(files)
    exact = {"W": all(hashlib.md5(torch.cat([whole[i][c].flatten() for c in "yuv"]).cpu().numpy().tobytes()).hexdigest()
                      == MD5["jvet/" + job[i].name]["md5"] for i in list(range(nf)) + list(range(n - nf, n)))}
    for k, (_, r) in legs.items():
        if r is None:
            continue
        ok = True
        for i in list(range(nf)) + list(range(n - nf, n)):
            x, y, w, h = r[i]
            ok &= torch.equal(last[k]["y"][i], whole[i]["y"][y: y + h, x: x + w])
            for c in "uv":
                ok &= torch.equal(last[k][c][i], whole[i][c][y // 2: (y + h) // 2, x // 2: (x + w) // 2])
        exact[k] = bool(ok)
    out = {"set": f"class {cls}: {nf} streams x {copies} = {n} frames of {W}x{H}", "pixels": n * H * W, "legs": {}}
    for k, (_, r) in legs.items():
        e = {s: _stat(v) for s, v in rec[k].items()}
        e["exact"] = exact[k]
        if r is not None:
            plan = decode.roi_plan(streams, r)
            e["predicted_tail_ratio"] = predicted_tail(descs, r)
            e["predicted_arm_ratio"] = max(p["arm_rows"][0] for p in plan) / H
            for s in rec[k]:
                e[s + "_ratio"] = e[s]["median"] / statistics.median(rec["W"][s])
            e["workspace_bytes"] = decode.decode_batch_geometry(streams, roi=r)[1]
        else:
            e["workspace_bytes"] = decode.decode_batch_geometry(streams)[1]
            e["mpixel_s"] = n * H * W / (1e3 * e["wall_ms"]["median"])
        out["legs"][k] = e
    return out


NAMES = {"W": "W whole frames ", "R": "R random 256^2 ", "T": "T top-left     ", "B": "B bottom-right "}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("roi", "whole"), default="roi")
    ap.add_argument("--label", default="", help="names the library of a --mode whole run")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="E,B")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_roi_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_roi_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_roi_ab: at least 7 repetitions")
    head = ("region decode A/B: whole-frame decode_batch_tensors and 256x256 region decodes, alternating" if a.mode == "roi"
            else f"whole-frame decode_batch_tensors, library: {a.label or decode.lib()._name}")
    lines = [head, f"device: {torch.cuda.get_device_name(0)}; one process; median [min .. max] of {a.reps} repetitions "
                   f"after {a.warmup} warm-up rounds", ""]
    for cls in a.sets.split(","):
        r = run_set(cls, a.copies, a.reps, a.warmup, a.mode)
        lines.append(r["set"])
        for k, e in r["legs"].items():
            def f(s):
                return f"{e[s]['median']:8.2f} [{e[s]['min']:8.2f} .. {e[s]['max']:8.2f}] ms"
            rate = f"  {e['mpixel_s']:8.1f} Mpixel/s" if "mpixel_s" in e else ""
            lines.append(f"  {NAMES[k]} wall {f('wall_ms')}  arm_cabac {f('arm_cabac_ms')}  ups_syn_out {f('ups_syn_out_ms')}"
                         f"{rate}  workspace {e['workspace_bytes'] / 2**20:8.1f} MiB  exact: {e['exact']}")
            if "predicted_tail_ratio" in e:
                lines.append(f"  {' ' * len(NAMES[k])} / W: wall x{e['wall_ms_ratio']:.3f}; ups_syn_out x{e['ups_syn_out_ms_ratio']:.3f} "
                             f"(plan: window samples / frame samples = {e['predicted_tail_ratio']:.3f}); arm_cabac "
                             f"x{e['arm_cabac_ms_ratio']:.3f} (plan: largest arm_rows[0] / h_0 = {e['predicted_arm_ratio']:.3f})")
        lines.append("  json: " + json.dumps(r))
        lines.append("")
    text = "\n".join(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
