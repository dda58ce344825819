"""A/B of the bicubic output stage (LatentStore.render_model(interpolation="bicubic") with size= and
with affine=) on one GPU, in one process, legs alternating, on the bench's `bitexact_decode` set (the
15 committed class-E 1280x720 streams x 64 = 960 frames) held in an int16 LatentStore; output
224 x 224, RGB, ImageNet mean / std, bfloat16.  In the form of tools/decode_resample_ab.py and
tools/decode_warp_ab.py, whose regions, matrices and composed legs these are.
  a  RandomResizedCrop regions (decode_resample_ab's, with its random mirror):
       Q  render_model(roi=, size=, interpolation="bicubic")
       L  the same call, bilinear
       C  the composed path: render_model(dtype=float32) once per distinct region size, then
          torch.nn.functional.interpolate(mode="bicubic", antialias=True), * scale + bias, the cast
          and the flip
  b  decode_warp_ab's matrices (rotation +-30 degrees, scale 0.5 .. 1.5, random centres), pad fill 0:
       Q  render_model(affine=, size=, interpolation="bicubic")
       L  the same call, bilinear
       C  composed: the bicubic windows (LatentStore.warp_plan) rendered as float32 per window size,
          then torch grid_sample(mode="bicubic", zeros, align_corners=False)
  c  with a and b: the share of bf16 elements of Q that differ from C, and by how many bf16 steps
     (Q follows the contract's float32 order, torch its own: counted, not asserted)
  d  the UNCHANGED bilinear calls, render_model(size=) on a's regions and render_model(affine=) on
     b's matrices, through the C ABI of two libraries in one process, alternating: --parent (a
     libccmi.so built from the parent commit) and the tree's own, under the rule of
     profiles/decode_split_ab.txt: reference = the lowest of the parent's three block medians,
     allowance = their spread; the new library's median of block medians must not exceed reference
     + allowance.  The outputs are compared in every element.
Warm-up rounds of all legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a
device synchronise; medians and ranges.  Run twice; the report is appended to --out."""
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

import decode_resample_ab as rs_ab  # noqa: E402
import decode_warp_ab as warp_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H


def _norm():
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    return scale, bias


def _bf16_steps(a, b):
    """|a - b| in steps of the bf16 grid: the difference of the two bit patterns on the monotone integer line"""
    def line(t):
        v = t.view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return (line(a) - line(b)).abs()


def _time_legs(a, legs):
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
    return rec, last, groups


def _report(names, rec, groups, last):
    lines = []
    for k in names:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    q, c = last["Q"], last["C"]
    steps = _bf16_steps(q, c)
    n = q.numel()
    hist = [int((steps == s).sum()) for s in (1, 2)] + [int((steps > 2).sum())]
    lines.append(f"  c. Q against C: {n - int((steps == 0).sum())} of {n} bf16 elements differ "
                 f"({100.0 * (n - int((steps == 0).sum())) / n:.3f} %): by 1 step {hist[0]}, by 2 {hist[1]}, by more {hist[2]} "
                 f"(largest {int(steps.max())} steps, {float((q.float() - c.float()).abs().max()):.3g} in normalised values; "
                 "one bf16 step near 2 is 0.0156)")
    ql = int((last["Q"].view(torch.int16) != last["L"].view(torch.int16)).sum())
    lines.append(f"     Q against L (bicubic against bilinear): {100.0 * ql / n:.1f} % of the elements differ")
    return lines


def leg_a(a, store, n):
    rng = np.random.default_rng(17)
    rects = rs_ab.rrc_rects(n, rng)
    mirror = [bool(v) for v in rng.integers(0, 2, n)]
    scale, bias = _norm()
    by_size = {}
    for j, r in enumerate(rects):
        by_size.setdefault((r[3], r[2]), []).append(j)
    need_n = store.render_model_workspace_bytes(roi=rects, size=OUT, interpolation="bicubic")
    need_c = max(store.render_model_workspace_bytes(index=js, roi=[rects[j] for j in js]) for js in by_size.values())
    ws_n = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")
    ws_c = torch.empty(max(need_c, 256), dtype=torch.uint8, device="cuda")

    def fused(interpolation):
        def leg():
            out = store.render_model(roi=rects, size=OUT, mean=MEAN, std=STD, dtype=torch.bfloat16, mirror=mirror, workspace=ws_n,
                                     interpolation=interpolation)
            return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]
        return leg

    def composed():
        out = torch.empty(n, 3, *OUT, dtype=torch.bfloat16, device="cuda")
        groups, tail = [0, 0], 0.0
        for js in by_size.values():
            x = store.render_model(index=js, roi=[rects[j] for j in js], dtype=torch.float32, workspace=ws_c)
            g = decode.last_tail_groups()
            groups[0] += g[0]
            groups[1] += g[1]
            tail += decode.last_timing()["ups_syn_out"]
            y = torch.nn.functional.interpolate(x, size=OUT, mode="bicubic", antialias=True, align_corners=False)
            y = (y * scale + bias).to(torch.bfloat16)
            for k, j in enumerate(js):
                out[j] = y[k].flip(-1) if mirror[j] else y[k]
        return out, tuple(groups), tail

    rec, last, groups = _time_legs(a, {"Q": fused("bicubic"), "L": fused("bilinear"), "C": composed})
    area = [r[2] * r[3] / (W * H) for r in rects]
    names = {"Q": "Q  render_model(size=, bicubic)             ", "L": "L  render_model(size=, bilinear)            ",
             "C": "C  render_model(float32) + interpolate(bicubic, antialias)"}
    lines = [f"a. RandomResizedCrop regions (area {min(area):.2f} .. {max(area):.2f} of the frame, mean {sum(area) / n:.2f}; "
             f"{len(by_size)} distinct sizes) -> {OUT[0]}x{OUT[1]} bf16 RGB normalised, random mirror; workspaces (caller-owned, "
             f"not in the peaks): Q = L {need_n / 2**20:.0f} MiB, C {need_c / 2**20:.0f} MiB"]
    return lines + _report(names, rec, groups, last), rects


def leg_b(a, store, n):
    rng = np.random.default_rng(23)
    mats = warp_ab.random_affines(n, rng)
    wins = [p["window"] for p in store.warp_plan(None, mats, OUT, interpolation="bicubic")]
    scale, bias = _norm()
    by_size = {}
    for j, r in enumerate(wins):
        by_size.setdefault((r[3], r[2]), []).append(j)
    need_q = store.render_model_workspace_bytes(affine=mats, size=OUT, interpolation="bicubic")
    need_l = store.render_model_workspace_bytes(affine=mats, size=OUT)
    need_c = max(store.render_model_workspace_bytes(index=js, roi=[wins[j] for j in js]) for js in by_size.values())
    ws_n = torch.empty(max(need_q, need_l, 256), dtype=torch.uint8, device="cuda")
    ws_c = torch.empty(max(need_c, 256), dtype=torch.uint8, device="cuda")
    m = torch.from_numpy(mats).cuda().double()
    cx = (torch.arange(OUT[1], device="cuda", dtype=torch.float64) + 0.5).view(1, 1, -1)
    cy = (torch.arange(OUT[0], device="cuda", dtype=torch.float64) + 0.5).view(1, -1, 1)
    xs = m[:, 0, 0].view(-1, 1, 1) * cx + m[:, 0, 1].view(-1, 1, 1) * cy + m[:, 0, 2].view(-1, 1, 1)
    ys = m[:, 1, 0].view(-1, 1, 1) * cx + m[:, 1, 1].view(-1, 1, 1) * cy + m[:, 1, 2].view(-1, 1, 1)
    wt = torch.tensor(wins, device="cuda", dtype=torch.float64)
    grid = torch.stack([2 * (xs - wt[:, 0].view(-1, 1, 1)) / wt[:, 2].view(-1, 1, 1) - 1,
                        2 * (ys - wt[:, 1].view(-1, 1, 1)) / wt[:, 3].view(-1, 1, 1) - 1], dim=-1).float()
    groups_idx = {k: torch.tensor(js, device="cuda") for k, js in by_size.items()}

    def fused(interpolation):
        def leg():
            out = store.render_model(affine=mats, size=OUT, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws_n,
                                     interpolation=interpolation)
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
            y = torch.nn.functional.grid_sample(x, grid[groups_idx[k]], mode="bicubic", padding_mode="zeros", align_corners=False)
            out[groups_idx[k]] = (y * scale + bias).to(torch.bfloat16)
        return out, tuple(groups), tail

    rec, last, groups = _time_legs(a, {"Q": fused("bicubic"), "L": fused("bilinear"), "C": composed})
    area = [r[2] * r[3] / (W * H) for r in wins]
    names = {"Q": "Q  render_model(affine=, bicubic)           ", "L": "L  render_model(affine=, bilinear)          ",
             "C": "C  render_model(float32) + grid_sample(bicubic)"}
    lines = [f"b. rotation +-30 deg, scale 0.5 .. 1.5, random centres (bicubic windows {min(area):.3f} .. {max(area):.3f} of the "
             f"frame, mean {sum(area) / n:.3f}; {len(by_size)} distinct sizes) -> {OUT[0]}x{OUT[1]} bf16 RGB normalised, pad fill 0; "
             f"workspaces: Q {need_q / 2**20:.0f} MiB, L {need_l / 2**20:.0f} MiB, C {need_c / 2**20:.0f} MiB"]
    # the windows hold in-frame taps only, so a tap outside the WINDOW but inside the frame would show as a large difference in c
    return lines + _report(names, rec, groups, last), mats


class RawSized(rs_ab.RawStore):
    """decode_resample_ab's raw store with the unchanged sized calls: ccmi_latents_render_rs (bilinear) on regions and
    ccmi_latents_render_warp (bilinear, pad fill 0) on matrices, bf16 224 x 224."""

    def __init__(self, path, streams, rects, mats):
        super().__init__(path, streams, [(0, 0, rs_ab.SIDE, rs_ab.SIDE)] * len(streams), torch.bfloat16)
        P, I, Z = C.c_void_p, C.c_int, C.c_size_t
        L, n = self.L, self.n
        L.ccmi_latents_render_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
        L.ccmi_latents_render_rs.argtypes = [P, P, I, P, P, P, P, P, I, I, P, Z, P]
        L.ccmi_latents_render_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
        L.ccmi_latents_render_warp.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
        self.rs_rects = (decode.Rect * n)(*[decode.Rect(*r) for r in rects])
        self.rs = decode.Resample(out_w=OUT[1], out_h=OUT[0], filter=0)
        self.mats = np.ascontiguousarray(mats, dtype=np.float32)
        self.wp = decode.Warp(out_w=OUT[1], out_h=OUT[0], pad=0, matrix=self.mats.ctypes.data)
        geom, need_rs, need_wp = (rs_ab.Geom * n)(), C.c_size_t(0), C.c_size_t(0)
        self.ok(L.ccmi_latents_render_rs_plan(self.h, None, n, self.rs_rects, 0, 0, C.byref(self.fmt), C.byref(self.rs), geom, None,
                                              C.byref(need_rs)))
        self.ok(L.ccmi_latents_render_warp_plan(self.h, None, n, 0, 0, C.byref(self.fmt), C.byref(self.wp), geom, None, None,
                                                C.byref(need_wp)))
        self.ws = torch.empty(max(need_rs.value, need_wp.value, 256), dtype=torch.uint8, device="cuda")
        self.outs = {k: torch.empty(n, 3, *OUT, dtype=torch.bfloat16, device="cuda") for k in ("size", "affine")}
        self.ops = {k: (C.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for k, t in self.outs.items()}
        self.cap = (C.c_size_t * n)(*[3 * OUT[0] * OUT[1] * 2] * n)

    def render(self, which):
        if which == "size":
            self.ok(self.L.ccmi_latents_render_rs(self.h, None, self.n, self.rs_rects, self.ops[which], self.cap, C.byref(self.fmt),
                                                  C.byref(self.rs), 0, 0, self.ws.data_ptr(), self.ws.numel(), self.stream))
        else:
            self.ok(self.L.ccmi_latents_render_warp(self.h, None, self.n, self.ops[which], self.cap, C.byref(self.fmt),
                                                    C.byref(self.wp), 0, 0, self.ws.data_ptr(), self.ws.numel(), self.stream))


def leg_d(a, streams, rects, mats):
    import ccmi
    libs = {"parent": RawSized(a.parent, streams, rects, mats), "new": RawSized(ccmi.LIB_PATH, streams, rects, mats)}
    blocks = 3
    reps = blocks * a.reps
    lines = [f"d. the unchanged bilinear calls, parent library against this tree's, alternating; {blocks} blocks of {a.reps} "
             f"repetitions after {a.warmup} warm-up rounds; wall ms per call"]
    for which in ("size", "affine"):
        rec = {k: [] for k in libs}
        for it in range(a.warmup + reps):
            for k, s in libs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.render(which)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    rec[k].append(1e3 * (time.perf_counter() - t0))
        same = bool((libs["parent"].outs[which].view(torch.int16) == libs["new"].outs[which].view(torch.int16)).all())
        med = {k: [statistics.median(v[b * a.reps:(b + 1) * a.reps]) for b in range(blocks)] for k, v in rec.items()}
        ref, spread = min(med["parent"]), max(med["parent"]) - min(med["parent"])
        new = statistics.median(med["new"])
        lines += [f"  render_model({which}=): parent block medians " + ", ".join(f"{v:.3f}" for v in med["parent"]) +
                  f"  (reference {ref:.3f}, spread {spread:.3f})",
                  "      new block medians " + ", ".join(f"{v:.3f}" for v in med["new"]) +
                  f"  (median {new:.3f}; limit {ref + spread:.3f})  {'ok' if new <= ref + spread else 'OUTSIDE the allowance by %.3f' % (new - ref - spread)}",
                  f"      all repetitions: parent {rs_ab._fmt_stat(rec['parent'])}  new {rs_ab._fmt_stat(rec['new'])};  "
                  f"outputs equal in every element: {same}"]
    for s in libs.values():
        s.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default="", help="leg d: a libccmi.so built from the parent commit (without it the leg is left out)")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_cubic_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_cubic_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_cubic_ab: at least 7 repetitions")
    if a.parent and not Path(a.parent).exists():
        sys.exit("decode_cubic_ab: --parent does not exist")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    n = len(streams)
    lines = ["bicubic output stage A/B: LatentStore.render_model(interpolation=\"bicubic\") against the same call bilinear and against "
             "the composed torch path, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H} in an int16 store; median "
             f"[min .. max] of {a.reps} repetitions after {a.warmup} warm-up rounds"]
    store = decode.LatentStore(streams, dtype=torch.int16)
    la, rects = leg_a(a, store, n)
    lb, mats = leg_b(a, store, n)
    store.close()
    del store
    torch.cuda.empty_cache()
    lines += la + lb
    lines += leg_d(a, streams, rects, mats) if a.parent else ["d. left out (no --parent)"]
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
