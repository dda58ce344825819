"""A/B of the latent store (decode.LatentStore: decode once, render often) against the decodes
it replaces, on one GPU, in one process, alternating, on the bench's `bitexact_decode` set (the
15 committed class-E 1280x720 streams x 64) and on the class-B set (5 committed 1920x1080
streams x 64):
  W    decode.decode_batch_tensors(streams)                      whole frames
  D    decode.LatentStore(streams, dtype=torch.int16)            the build (ARM + CABAC, pack)
  SW   store.render()                                            whole frames from the store
  R    decode.decode_batch_tensors(streams, roi=..., stack=True) 256 x 256 regions at seeded random
       even origins, T the same at the top-left corner, B at the bottom-right corner
  SR / ST / SB  store.render(roi=..., stack=True)                the same regions from the store

Per set: warm-up rounds of every leg, then `--reps` (>= 7) alternating wall-clock repetitions;
every call ends in a stream synchronise inside the library.  Reported per leg: the median and
the range of the whole-call time and of the stage times of decode.last_timing() (HIP events; a
render's are upload = table upload, arm_cabac = the unpack, ups_syn_out = the tail; the
build's ups_syn_out is the pack), the host's share of a render (wall - device stages) and the
time of the header-only planning call for the same arguments, the store's bytes per stream
at each element type against the 4-byte planes, and the workspaces.  Every store leg's last
result is compared with the decode leg's (whole frames also against the reference md5s).

--mode whole measures leg W alone (any libccmi, e.g. one built from the parent commit and
named by CCMI_LIB) for the parent-against-new comparison.  The report is appended to --out."""
import argparse
import ctypes as C
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
STAGES = ("upload", "arm_cabac", "ups_syn_out")


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def store_sizes(streams):
    """Header-only: bytes of the store at each element type, and the build workspace."""
    L = decode._bind()
    keep, sp, ln = decode._marshal(streams)
    out = {}
    for name, t in (("int8", 0), ("int16", 1), ("int32", 2)):
        tot, ws = C.c_size_t(0), C.c_size_t(0)
        decode.check(L.ccmi_latents_plan(sp, ln, len(streams), t, C.byref(tot), None, C.byref(ws)))
        out[name] = tot.value
        out["build_workspace"] = ws.value
    return out


def same(a, b):
    if isinstance(a, dict):
        return all(torch.equal(a[k], b[k]) for k in "yuv")
    if isinstance(a, list):
        return all(same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


def run_set(cls, copies, reps, warmup, mode):
    files = sorted((ROOT / "tests/golden/cool").glob(f"{cls}-*.cool"))
    job = [f for _ in range(copies) for f in files]
    streams = [f.read_bytes() for f in job]
    desc = encode.parse(streams[0]).desc
    H, W = desc.h, desc.w
    n, nf = len(job), len(files)
    legs = {"W": lambda: decode.decode_batch_tensors(streams)}
    rois, box = {}, {}
    if mode == "store":
        rng = np.random.default_rng(17)
        rois = {"R": [(2 * int(rng.integers(0, (W - SIDE) // 2 + 1)), 2 * int(rng.integers(0, (H - SIDE) // 2 + 1)), SIDE, SIDE)
                      for _ in range(n)],
                "T": [(0, 0, SIDE, SIDE)] * n,
                "B": [(W - SIDE, H - SIDE, SIDE, SIDE)] * n}

        def build():
            box["store"] = None  # one store at a time
            box["store"] = decode.LatentStore(streams, dtype=torch.int16)
        legs["D"] = build
        legs["SW"] = lambda: box["store"].render()
        for k, r in rois.items():
            legs[k] = lambda r=r: decode.decode_batch_tensors(streams, roi=r, stack=True)
            legs["S" + k] = lambda r=r: box["store"].render(roi=r, stack=True)
    rec = {k: {s: [] for s in ("wall_ms",) + STAGES} for k in legs}
    last = {}
    for it in range(warmup + reps):
        for k, fn in legs.items():
            last[k] = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            dt = time.perf_counter() - t0
            tm = decode.last_timing()
            if it >= warmup:
                rec[k]["wall_ms"].append(1e3 * dt)
                for s in STAGES:
                    rec[k][s].append(tm[s])
    whole = last["W"]
    probe = list(range(nf)) + list(range(n - nf, n))
    exact = {"W": all(hashlib.md5(torch.cat([whole[i][c].flatten() for c in "yuv"]).cpu().numpy().tobytes()).hexdigest()
                      == MD5["jvet/" + job[i].name]["md5"] for i in probe)}
    if mode == "store":
        exact["SW"] = same(last["SW"], whole)
        for k in rois:
            exact["S" + k] = same(last["S" + k], last[k])
    out = {"set": f"class {cls}: {nf} streams x {copies} = {n} frames of {W}x{H}", "frames": n, "legs": {}}
    for k in legs:
        e = {s: _stat(v) for s, v in rec[k].items()}
        if k in exact:
            e["exact"] = exact[k]
        if k.startswith("S"):
            st, r = box["store"], rois.get(k[1:])
            e["host_ms"] = _stat([w - sum(x) for w, *x in zip(rec[k]["wall_ms"], *(rec[k][s] for s in STAGES))])
            plan = []
            for _ in range(5):
                t0 = time.perf_counter()
                need = st.render_geometry(roi=r)[1]
                plan.append(1e3 * (time.perf_counter() - t0))
            e["plan_ms"] = _stat(plan)
            e["workspace_bytes"] = need
        elif k != "D":
            e["workspace_bytes"] = decode.decode_batch_geometry(streams, roi=rois.get(k))[1]
        out["legs"][k] = e
    if mode == "store":
        sizes = store_sizes(streams)
        lat = sum(h * w for h, w in encode.parse(streams[0]).grid_sizes)
        out["store"] = {"latents_per_stream": lat, "int32_planes_bytes_per_stream": 4 * lat,
                        **{t: sizes[t] / n for t in ("int8", "int16", "int32")}, "build_workspace": sizes["build_workspace"],
                        "built_nbytes": box["store"].nbytes}
        box["store"].close()
    else:
        out["legs"]["W"]["mpixel_s"] = n * H * W / (1e3 * out["legs"]["W"]["wall_ms"]["median"])
    return out


NAMES = {"W": "W  whole frames, decode     ", "D": "D  store build (int16)      ", "SW": "SW whole frames, render     ",
         "R": "R  random 256^2, decode     ", "SR": "SR random 256^2, render     ", "T": "T  top-left, decode         ",
         "ST": "ST top-left, render         ", "B": "B  bottom-right, decode     ", "SB": "SB bottom-right, render     "}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("store", "whole"), default="store")
    ap.add_argument("--label", default="", help="names the library of a --mode whole run")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="E,B")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_latents_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_latents_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_latents_ab: at least 7 repetitions")
    head = ("latent store A/B: decode_batch_tensors against LatentStore build / render, alternating" if a.mode == "store"
            else f"whole-frame decode_batch_tensors, library: {a.label or decode.lib()._name}")
    lines = [head, f"device: {torch.cuda.get_device_name(0)}; one process; median [min .. max] of {a.reps} repetitions "
                   f"after {a.warmup} warm-up rounds", ""]
    for cls in a.sets.split(","):
        r = run_set(cls, a.copies, a.reps, a.warmup, a.mode)
        lines.append(r["set"])
        for k, e in r["legs"].items():
            def f(s):
                return f"{e[s]['median']:8.2f} [{e[s]['min']:8.2f} .. {e[s]['max']:8.2f}]"
            names = (("table upload", "unpack", "tail") if k.startswith("S") else
                     ("upload", "arm_cabac", "pack") if k == "D" else ("upload", "arm_cabac", "ups_syn_out"))
            line = f"  {NAMES[k]} wall {f('wall_ms')} ms  " + "  ".join(f"{nm} {f(s)}" for nm, s in zip(names, STAGES))
            if "host_ms" in e:
                line += f"  host (wall - stages) {f('host_ms')}  plan call {f('plan_ms')}"
            if "workspace_bytes" in e:
                line += f"  workspace {e['workspace_bytes'] / 2**20:8.1f} MiB"
            if "mpixel_s" in e:
                line += f"  {e['mpixel_s']:8.1f} Mpixel/s"
            if "exact" in e:
                line += f"  exact: {e['exact']}"
            lines.append(line)
        if "store" in r:
            s = r["store"]
            lines.append(f"  store bytes per stream ({s['latents_per_stream']} latents; int32 planes {s['int32_planes_bytes_per_stream']}): "
                         f"int8 {s['int8']:.0f}, int16 {s['int16']:.0f}, int32 {s['int32']:.0f}; built (int16) "
                         f"{s['built_nbytes'] / 2**20:.1f} MiB in all; build workspace {s['build_workspace'] / 2**20:.1f} MiB")
        lines.append("  json: " + json.dumps(r))
        lines.append("")
    text = "\n".join(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
