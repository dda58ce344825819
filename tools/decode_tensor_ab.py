"""A/B of the bit-exact decoder's two sinks on one GPU, in one process, alternating:
  A  decode.decode_batch(views=True)   host streams -> decoded bytes in pinned host memory
  B  decode.decode_batch_tensors       host streams -> planar u8 tensors on the device
on the bench's `bitexact_decode` set (the 15 committed class-E 1280x720 streams x 64) and,
separately, on the class-B set (5 committed 1920x1080 streams x 64).

Per set: warm-up calls of both (pinned pool, cached device blocks, code objects), then
`--reps` (>= 7) alternating wall-clock repetitions of each; every call ends in a stream
synchronise inside the library, so the wall clock covers header parse, weight decode,
upload, kernels and -- for A -- the downloads.  Reported: the median and the range of the
whole-call rate in Mpixel/s, and of the `ups_syn_out` and `arm_cabac` stage times of
decode.last_timing() (HIP events).  The outputs of the last repetition of each are checked
against the reference decoder's md5s.  Writes the report to --out and prints it."""
import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))

import torch  # noqa: E402

from ccmi import decode  # noqa: E402

MD5 = json.loads((ROOT / "tests/golden/ref_md5.json").read_text())


def _md5_tensor(o) -> str:
    return hashlib.md5(torch.cat([o[k].flatten() for k in "yuv"]).cpu().numpy().tobytes()).hexdigest()


def run_set(cls: str, copies: int, reps: int, warmup: int) -> dict:
    files = sorted((ROOT / "tests/golden/cool").glob(f"{cls}-*.cool"))
    job = [f for _ in range(copies) for f in files]
    streams = [f.read_bytes() for f in job]
    geom, _ = decode.decode_batch_geometry(streams[:1])
    pixels = len(job) * geom[0]["height"] * geom[0]["width"]
    legs = {"A": lambda: decode.decode_batch(streams, views=True), "B": lambda: decode.decode_batch_tensors(streams)}
    rec = {k: {"wall_s": [], "ups_syn_out_ms": [], "arm_cabac_ms": [], "download_ms": []} for k in legs}
    last = {}
    for it in range(warmup + reps):
        for k, fn in legs.items():
            last[k] = None  # B's tensors go back to the caching allocator before the next call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            dt = time.perf_counter() - t0
            tm = decode.last_timing()
            if it >= warmup:
                rec[k]["wall_s"].append(dt)
                for s in ("ups_syn_out", "arm_cabac", "download"):
                    rec[k][s + "_ms"].append(tm[s])
    want = [MD5["jvet/" + f.name]["md5"] for f in job]
    exact = {"A": all(hashlib.md5(o).hexdigest() == w for o, w in zip(last["A"], want)),
             "B": all(_md5_tensor(o) == w for o, w in zip(last["B"][: len(files)] + last["B"][-len(files):],
                                                          want[: len(files)] + want[-len(files):]))}

    def stat(v, f=lambda x: x):
        return {"median": f(statistics.median(v)), "min": f(min(v)), "max": f(max(v))}
    out = {"set": f"class {cls}: {len(files)} streams x {copies} = {len(job)} frames of "
                  f"{geom[0]['width']}x{geom[0]['height']}", "reps": reps, "warmup": warmup}
    for k in legs:
        w = rec[k]["wall_s"]
        out[k] = {"mpixel_s": {"median": pixels / statistics.median(w) / 1e6, "min": pixels / max(w) / 1e6,
                               "max": pixels / min(w) / 1e6},
                  "wall_ms": stat(w, lambda x: 1e3 * x), "ups_syn_out_ms": stat(rec[k]["ups_syn_out_ms"]),
                  "arm_cabac_ms": stat(rec[k]["arm_cabac_ms"]), "download_ms": stat(rec[k]["download_ms"]),
                  "bit_exact_vs_reference_md5": exact[k]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="E,B")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_tensor_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_tensor_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_tensor_ab: at least 7 repetitions")
    lines = ["decode sinks A/B: A = decode_batch(views=True) (host to pinned host), B = decode_batch_tensors "
             "(host to device u8 planes)",
             f"device: {torch.cuda.get_device_name(0)}; one process, A and B alternating; median [min .. max] of "
             f"{a.reps} repetitions after {a.warmup} warm-up rounds", ""]
    for cls in a.sets.split(","):
        r = run_set(cls, a.copies, a.reps, a.warmup)
        lines.append(r["set"])
        for k, name in (("A", "A host-to-host "), ("B", "B to-device    ")):
            x = r[k]

            def f(s, unit):
                return f"{x[s]['median']:9.2f} [{x[s]['min']:9.2f} .. {x[s]['max']:9.2f}] {unit}"
            lines.append(f"  {name} whole call {f('mpixel_s', 'Mpixel/s')}   wall {f('wall_ms', 'ms')}")
            lines.append(f"  {' ' * len(name)} ups_syn_out {f('ups_syn_out_ms', 'ms')}  arm_cabac {f('arm_cabac_ms', 'ms')}"
                         f"  download {f('download_ms', 'ms')}  md5 ok: {x['bit_exact_vs_reference_md5']}")
        ra = r["B"]["mpixel_s"]["median"] / r["A"]["mpixel_s"]["median"]
        rt = r["B"]["ups_syn_out_ms"]["median"] / r["A"]["ups_syn_out_ms"]["median"]
        lines.append(f"  B / A: whole-call rate x{ra:.3f}, ups_syn_out time x{rt:.3f}")
        lines.append("  json: " + json.dumps(r))
        lines.append("")
    text = "\n".join(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
