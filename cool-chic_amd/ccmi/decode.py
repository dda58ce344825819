"""Path B (bit-exact .cool decoder) launchers over the C ABI."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

from . import ERR_IO, MAX_GRIDS, MAX_SYN_LAYERS, CcmiError, SynLayer, check, lib


class UpsI32Args(C.Structure):
    _fields_ = [("latent", C.c_void_p), ("n_grids", C.c_int), ("h", C.c_int * MAX_GRIDS), ("w", C.c_int * MAX_GRIDS),
                ("kernels", C.c_void_p), ("ups_k", C.c_int), ("n_ups", C.c_int), ("pre_k", C.c_int), ("n_pre", C.c_int),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class SynI32Args(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("c_in", C.c_int), ("h", C.c_int), ("w", C.c_int), ("n_layers", C.c_int),
                ("layers", SynLayer * MAX_SYN_LAYERS), ("params", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


_P, _I, _Z = C.c_void_p, C.c_int, C.c_size_t
# every decoder prototype this module calls: name -> argument types (the result is an int but for _RESTYPES)
_PROTOS = {
    "ccmi_decode_weights_i32": [_P, _Z, _P, _Z, _P, _Z, _P, _Z, _P],
    "ccmi_ups_workspace_bytes_i32": [_I, _P, _P],
    "ccmi_ups_forward_i32": [C.POINTER(UpsI32Args), _P],
    "ccmi_syn_workspace_bytes_i32": [C.POINTER(SynI32Args)],
    "ccmi_syn_forward_i32": [C.POINTER(SynI32Args), _P],
    "ccmi_decode_latents": [_P, _Z, _P, _Z, _P],
    "ccmi_decode_batch_workspace_bytes": [_P, _P, _I, _I, _I, _I, _P],
    "ccmi_decode_batch_ws": [_P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_plan": [_P, _P, _I, _I, _I, _I, _P, _P],
    "ccmi_decode_batch_dev_plan": [_P, _P, _I, _I, _I, _I, _P, _P],
    "ccmi_decode_batch_dev": [_P, _P, _I, _P, _P, _I, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_roi_plan": [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P],
    "ccmi_decode_batch_dev_roi": [_P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_fmt_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_fmt": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_rs_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_rs": [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_last_tail_groups": [_P, _P],
    "ccmi_decode_batch_dev_warp_plan": [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_warp": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_warp_plan": [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "ccmi_latents_render_warp": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_col_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_col": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_col_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_latents_render_col": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_flt_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_flt": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_flt_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_latents_render_flt": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_tone_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_tone": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_tone_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_latents_render_tone": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_mix_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_mix": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_mix_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_latents_render_mix": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_decode_batch_dev_blend_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_decode_batch_dev_blend": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_blend_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "ccmi_latents_render_blend": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_plan": [_P, _P, _I, _I, _P, _P, _P],
    "ccmi_latents_decode": [_P, _P, _I, _I, _P, _Z, _P, _Z, _P, _P],
    "ccmi_latents_free": [_P],
    "ccmi_latents_count": [_P],
    "ccmi_latents_values": [_P, _I, _P, _Z, _P],
    "ccmi_latents_render_plan": [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P],
    "ccmi_latents_render": [_P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_fmt_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P],
    "ccmi_latents_render_fmt": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_render_rs_plan": [_P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P],
    "ccmi_latents_render_rs": [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P],
    "ccmi_latents_compact_plan": [_P, _P, _P],
    "ccmi_latents_compact_measure": [_P, _P, _Z, _P, _P, _P],
    "ccmi_latents_compact": [_P, _P, _Z, _P, _Z, _P, _P],
    "ccmi_latents_concat": [_P, _I, _P],
    "ccmi_latents_stream_info": [_P, _I, _P, _P],
    "ccmi_latents_file_head": [_P, _Z, _P, _P, _P],
    "ccmi_latents_export_plan": [_P, _P, _I, _P, _P, _P],
    "ccmi_latents_export": [_P, _P, _I, _P, _P, _Z, _P, _Z, _P],
    "ccmi_latents_import_plan": [_P, _Z, _I, _I, _P, _P, _P, _P],
    "ccmi_latents_import": [_P, _Z, _I, _I, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P],
}
_RESTYPES = {"ccmi_ups_workspace_bytes_i32": _Z, "ccmi_syn_workspace_bytes_i32": _Z, "ccmi_latents_free": None}


def _bind():
    """The library with every prototype of _PROTOS declared that it has: older builds, loaded
    for A/B runs, lack the newer entry points."""
    L = lib()
    if not getattr(L, "_ccmi_dec_bound", False):
        for name, argtypes in _PROTOS.items():
            if hasattr(L, name):
                f = getattr(L, name)
                f.argtypes, f.restype = argtypes, _RESTYPES.get(name, C.c_int)
        L._ccmi_dec_bound = True
    return L


# the names the tests reach the bound library by, from when each sink had a binder of its own
_bind_dev = _bind_latents = _bind_fmt = _bind_rs = _bind


def decode_file(inp: str, out: str = "", output_bitdepth: int = 0, output_chroma_format: int = 0,
                verbosity: int = 0, device: int = 0) -> int:
    """Same contract as the reference's cc_decode_cpu (ccdecapi_cpu.cpp:20-30): returns 0 / 1."""
    return lib().ccmi_decode_file(inp.encode(), out.encode(), output_bitdepth, output_chroma_format, verbosity,
                                  device)


def output_size(stream: bytes, output_bitdepth: int = 0, output_chroma_format: int = 0, as_yuv: bool = True) -> int:
    n = C.c_size_t(0)
    buf = C.create_string_buffer(stream, len(stream))
    check(lib().ccmi_decode_output_size(C.cast(buf, C.c_void_p), len(stream), output_bitdepth,
                                        output_chroma_format, int(as_yuv), C.byref(n)))
    return n.value


class _PinnedPool:
    """Grow-only pinned host buffer per thread for decode_batch's outputs: the decoder's
    per-chunk downloads are then DMA copies that overlap the rest of the batch, and the
    buffer is reused across calls (hipHostMalloc of a GB-sized buffer costs more than the
    decode).  Like the reference decoder's frame_memory (cc-frame-decoder.cpp:1151), what
    decode_batch(views=True) returns stays valid until the next call on this thread."""

    def __init__(self):
        import threading
        self.tls = threading.local()

    def get(self, nbytes: int):
        import torch
        t = getattr(self.tls, "buf", None)
        if t is None or t.numel() < nbytes:
            self.tls.buf = None
            t = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self.tls.buf = t
        return t


_POOL = _PinnedPool()


def _marshal(streams, who="decode_batch_tensors"):
    """(what keeps them alive, pointer array, length array) of the streams; who names the caller
    that refuses an empty list itself (None: the library does)."""
    n = len(streams)
    if n < 1 and who:
        raise ValueError(f"{who}: no streams")
    bufs = [C.create_string_buffer(s, len(s)) for s in streams]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
    ln = (C.c_size_t * n)(*[len(s) for s in streams])
    return bufs, sp, ln


def _stream_ws(dev, stream_handle, workspace, need):
    """The caller's stream and workspace, or the defaults: torch's current stream of dev and
    `need` bytes from its caching allocator."""
    import torch
    if stream_handle is None:
        stream_handle = torch.cuda.current_stream(dev).cuda_stream
    if workspace is None:
        workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    return stream_handle, workspace


def decode_batch(streams: Sequence[bytes], output_bitdepth: int = 0, output_chroma_format: int = 0,
                 as_yuv: bool = True, stream_handle: int | None = None, workspace=None, views: bool = False) -> list:
    """Decode independent intra .cool streams in one batched launch sequence; returns the
    bytes the reference decoder would write for each (YUV planes, or PPM).

    One header-only pass sizes the outputs and the device workspace
    (ccmi_decode_batch_plan); the outputs land in a pinned host pool and the device
    workspace comes from torch's caching allocator unless `workspace` (a uint8 CUDA tensor of
    at least decode_batch_workspace_bytes(...) bytes) is given: ccmi_decode_batch_ws, no
    allocation inside the library.  views=True returns memoryviews into the pool (no copy;
    valid until the next call on this thread), otherwise bytes."""
    import torch
    n = len(streams)
    keep, sp, ln = _marshal(streams, "decode_batch")
    cap = (C.c_size_t * n)()
    need = C.c_size_t(0)
    L = _bind()
    check(L.ccmi_decode_batch_plan(sp, ln, n, output_bitdepth, output_chroma_format, int(as_yuv), cap, C.byref(need)))
    offs, tot = [], 0
    for k in cap:
        offs.append(tot)
        tot += (int(k) + 255) // 256 * 256
    pool = _POOL.get(tot)
    base = pool.data_ptr()
    op = (C.c_void_p * n)(*[base + o for o in offs])
    got = (C.c_size_t * n)()
    stream_handle, workspace = _stream_ws(torch.device("cuda", torch.cuda.current_device()), stream_handle, workspace,
                                          need.value)
    check(L.ccmi_decode_batch_ws(sp, ln, n, op, cap, got, output_bitdepth, output_chroma_format, int(as_yuv),
                                 workspace.data_ptr(), workspace.numel(), stream_handle))
    mv = memoryview(pool.numpy())
    if views:
        return [mv[o: o + got[i]] for i, o in enumerate(offs)]
    return [bytes(mv[o: o + got[i]]) for i, o in enumerate(offs)]


def decode_batch_workspace_bytes(streams: Sequence[bytes], output_bitdepth: int = 0, output_chroma_format: int = 0,
                                 as_yuv: bool = True) -> int:
    keep, sp, ln = _marshal(streams, None)
    out = C.c_size_t(0)
    check(_bind().ccmi_decode_batch_workspace_bytes(sp, ln, len(streams), output_bitdepth, output_chroma_format,
                                                    int(as_yuv), C.byref(out)))
    return out.value


class FrameGeom(C.Structure):
    """ccmi_frame_geom: geometry of one stream's decoded tensor."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bitdepth", C.c_int), ("chroma", C.c_int),
                ("frame_data_type", C.c_int), ("elems", C.c_size_t)]


class Rect(C.Structure):
    """ccmi_rect: a region of a frame in luma samples, x / y = its top-left corner."""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class RoiInfo(C.Structure):
    """ccmi_roi_info: what a region decode of one stream does."""
    _fields_ = [("n_grids", C.c_int), ("arm_rows", C.c_int * MAX_GRIDS), ("windowed", C.c_int)]


SAMPLE_U8, SAMPLE_U16, SAMPLE_F32 = 0, 1, 2  # CCMI_SAMPLE_*


def _roi_rects(roi, n, whole, noun):
    """roi argument -> ccmi_rect array of n entries, or None for whole frames.  One (x, y, w, h)
    for every stream / frame (the noun), or a sequence with one entry per; an entry None is
    whole(i), that entry's whole frame."""
    if roi is None:
        return None
    one = len(roi) == 4 and all(isinstance(v, int) for v in roi)
    rois = [tuple(roi)] * n if one else list(roi)
    if len(rois) != n:
        raise ValueError(f"roi: one (x, y, w, h), or one entry per {noun} ({n}), got {len(rois)}")
    arr = (Rect * n)()
    for i, r in enumerate(rois):
        if r is None:
            r = whole(i)
        if len(r) != 4:
            raise ValueError(f"roi[{i}]: (x, y, w, h) expected")
        arr[i] = Rect(*[int(v) for v in r])
    return arr


def _rects(roi, streams, n):
    """_roi_rects of streams: a whole frame's size is read from the stream's GOP header."""
    def whole(i):
        s = streams[i]
        if len(s) < 6:
            raise ValueError(f"stream {i}: truncated GOP header")
        return 0, 0, int.from_bytes(s[4:6], "big"), int.from_bytes(s[2:4], "big")
    return _roi_rects(roi, n, whole, "stream")


def _pick_sample(plan, geom, dtype, who):
    """Runs plan(sample type), which fills geom, with the sample type of dtype, and returns the
    type.  dtype None: planned at U16 first (any bitdepth: learns every output bitdepth), then U8
    when every output fits it."""
    import torch
    if dtype is None:
        plan(SAMPLE_U16)
        sample = SAMPLE_U8 if all(g.bitdepth <= 8 for g in geom) else SAMPLE_U16
    else:
        table = {torch.uint8: SAMPLE_U8, torch.uint16: SAMPLE_U16, torch.float32: SAMPLE_F32}
        if dtype not in table:
            raise ValueError(f"{who}: dtype {dtype} (torch.uint8, torch.uint16, torch.float32 or None)")
        sample = table[dtype]
    plan(sample)
    return sample


def _plan_dev(m, output_bitdepth, output_chroma_format, dtype, rects=None, info=None):
    """(sample type, ccmi_frame_geom array, workspace bytes) of marshalled streams."""
    n = len(m[0])
    geom = (FrameGeom * n)()
    need = C.c_size_t(0)

    def plan(sample):
        if rects is None and info is None:
            check(_bind().ccmi_decode_batch_dev_plan(m[1], m[2], n, output_bitdepth, output_chroma_format, sample,
                                                     geom, C.byref(need)))
        else:
            check(_bind().ccmi_decode_batch_dev_roi_plan(m[1], m[2], n, rects, output_bitdepth,
                                                         output_chroma_format, sample, geom, info, C.byref(need)))
    return _pick_sample(plan, geom, dtype, "decode_batch_tensors"), geom, need.value


def decode_batch_geometry(streams: Sequence[bytes], output_bitdepth: int = 0, output_chroma_format: int = 0,
                          dtype=None, roi=None) -> tuple:
    """Header-only pass of decode_batch_tensors (ccmi_decode_batch_dev_plan / _roi_plan; no
    CABAC, no GPU):
    ([{'width', 'height', 'bitdepth', 'chroma', 'frame_data_type', 'elems'} per stream],
    device workspace bytes the same arguments need).  roi as for decode_batch_tensors: width,
    height and elems are then the region's."""
    _, geom, need = _plan_dev(_marshal(streams), output_bitdepth, output_chroma_format, dtype,
                              _rects(roi, streams, len(streams)))
    return [{k: int(getattr(g, k)) for k, _ in FrameGeom._fields_} for g in geom], need


def roi_plan(streams: Sequence[bytes], roi, output_bitdepth: int = 0, output_chroma_format: int = 0, dtype=None) -> list:
    """What a region decode will do, per stream (ccmi_decode_batch_dev_roi_plan, header-only):
    {'arm_rows': [rows of latent grid l the ARM + CABAC decode produces], 'windowed': True when
    the decoder tail runs on the region's windows, False when it runs on the whole frame and the
    output kernel crops}."""
    n = len(streams)
    info = (RoiInfo * n)()
    _plan_dev(_marshal(streams), output_bitdepth, output_chroma_format, dtype, _rects(roi, streams, n), info)
    return [{"arm_rows": [int(v) for v in i.arm_rows[: i.n_grids]], "windowed": bool(i.windowed)} for i in info]


def _alloc_outs(geom, sample, stack, dev):
    """Output tensors of a device-sink call: (the stacked allocation or None, one flat tensor
    per frame, their pointers, their capacities in bytes)."""
    import torch
    tdtype = (torch.uint8, torch.uint16, torch.float32)[sample]
    n = len(geom)
    flat = None
    if stack:
        g0 = geom[0]
        if any((g.width, g.height, g.chroma) != (g0.width, g0.height, g0.chroma) for g in geom):
            raise ValueError("decode_batch_tensors: stack=True needs outputs of one size and chroma format")
        flat = torch.empty(n, g0.elems, dtype=tdtype, device=dev)
        outs = [flat[i] for i in range(n)]
    else:
        outs = [torch.empty(g.elems, dtype=tdtype, device=dev) for g in geom]
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    cap = (C.c_size_t * n)(*[o.numel() * o.element_size() for o in outs])
    return flat, outs, op, cap


def _shape_outs(flat, outs, geom, stack):
    from .forward import split_420

    def shaped(t, g):
        return split_420(t, g.height, g.width) if g.chroma == 420 else t.reshape(*t.shape[:-1], 3, g.height, g.width)
    if stack:
        return shaped(flat, geom[0])
    return [shaped(o, g) for o, g in zip(outs, geom)]


def decode_batch_tensors(streams: Sequence[bytes], output_bitdepth: int = 0, output_chroma_format: int = 0,
                         dtype=None, stack: bool = False, workspace=None, stream_handle: int | None = None, roi=None):
    """Decode independent intra .cool streams straight into device tensors
    (ccmi_decode_batch_dev): the integers decode_batch's bytes hold, in planar tensor layout on
    the current CUDA device; no frame data crosses PCIe.

    dtype None: torch.uint8 when every output bitdepth is <= 8, else torch.uint16;
    torch.float32: sample / (2^bitdepth - 1), bitwise what u.to(float32) / maxv gives.
    Returns one item per stream: a [3, H, W] tensor for 444 output (RGB streams: planar R, G,
    B), or for 420 the {'y', 'u', 'v'} views of one flat allocation (forward.split_420).
    stack=True (one output size and chroma format required): one [n, 3, H, W] tensor, or the
    dict of [n, ., .] views over one [n, elems] allocation.  workspace: a uint8 CUDA tensor of
    at least decode_batch_geometry(...)[1] bytes, else torch's caching allocator provides it.
    roi: decode a region only (ccmi_decode_batch_dev_roi): one (x, y, w, h) in luma samples for
    every stream, or a sequence with one entry per stream (None: that stream's whole frame).
    The result is, sample for sample, the crop [y:y+h, x:x+w] of the whole-frame decode (420: x
    and y even, chroma [y/2 : y/2 + h/2, x/2 : x/2 + w/2]) and H, W above are the region's, so
    stack=True takes equal-size crops of frames of different sizes."""
    import torch
    m = _marshal(streams)
    _, sp, ln = m
    rects = _rects(roi, streams, len(streams))
    sample, geom, need = _plan_dev(m, output_bitdepth, output_chroma_format, dtype, rects)
    n = len(streams)
    dev = torch.device("cuda", torch.cuda.current_device())
    flat, outs, op, cap = _alloc_outs(geom, sample, stack, dev)
    stream_handle, workspace = _stream_ws(dev, stream_handle, workspace, need)
    if rects is None:
        check(_bind().ccmi_decode_batch_dev(sp, ln, n, op, cap, sample, output_bitdepth, output_chroma_format,
                                            workspace.data_ptr(), workspace.numel(), stream_handle))
    else:
        check(_bind().ccmi_decode_batch_dev_roi(sp, ln, n, rects, op, cap, sample, output_bitdepth,
                                                output_chroma_format, workspace.data_ptr(), workspace.numel(),
                                                stream_handle))
    return _shape_outs(flat, outs, geom, stack)


ELEM_F32, ELEM_F16, ELEM_BF16 = 0, 1, 2  # CCMI_ELEM_*
COLOUR_ASIS, COLOUR_RGB = 0, 1           # CCMI_COLOUR_*


class TensorFmt(C.Structure):
    """ccmi_tensor_fmt: the formatted output of one call."""
    _fields_ = [("elem", C.c_int), ("colour", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3),
                ("stride_c", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("mirror", C.c_void_p)]


FILTER_TRIANGLE, FILTER_CUBIC, FILTER_CLAMP = 0, 2, 0x100  # CCMI_FILTER_*


class Resample(C.Structure):
    """ccmi_resample: the output size of a resampling call."""
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("filter", C.c_int)]


def _resample(size, interp=(FILTER_TRIANGLE, 0)):
    """size=(out_h, out_w) of a *_model call -> ccmi_resample (the library checks the range);
    interp: _interp()'s pair."""
    if len(size) != 2:
        raise ValueError(f"model output: size takes (out_h, out_w), got {size!r}")
    return Resample(out_w=int(size[1]), out_h=int(size[0]), filter=interp[0])


PAD_FILL, PAD_EDGE = 0, 1  # CCMI_PAD_*
WARP_CUBIC, WARP_CLAMP, WARP_PROJECTIVE = 0x100, 0x200, 0x800  # or'ed into ccmi_warp.pad


def _interp(interpolation, clamp):
    """interpolation= / clamp= of a *_model call -> (ccmi_resample.filter, the flags of ccmi_warp.pad)."""
    if interpolation not in ("bilinear", "bicubic"):
        raise ValueError(f"model output: interpolation {interpolation!r} ('bilinear' or 'bicubic')")
    if interpolation == "bilinear":
        if clamp:
            raise ValueError("model output: clamp=True needs interpolation='bicubic'")
        return FILTER_TRIANGLE, 0
    return (FILTER_CUBIC | FILTER_CLAMP, WARP_CUBIC | WARP_CLAMP) if clamp else (FILTER_CUBIC, WARP_CUBIC)


class Warp(C.Structure):
    """ccmi_warp: the output size, the padding and the per-frame matrices of a warping call."""
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("pad", C.c_int), ("fill", C.c_float * 3),
                ("matrix", C.c_void_p)]


def _warp(affine, n, size, roi, pad, fill, interp=(FILTER_TRIANGLE, 0), perspective=None):
    """affine= or perspective= / pad= / fill= of a *_model call -> (ccmi_warp, what it points to), or
    (None, None) without either.  The library checks the values; the shapes are checked here.  interp:
    _interp()'s pair.  perspective= sets CCMI_WARP_PROJECTIVE: the matrices are [n, 3, 3]."""
    import numpy as np
    if affine is None and perspective is None:
        return None, None
    if affine is not None and perspective is not None:
        raise ValueError("model output: perspective excludes affine (a call is wholly affine or wholly projective; "
                         "an affine frame of a perspective call has the last row 0 0 1)")
    word, rows = ("affine", 2) if perspective is None else ("perspective", 3)
    if perspective is not None:
        affine, interp = perspective, (interp[0], interp[1] | WARP_PROJECTIVE)
    if size is None:
        raise ValueError(f"model output: {word} needs size=(out_h, out_w)")
    if roi is not None:
        raise ValueError(f"model output: {word} excludes roi (the matrix says where the output lies in the frame)")
    if len(size) != 2:
        raise ValueError(f"model output: size takes (out_h, out_w), got {size!r}")
    pads = {"fill": PAD_FILL, "edge": PAD_EDGE}
    if pad not in pads:
        raise ValueError(f"model output: pad {pad!r} ('fill' or 'edge')")
    a = affine.detach().cpu().numpy() if hasattr(affine, "detach") else np.asarray(affine)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape == (rows, 3):
        a = np.ascontiguousarray(np.broadcast_to(a, (n, rows, 3)))
    if a.shape != (n, rows, 3):
        raise ValueError(f"model output: {word} takes [{n}, {rows}, 3] or one [{rows}, 3], got {list(a.shape)}")
    f = [float(v) for v in fill] if hasattr(fill, "__len__") else [float(fill)] * 3
    if len(f) != 3:
        raise ValueError("model output: fill takes one value, or one per channel")
    w = Warp(out_w=int(size[1]), out_h=int(size[0]), pad=pads[pad] | interp[1], matrix=a.ctypes.data)
    for c in range(3):
        w.fill[c] = f[c]
    return w, a


def affine_matrix(size, centre, angle: float = 0.0, scale: float = 1.0, flip: bool = False):
    """The [2, 3] float32 matrix (affine= of the *_model calls) of a rotated, scaled and optionally
    flipped view: the size = (out_h, out_w) output is centred on centre = (cx, cy) of the frame
    (pixels; pixel (y, x) covers [x, x + 1) x [y, y + 1)), turned by `angle` radians and showing
    out / scale frame pixels a side.  For output row i, column k:
        dx = k + 0.5 - out_w / 2, negated if flip;   dy = i + 0.5 - out_h / 2;
        xs = cx + (cos(angle) dx - sin(angle) dy) / scale;
        ys = cy + (sin(angle) dx + cos(angle) dy) / scale."""
    import math
    import numpy as np
    oh, ow = size
    cx, cy = centre
    c, s, f = math.cos(angle), math.sin(angle), -1.0 if flip else 1.0
    return np.array([[f * c / scale, -s / scale, cx + (-f * c * ow / 2 + s * oh / 2) / scale],
                     [f * s / scale, c / scale, cy + (-f * s * ow / 2 - c * oh / 2) / scale]], dtype=np.float32)


def _perspective_f64(startpoints, endpoints):
    """perspective_matrix() before its rounding to float32."""
    import numpy as np
    s, e = np.asarray(startpoints, dtype=np.float64), np.asarray(endpoints, dtype=np.float64)
    if s.shape != (4, 2) or e.shape != (4, 2):
        raise ValueError("perspective_matrix: startpoints and endpoints take four (x, y) points each")
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        (ex, ey), (sx, sy) = e[i], s[i]
        A[2 * i] = [ex, ey, 1, 0, 0, 0, -sx * ex, -sx * ey]
        A[2 * i + 1] = [0, 0, 0, ex, ey, 1, -sy * ex, -sy * ey]
        b[2 * i], b[2 * i + 1] = sx, sy
    try:
        h = np.linalg.solve(A, b)
    except np.linalg.LinAlgError as err:
        raise ValueError("perspective_matrix: the points do not determine a homography") from err
    return np.append(h, 1.0).reshape(3, 3)


def perspective_matrix(startpoints, endpoints):
    """The [3, 3] float32 matrix (perspective= of the *_model calls), m22 = 1, of the homography that
    sends each of the four endpoints (x, y) of the OUTPUT to its startpoint (x, y) of the FRAME, in
    pixels (pixel (y, x) covers [x, x + 1) x [y, y + 1)): torchvision's _get_perspective_coeffs
    system -- per pair the two rows
        [ex, ey, 1, 0, 0, 0, -sx ex, -sx ey] . h = sx,    [0, 0, 0, ex, ey, 1, -sy ex, -sy ey] . h = sy
    -- solved in float64 (an exact solve; torchvision takes a float32 least squares).  A degenerate
    quadrilateral is a ValueError."""
    import numpy as np
    return _perspective_f64(startpoints, endpoints).astype(np.float32)


def random_perspective(n: int, size, distortion_scale: float = 0.5, p: float = 0.5, base=None, generator=None):
    """n [3, 3] float32 matrices for perspective= of the *_model calls, drawn as torchvision's
    RandomPerspective does for an image of size = (height, width) = (h, w): with hh = floor(d h / 2),
    hw = floor(d w / 2), d = distortion_scale, the four endpoints are integers drawn uniformly from
        top left      x in [0, hw],          y in [0, hh]
        top right     x in [w - hw - 1, w - 1],  y in [0, hh]
        bottom right  x in [w - hw - 1, w - 1],  y in [h - hh - 1, h - 1]
        bottom left   x in [0, hw],          y in [h - hh - 1, h - 1]
    (both ends included), and the frame's matrix is P = perspective_matrix(startpoints = (0, 0),
    (w - 1, 0), (w - 1, h - 1), (0, h - 1), endpoints = the drawn points): as F.perspective does, the
    output shows the image's own corners at the drawn points.  A frame is drawn with probability p and
    is the identity otherwise.  base: None, or [n, 2, 3] (or one [2, 3]) matrices that map the image of
    that size to the frame -- the crop / RandomResizedCrop matrices, as for rand_augment(base=...); the
    result is [base; 0 0 1] @ P, composed in float64 and rounded to float32 once.  generator: a numpy
    Generator, a seed, or None.  torchvision is not a dependency: the ranges above are the contract."""
    import numpy as np
    rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
    h, w = int(size[0]), int(size[1])
    if not 0.0 <= distortion_scale <= 1.0 or not 0.0 <= p <= 1.0:
        raise ValueError("random_perspective: distortion_scale and p lie in [0, 1]")
    hh, hw = int(distortion_scale * h / 2), int(distortion_scale * w / 2)
    if base is not None:
        base = np.asarray(base.detach().cpu().numpy() if hasattr(base, "detach") else base, dtype=np.float64)
        if base.shape == (2, 3):
            base = np.broadcast_to(base, (n, 2, 3))
        if base.shape != (n, 2, 3):
            raise ValueError(f"random_perspective: base takes [{n}, 2, 3] or one [2, 3], got {list(base.shape)}")
    starts = [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)]
    out = np.empty((n, 3, 3), dtype=np.float32)
    for j in range(n):
        P = np.eye(3)
        if rng.random() < p:
            xl, xr = rng.integers(0, hw + 1, 2), rng.integers(w - hw - 1, w, 2)
            yt, yb = rng.integers(0, hh + 1, 2), rng.integers(h - hh - 1, h, 2)
            P = _perspective_f64(starts, [(xl[0], yt[0]), (xr[0], yt[1]), (xr[1], yb[0]), (xl[1], yb[1])])
        if base is not None:
            P = np.vstack([base[j], [0.0, 0.0, 1.0]]) @ P
        out[j] = P
    return out


COL_BRIGHTNESS, COL_SATURATION, COL_CONTRAST, COL_MATRIX = 0, 1, 2, 3  # CCMI_COL_*
COL_MAX_OPS = 8
_COL_NAMES = {"brightness": COL_BRIGHTNESS, "saturation": COL_SATURATION, "contrast": COL_CONTRAST, "matrix": COL_MATRIX}


class ColourOp(C.Structure):
    """ccmi_colour_op: one photometric operation (v[0] the factor, or the 3 x 4 matrix row-major)."""
    _fields_ = [("op", C.c_int), ("v", C.c_float * 12)]


class Colour(C.Structure):
    """ccmi_colour: the per-frame op counts and the flat op array of a colouring call."""
    _fields_ = [("count", C.c_void_p), ("ops", C.c_void_p)]


def _colour(colour_ops, n):
    """colour_ops= of a *_model call -> (ccmi_colour, what it points to), or (None, None) without ops.
    One list of (op, value) tuples for every frame, or one such list per frame; op is 'brightness',
    'saturation', 'contrast' or 'matrix' (or a COL_* code), value the factor, or the matrix as 12
    numbers or [3][4].  The library checks the values; the shapes are checked here."""
    import numpy as np
    if colour_ops is None:
        return None, None
    ops = list(colour_ops)
    if not ops:
        return None, None
    if isinstance(ops[0], tuple) and len(ops[0]) == 2 and isinstance(ops[0][0], (str, int)):
        ops = [ops] * n  # one list for all frames
    if len(ops) != n:
        raise ValueError(f"model output: colour_ops takes one op list, or one per frame ({n}), got {len(ops)}")
    counts = np.fromiter((len(f) for f in ops), dtype=np.int32, count=n)
    # ccmi_colour_op as a packed record (52 bytes): filled row by row, no per-element ctypes stores
    flat = np.zeros(max(int(counts.sum()), 1), dtype=np.dtype([("op", "<i4"), ("v", "<f4", (12,))]))
    codes, at_f, fs, at_m, ms = [], [], [], [], []  # gathered in one pass, stored in bulk
    for f in ops:
        for op, value in f:
            code = _COL_NAMES.get(op) if isinstance(op, str) else int(op)
            if code is None:
                raise ValueError(f"model output: colour op {op!r} ({', '.join(_COL_NAMES)})")
            if code == COL_MATRIX:
                at_m.append(len(codes))
                ms.append(value)
            else:
                at_f.append(len(codes))
                fs.append(value)
            codes.append(code)
    if codes:
        flat["op"] = codes
    if fs:
        fs = np.asarray(fs, dtype=np.float32)
        if fs.ndim != 1:
            raise ValueError("model output: a brightness / saturation / contrast op takes one factor")
        flat["v"][at_f, 0] = fs
    if ms:
        try:
            ms = np.asarray(ms, dtype=np.float32).reshape(len(at_m), 12)
        except ValueError:
            raise ValueError("model output: a matrix colour op takes a 3 x 4 matrix (12 values)") from None
        flat["v"][at_m] = ms
    return Colour(count=counts.ctypes.data, ops=flat.ctypes.data), (counts, flat)


# RGB -> YIQ (NTSC); rows 1 and 2 sum to 0, so a grey pixel has no chroma and every rotation keeps it
_YIQ = ((0.299, 0.587, 0.114), (0.595716, -0.274453, -0.321263), (0.211456, -0.522591, 0.311135))


def hue_matrix(h: float):
    """The [3, 4] float32 matrix of a 'matrix' colour op that turns the hue by h turns: RGB -> YIQ,
    a rotation of the (I, Q) plane by 2 pi h, YIQ -> RGB, composed in float64 and rounded once.  Luma
    and greys are kept; the result is clamped to [0, 1] per channel by the op.  It is NOT
    torchvision's adjust_hue, which shifts H of HSV."""
    import math
    import numpy as np
    t = np.array(_YIQ, dtype=np.float64)
    c, s = math.cos(2 * math.pi * h), math.sin(2 * math.pi * h)
    r = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    m = np.zeros((3, 4), dtype=np.float64)
    m[:, :3] = np.linalg.inv(t) @ r @ t
    return m.astype(np.float32)


def grey_matrix():
    """The [3, 4] float32 matrix of a 'matrix' colour op that sets every channel to the grey
    0.2989 R + 0.587 G + 0.114 B (RandomGrayscale with three output channels)."""
    import numpy as np
    return np.array([[0.2989, 0.587, 0.114, 0.0]] * 3, dtype=np.float32)


def colour_jitter(n: int, brightness: float = 0.0, contrast: float = 0.0, saturation: float = 0.0, hue: float = 0.0,
                  grey_p: float = 0.0, generator=None) -> list:
    """n op lists (colour_ops= of the *_model calls) drawn as torchvision's ColorJitter draws them:
    brightness / contrast / saturation = b gives a factor in U[max(0, 1 - b), 1 + b], hue = h a turn
    in U[-h, h] (hue_matrix), an argument of 0 leaves its op out, and every frame applies its ops in
    a random order of its own.  grey_p: with that probability a frame ends with grey_matrix()
    (RandomGrayscale).  generator: a torch.Generator (CPU); the same seed gives the same lists."""
    import torch
    kinds = [(name, float(b)) for name, b in (("brightness", brightness), ("contrast", contrast),
                                              ("saturation", saturation), ("hue", hue)) if b]
    for name, b in kinds:
        if b < 0 or (name == "hue" and b > 0.5):
            raise ValueError(f"colour_jitter: {name} = {b}")
    out = []
    for _ in range(n):
        u = torch.rand(len(kinds) + 1, generator=generator, dtype=torch.float64).tolist()
        order = torch.randperm(len(kinds), generator=generator).tolist() if kinds else []
        ops = []
        for k in order:
            name, b = kinds[k]
            if name == "hue":
                ops.append(("matrix", hue_matrix(-b + 2 * b * u[k])))
            else:
                lo = max(0.0, 1.0 - b)
                ops.append((name, lo + (1.0 + b - lo) * u[k]))
        if grey_p and u[-1] < grey_p:
            ops.append(("matrix", grey_matrix()))
        out.append(ops)
    return out


FLT_MAX_RADIUS = 15


class Filter(C.Structure):
    """ccmi_filter: the per-frame radii, the flat half taps and the per-frame solarize thresholds."""
    _fields_ = [("radius", C.c_void_p), ("taps", C.c_void_p), ("solarize", C.c_void_p)]


def _filter(blur, solarize, n):
    """blur= / solarize= of a *_model call -> (ccmi_filter, what it points to), or (None, None) with
    both None.  blur: one entry for every frame, or one per frame; an entry is None (no blur) or a 1-D
    float32 array of half taps w_0 (centre) .. w_r.  solarize: None, one threshold for every frame, or
    one per frame (None or a value above 1: off).  The library checks the values; the shapes are
    checked here."""
    import numpy as np
    if blur is None and solarize is None:
        return None, None
    if blur is None:
        entries = [None] * n
    elif isinstance(blur, (list, tuple)) and (len(blur) == 0 or blur[0] is None or hasattr(blur[0], "__len__")):
        entries = list(blur)  # one per frame
    else:
        entries = [blur] * n  # one array of taps for all frames
    if len(entries) != n:
        raise ValueError(f"model output: blur takes one entry, or one per frame ({n}), got {len(entries)}")
    taps = []
    for e in entries:
        t = np.zeros(0, dtype=np.float32) if e is None else np.asarray(e, dtype=np.float32)
        if t.ndim != 1 or t.size - 1 > FLT_MAX_RADIUS:
            raise ValueError(f"model output: a blur entry is None or 1 .. {FLT_MAX_RADIUS + 1} half taps, got shape "
                             f"{tuple(t.shape)}")
        taps.append(t if t.size > 1 else t[:0])  # a centre tap alone is radius 0: no blur
    radius = np.fromiter((max(t.size - 1, 0) for t in taps), dtype=np.int32, count=n)
    flat = np.ascontiguousarray(np.concatenate(taps + [np.zeros(1, dtype=np.float32)]), dtype=np.float32)
    th = None
    if solarize is not None:
        s = [solarize] * n if not hasattr(solarize, "__len__") else list(solarize)
        if len(s) != n:
            raise ValueError(f"model output: solarize takes one threshold, or one per frame ({n}), got {len(s)}")
        th = np.array([2.0 if v is None else float(v) for v in s], dtype=np.float32)
    flt = Filter(radius=radius.ctypes.data, taps=flat.ctypes.data, solarize=None if th is None else th.ctypes.data)
    return flt, (radius, flat, th)


def gaussian_taps(sigma: float, kernel_size: int):
    """The half taps w_0 (centre) .. w_r, r = (kernel_size - 1) / 2, of torchvision's Gaussian kernel
    (_get_gaussian_kernel1d, restated in torch CPU float32 operations): half = (k - 1) 0.5,
    x = linspace(-half, half, k), pdf = exp(-0.5 (x / sigma)^2), pdf / pdf.sum().  A float32 numpy
    array for blur= of the *_model calls; raises if the full kernel is not symmetric bit for bit."""
    import torch
    k = int(kernel_size)
    if k < 1 or k % 2 == 0 or (k - 1) // 2 > FLT_MAX_RADIUS:
        raise ValueError(f"gaussian_taps: kernel_size {kernel_size} (odd, 1 .. {2 * FLT_MAX_RADIUS + 1})")
    if not sigma > 0:
        raise ValueError(f"gaussian_taps: sigma {sigma}")
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    kern = pdf / pdf.sum()
    if not torch.equal(kern, kern.flip(0)):
        raise ValueError(f"gaussian_taps: the kernel of sigma {sigma}, size {k} is not symmetric in float32")
    return kern[k // 2:].contiguous().numpy()


def gaussian_blur(n: int, kernel_size: int, sigma=(0.1, 2.0), p: float = 1.0, generator=None) -> list:
    """n blur entries (blur= of the *_model calls) drawn as torchvision's GaussianBlur under
    RandomApply(p) draws them: with probability p a frame gets gaussian_taps(s, kernel_size) with s in
    U[sigma[0], sigma[1]], else None.  generator: a torch.Generator (CPU); the same seed gives the
    same list."""
    import torch
    lo, hi = (float(sigma), float(sigma)) if not hasattr(sigma, "__len__") else (float(sigma[0]), float(sigma[1]))
    if not 0 < lo <= hi:
        raise ValueError(f"gaussian_blur: sigma {sigma}")
    out = []
    for _ in range(n):
        u = torch.rand(2, generator=generator, dtype=torch.float64).tolist()
        out.append(gaussian_taps(lo + (hi - lo) * u[1], kernel_size) if u[0] < p else None)
    return out


def random_solarize(n: int, threshold: float = 0.5, p: float = 0.2, generator=None) -> list:
    """n solarize thresholds (solarize= of the *_model calls) drawn as torchvision's RandomSolarize
    draws them: with probability p a frame gets `threshold`, else None (off).  generator: a
    torch.Generator (CPU); the same seed gives the same list."""
    import torch
    u = torch.rand(n, generator=generator, dtype=torch.float64).tolist()
    return [float(threshold) if v < p else None for v in u]


TONE_BRIGHTNESS, TONE_SATURATION, TONE_CONTRAST, TONE_MATRIX, TONE_SOLARIZE = 0, 1, 2, 3, 4  # CCMI_TONE_*
TONE_POSTERIZE, TONE_AUTOCONTRAST, TONE_EQUALIZE, TONE_SHARPNESS = 5, 6, 7, 8
TONE_MAX_OPS = 8
_TONE_NAMES = {"brightness": TONE_BRIGHTNESS, "saturation": TONE_SATURATION, "contrast": TONE_CONTRAST,
               "matrix": TONE_MATRIX, "solarize": TONE_SOLARIZE, "posterize": TONE_POSTERIZE,
               "autocontrast": TONE_AUTOCONTRAST, "equalize": TONE_EQUALIZE, "sharpness": TONE_SHARPNESS}


class ToneOp(C.Structure):
    """ccmi_tone_op: one tone operation (v[0] the factor, threshold or bits, or the 3 x 4 matrix row-major)."""
    _fields_ = [("op", C.c_int), ("v", C.c_float * 12)]


class Tone(C.Structure):
    """ccmi_tone: the per-frame op counts and the flat op array of a call with tone ops."""
    _fields_ = [("count", C.c_void_p), ("ops", C.c_void_p)]


def _tone(tone_ops, n):
    """tone_ops= of a *_model call -> (ccmi_tone, what it points to), or (None, None) without ops.
    One list of (op, value) tuples for every frame, or one such list per frame; op is a name of
    _TONE_NAMES (or a TONE_* code), value the factor, threshold or bits, the matrix as 12 numbers or
    [3][4], and None for 'autocontrast' and 'equalize'.  The library checks the values."""
    import numpy as np
    if tone_ops is None:
        return None, None
    ops = list(tone_ops)
    if not ops:
        return None, None
    if isinstance(ops[0], tuple) and len(ops[0]) == 2 and isinstance(ops[0][0], (str, int)):
        ops = [ops] * n  # one list for all frames
    if len(ops) != n:
        raise ValueError(f"model output: tone_ops takes one op list, or one per frame ({n}), got {len(ops)}")
    counts = np.fromiter((len(f) for f in ops), dtype=np.int32, count=n)
    if not counts.any():
        return None, None
    flat = np.zeros(int(counts.sum()), dtype=np.dtype([("op", "<i4"), ("v", "<f4", (12,))]))
    k = 0
    for f in ops:
        for op, value in f:
            code = _TONE_NAMES.get(op) if isinstance(op, str) else int(op)
            if code is None:
                raise ValueError(f"model output: tone op {op!r} ({', '.join(_TONE_NAMES)})")
            flat["op"][k] = code
            if code == TONE_MATRIX:
                try:
                    flat["v"][k] = np.asarray(value, dtype=np.float32).reshape(12)
                except ValueError:
                    raise ValueError("model output: a matrix tone op takes a 3 x 4 matrix (12 values)") from None
            elif value is not None:
                flat["v"][k, 0] = np.float32(value)
            k += 1
    return Tone(count=counts.ctypes.data, ops=flat.ctypes.data), (counts, flat)


# torchvision's op table (RandAugment._augmentation_space): name, signed
_RA_OPS = (("Identity", False), ("ShearX", True), ("ShearY", True), ("TranslateX", True), ("TranslateY", True),
           ("Rotate", True), ("Brightness", True), ("Color", True), ("Contrast", True), ("Sharpness", True),
           ("Posterize", False), ("Solarize", False), ("AutoContrast", False), ("Equalize", False))


def _ra_magnitude(name, k, bins, size, wide):
    """The magnitude of bin k of op `name`: torchvision's RandAugment table, or TrivialAugmentWide's."""
    import numpy as np
    lin = lambda hi: float(np.linspace(0.0, hi, bins)[k])  # noqa: E731
    if name in ("ShearX", "ShearY", "Brightness", "Color", "Contrast", "Sharpness"):
        return lin(0.99 if wide else (0.3 if name.startswith("Shear") else 0.9))
    if name == "TranslateX":
        return lin(32.0 if wide else 150.0 / 331.0 * size[1])
    if name == "TranslateY":
        return lin(32.0 if wide else 150.0 / 331.0 * size[0])
    if name == "Rotate":
        return lin(135.0 if wide else 30.0)
    if name == "Posterize":
        return float(8 - int(round(k / ((bins - 1) / (6 if wide else 4)))))
    if name == "Solarize":
        return float(np.linspace(1.0, 0.0, bins)[k])  # the v2 transform's float threshold
    return 0.0


def _ra_apply(name, mag, size, geo, tone):
    """One drawn op: a geometric one is composed into geo (3 x 3, output pixel -> input pixel of an image of
    `size`, pixel centres at + 0.5), a photometric one appended to tone."""
    import math
    import numpy as np
    h, w = size
    m = np.eye(3)
    if name == "ShearX":
        m[0, 1] = mag  # F.affine(shear=[atan(mag), 0], center=[0, 0]): x_in = x + mag y
    elif name == "ShearY":
        m[1, 0] = mag
    elif name == "TranslateX":
        m[0, 2] = -float(int(mag))
    elif name == "TranslateY":
        m[1, 2] = -float(int(mag))
    elif name == "Rotate":  # F.rotate: counter-clockwise about the image's centre
        c, s = math.cos(math.radians(mag)), math.sin(math.radians(mag))
        m[:2, :2] = [[c, -s], [s, c]]
        m[0, 2] = w / 2 - c * w / 2 + s * h / 2
        m[1, 2] = h / 2 - s * w / 2 - c * h / 2
    elif name == "Brightness":
        tone.append(("brightness", 1.0 + mag))
    elif name == "Color":
        tone.append(("saturation", 1.0 + mag))
    elif name == "Contrast":
        tone.append(("contrast", 1.0 + mag))
    elif name == "Sharpness":
        tone.append(("sharpness", 1.0 + mag))
    elif name == "Posterize":
        tone.append(("posterize", mag))
    elif name == "Solarize":
        tone.append(("solarize", mag))
    elif name == "AutoContrast":
        tone.append(("autocontrast", None))
    elif name == "Equalize":
        tone.append(("equalize", None))
    return geo @ m


def _ra_draw(n, num_ops, magnitude, bins, generator, size, base, wide):
    import numpy as np
    import torch
    size = (int(size[0]), int(size[1]))
    if base is not None:
        base = np.asarray(base, dtype=np.float64).reshape(-1, 2, 3)
        if base.shape[0] not in (1, n):
            raise ValueError(f"augment: base takes one [2, 3] matrix, or one per frame ({n}), got {base.shape[0]}")
    mats, tones = np.zeros((n, 2, 3), dtype=np.float32), []
    for j in range(n):
        geo = np.eye(3)
        if base is not None:
            geo[:2] = base[j % base.shape[0]]
        tone = []
        for _ in range(num_ops):
            name, signed = _RA_OPS[int(torch.randint(len(_RA_OPS), (1,), generator=generator))]
            k = int(torch.randint(bins, (1,), generator=generator)) if wide else int(magnitude)
            mag = _ra_magnitude(name, k, bins, size, wide)
            if signed and int(torch.randint(2, (1,), generator=generator)):
                mag = -mag
            geo = _ra_apply(name, mag, size, geo, tone)
        mats[j] = geo[:2]
        tones.append(tone)
    return mats, tones


def rand_augment(n: int, num_ops: int = 2, magnitude: int = 9, num_magnitude_bins: int = 31, generator=None,
                 size=(224, 224), base=None):
    """n draws of torchvision's RandAugment(num_ops, magnitude, num_magnitude_bins) from its op table and
    magnitude ranges: (matrices, tone lists) for affine= and tone_ops= of the *_model calls (with
    size=size).  matrices: float32 [n, 2, 3]; the geometric draws of a frame (ShearX/Y, TranslateX/Y,
    Rotate) composed into ONE matrix that maps an output pixel of the size x size image to a pixel of
    the image before (pixel centres at + 0.5), after `base` (None: the identity; else one [2, 3] matrix
    or one per frame that maps the output image to the frame, e.g. affine_matrix()'s crop).  tone
    lists: the photometric draws in their order (Brightness, Color, Contrast, Sharpness as 1 +- m;
    Posterize bits; Solarize as the v2 transform's threshold in [0, 1]; AutoContrast; Equalize).
    Geometry always runs first, in one bilinear warp (torchvision resamples once per op, nearest by
    default): the result follows torchvision's when a frame's photometric ops come after its geometric
    ones; when one comes before, the statistics of autocontrast / equalize / contrast see the fill
    pixels the later warp brings in, and torchvision's do not.  magnitude must be below
    num_magnitude_bins.  generator: a torch.Generator (CPU); the same seed gives the same draws."""
    if not 0 <= int(magnitude) < int(num_magnitude_bins):
        raise ValueError(f"rand_augment: magnitude {magnitude} of {num_magnitude_bins} bins")
    if not 0 <= int(num_ops) <= TONE_MAX_OPS:
        raise ValueError(f"rand_augment: num_ops {num_ops} (0 .. {TONE_MAX_OPS})")
    return _ra_draw(n, int(num_ops), magnitude, int(num_magnitude_bins), generator, size, base, False)


def trivial_augment_wide(n: int, num_magnitude_bins: int = 31, generator=None, size=(224, 224), base=None):
    """n draws of torchvision's TrivialAugmentWide: one op per frame, its magnitude bin drawn uniformly, from
    the wide ranges (shear and the factors to 0.99, translate to 32 pixels, rotate to 135 degrees,
    posterize down to 2 bits).  Returns what rand_augment() returns, with the same caveats."""
    return _ra_draw(n, 1, 0, int(num_magnitude_bins), generator, size, base, True)


# AugMix's op table (torchvision's AugMix._augmentation_space): name, signed; the last four with all_ops
_AM_OPS = (("ShearX", True), ("ShearY", True), ("TranslateX", True), ("TranslateY", True), ("Rotate", True),
           ("Posterize", False), ("Solarize", False), ("AutoContrast", False), ("Equalize", False),
           ("Brightness", True), ("Color", True), ("Contrast", True), ("Sharpness", True))
_AM_BINS = 10  # torchvision's _PARAMETER_MAX


def _am_magnitude(name, k, size):
    """The magnitude of bin k of 10 of AugMix's op `name` for frames of `size` = (H, W)."""
    import numpy as np
    lin = lambda hi: float(np.linspace(0.0, hi, _AM_BINS)[k])  # noqa: E731
    if name in ("ShearX", "ShearY"):
        return lin(0.3)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return lin(0.9)
    if name == "TranslateX":
        return lin(size[1] / 3.0)
    if name == "TranslateY":
        return lin(size[0] / 3.0)
    if name == "Rotate":
        return lin(30.0)
    if name == "Posterize":
        return float(max(4 - int(round(k / ((_AM_BINS - 1) / 4))), 1))  # the library posterizes to 1 .. 8 bits
    if name == "Solarize":
        return float(np.linspace(1.0, 0.0, _AM_BINS)[k])
    return 0.0


def aug_mix(n: int, size, severity: int = 3, mixture_width: int = 3, chain_depth: int = -1, alpha: float = 1.0,
            all_ops: bool = True, generator=None, base=None) -> dict:
    """n draws of torchvision's AugMix(severity, mixture_width, chain_depth, alpha, all_ops) for frames stored
    at size = (H, W), as ONE call of m = n (1 + mixture_width) frames of the *_model calls: a dict with
      'repeat'    int array [m]: frame j of the call is frame repeat[j] of the n (repeat index, roi and
                  mirror by it: a frame and its chains share them),
      'matrices'  float32 [m, 2, 3] for affine= (with size=size),
      'tone_ops'  m tone lists for tone_ops=,
      'blend'     m entries for blend=,  'silent'  m flags for silent=.
    Frame j (1 + width) is frame j itself, clean: the base matrix (None: the identity; else one [2, 3]
    matrix or one per frame of the n, as for rand_augment()), no tone ops, not silent, and the blend list
    [(itself, m_0), (chain 1, w_1), ..., (chain width, w_width)].  Its chains follow it and are silent, so
    the call returns n frames.
    A chain is chain_depth ops (<= 0: 1 .. 3, drawn uniformly), each drawn uniformly from the op table:
    ShearX, ShearY (0 .. 0.3), TranslateX, TranslateY (0 .. W / 3, H / 3 pixels), Rotate (0 .. 30 degrees),
    Posterize (4 - round(bin / 2.25) bits: 4 .. 1; torchvision's 0 bits at bins 8 and 9, a black frame, is
    drawn as 1 bit), Solarize (threshold 1 .. 0), AutoContrast, Equalize, and with
    all_ops Brightness, Color, Contrast, Sharpness (1 +- 0 .. 0.9).  The magnitude is one of 10 bins, its
    index drawn uniformly below severity (1 .. 10); signed ops take a random sign.
    Weights: (m_0, m_1) ~ Beta(alpha, alpha) as a Dirichlet of two, (d_1 .. d_width) ~ Dirichlet(alpha),
    w_i = d_i m_1, all rounded to float32 here: non-negative, and m_0 + sum w_i = 1 within float32 rounding.
    As in rand_augment(), a chain's geometric ops are composed into one matrix that runs first, in one
    warp, and its photometric ops follow in their order; AugMix's interleaving inside a chain is not
    reproduced, with rand_augment()'s caveat for statistics ops.  generator: a torch.Generator (CPU); the
    same seed gives the same draws."""
    import numpy as np
    import torch
    size = (int(size[0]), int(size[1]))
    width, depth = int(mixture_width), int(chain_depth)
    if not 1 <= int(severity) <= _AM_BINS:
        raise ValueError(f"aug_mix: severity {severity} (1 .. {_AM_BINS})")
    if not 1 <= width <= BLEND_MAX_TERMS - 1:
        raise ValueError(f"aug_mix: mixture_width {mixture_width} (1 .. {BLEND_MAX_TERMS - 1})")
    if depth > TONE_MAX_OPS:
        raise ValueError(f"aug_mix: chain_depth {chain_depth} (at most {TONE_MAX_OPS})")
    if base is not None:
        base = np.asarray(base, dtype=np.float64).reshape(-1, 2, 3)
        if base.shape[0] not in (1, n):
            raise ValueError(f"augment: base takes one [2, 3] matrix, or one per frame ({n}), got {base.shape[0]}")
    ops = _AM_OPS if all_ops else _AM_OPS[:9]
    m = n * (1 + width)
    mats, tones, blend = np.zeros((m, 2, 3), dtype=np.float32), [], []
    # torch has no public Dirichlet or gamma draw that takes a generator; this private one is what torchvision's
    # AugMix calls (torch.distributions.Dirichlet would draw from the global generator instead)
    if not hasattr(torch, "_sample_dirichlet"):
        raise RuntimeError("aug_mix: this torch has no torch._sample_dirichlet(concentration, generator)")
    two = torch._sample_dirichlet(torch.full((n, 2), float(alpha), dtype=torch.float64), generator)
    chains = torch._sample_dirichlet(torch.full((n, width), float(alpha), dtype=torch.float64), generator)
    weights = torch.cat([two[:, :1], chains * two[:, 1:]], dim=1).to(torch.float32).numpy()
    for j in range(n):
        clean = j * (1 + width)
        geo0 = np.eye(3)
        if base is not None:
            geo0[:2] = base[j % base.shape[0]]
        mats[clean] = geo0[:2]
        tones.append([])
        blend.append([(clean + i, float(weights[j, i])) for i in range(1 + width)])
        for i in range(width):
            geo, tone = geo0.copy(), []
            d = depth if depth > 0 else int(torch.randint(1, 4, (1,), generator=generator))
            for _ in range(d):
                name, signed = ops[int(torch.randint(len(ops), (1,), generator=generator))]
                k = int(torch.randint(int(severity), (1,), generator=generator))
                mag = _am_magnitude(name, k, size)
                if signed and int(torch.randint(2, (1,), generator=generator)):
                    mag = -mag
                geo = _ra_apply(name, mag, size, geo, tone)
            mats[clean + 1 + i] = geo[:2]
            tones.append(tone)
            blend.append(None)
    silent = [(j % (1 + width)) != 0 for j in range(m)]
    return {"repeat": np.repeat(np.arange(n), 1 + width), "matrices": mats, "tone_ops": tones, "blend": blend,
            "silent": silent}


# AutoAugment's ImageNet policy (torchvision's AutoAugment._get_policies): 25 pairs of (op, probability, bin)
_AA_IMAGENET = (
    (("Posterize", 0.4, 8), ("Rotate", 0.6, 9)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)), (("Posterize", 0.6, 7), ("Posterize", 0.6, 6)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Equalize", 0.4, None), ("Rotate", 0.8, 8)),
    (("Solarize", 0.6, 3), ("Equalize", 0.6, None)), (("Posterize", 0.8, 5), ("Equalize", 1.0, None)),
    (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)), (("Equalize", 0.6, None), ("Posterize", 0.4, 6)),
    (("Rotate", 0.8, 8), ("Color", 0.4, 0)), (("Rotate", 0.4, 9), ("Equalize", 0.6, None)),
    (("Equalize", 0.0, None), ("Equalize", 0.8, None)), (("Invert", 0.6, None), ("Equalize", 1.0, None)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)), (("Rotate", 0.8, 8), ("Color", 1.0, 2)),
    (("Color", 0.8, 8), ("Solarize", 0.8, 7)), (("Sharpness", 0.4, 7), ("Invert", 0.6, None)),
    (("ShearX", 0.6, 5), ("Equalize", 1.0, None)), (("Color", 0.4, 0), ("Equalize", 0.6, None)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Invert", 0.6, None), ("Equalize", 1.0, None)), (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)))
_AA_SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
_INVERT = ((-1.0, 0.0, 0.0, 1.0), (0.0, -1.0, 0.0, 1.0), (0.0, 0.0, -1.0, 1.0))  # 1 - x as a matrix tone op


def auto_augment(n: int, policy: str = "imagenet", generator=None, size=(224, 224), base=None):
    """n draws of torchvision's AutoAugment(AutoAugmentPolicy.IMAGENET): what rand_augment() returns,
    (matrices, tone lists), with the same composition and caveats.  Per frame one of the policy's 25
    sub-policies is drawn uniformly; each of its two ops is applied with its probability at its bin of 10:
    ShearX 0 .. 0.3, Rotate 0 .. 30 degrees, Color, Contrast and Sharpness 1 +- 0 .. 0.9 (signed ops take a
    random sign), Posterize 8 - round(bin / 2.25) bits (8 .. 4), Solarize threshold 1 .. 0, AutoContrast,
    Equalize, and Invert, which is the matrix tone op 1 - x.  generator: a torch.Generator (CPU); the same
    seed gives the same draws."""
    import numpy as np
    import torch
    if policy != "imagenet":
        raise ValueError(f"auto_augment: policy {policy!r} ('imagenet')")
    size = (int(size[0]), int(size[1]))
    if base is not None:
        base = np.asarray(base, dtype=np.float64).reshape(-1, 2, 3)
        if base.shape[0] not in (1, n):
            raise ValueError(f"augment: base takes one [2, 3] matrix, or one per frame ({n}), got {base.shape[0]}")
    mats, tones = np.zeros((n, 2, 3), dtype=np.float32), []
    for j in range(n):
        geo = np.eye(3)
        if base is not None:
            geo[:2] = base[j % base.shape[0]]
        tone = []
        sub = _AA_IMAGENET[int(torch.randint(len(_AA_IMAGENET), (1,), generator=generator))]
        probs = torch.rand(2, generator=generator, dtype=torch.float64).tolist()
        signs = torch.randint(2, (2,), generator=generator).tolist()
        for (name, p, k), u, sign in zip(sub, probs, signs):
            if not u <= p:
                continue
            if name == "Invert":
                tone.append(("matrix", _INVERT))
                continue
            mag = _ra_magnitude(name, k, _AM_BINS, size, False) if k is not None else 0.0
            if name in _AA_SIGNED and sign:
                mag = -mag
            geo = _ra_apply(name, mag, size, geo, tone)
        mats[j] = geo[:2]
        tones.append(tone)
    return mats, tones


MIX_MAX_RECTS = 4  # CCMI_MIX_MAX_RECTS


class EraseRect(C.Structure):
    """ccmi_erase_rect: one erase rectangle in stored coordinates, its value per channel and its sigma."""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int), ("v", C.c_float * 3), ("sigma", C.c_float)]


class Mix(C.Structure):
    """ccmi_mix: per-frame rectangle counts, the flat rectangles, seeds, partners, blend weights and boxes."""
    _fields_ = [("count", C.c_void_p), ("rects", C.c_void_p), ("seed", C.c_void_p), ("partner", C.c_void_p),
                ("lam", C.c_void_p), ("box", C.c_void_p)]


def _mix(erase, erase_seed, mix, n):
    """erase= / erase_seed= / mix= of a *_model call -> (ccmi_mix, what it points to), or (None, None) with
    all three None.  erase: one entry per frame, None or a list of at most 4 (x, y, w, h, value[, sigma]) in
    stored coordinates (after mirror), value one float or three, in the normalised units; erase_seed: one
    int for every frame or one per frame (the noise of rectangles with sigma > 0); mix: one entry per
    frame, None, (partner, lam) or (partner, (x, y, w, h)).  The library checks the values; the shapes
    are checked here."""
    import numpy as np
    if erase is None and mix is None:
        return None, None
    counts = np.zeros(n, dtype=np.int32)
    rects = []
    if erase is not None:
        entries = list(erase)
        if len(entries) != n:
            raise ValueError(f"model output: erase takes one entry per frame ({n}), got {len(entries)}")
        for j, e in enumerate(entries):
            e = [] if e is None else list(e)
            if len(e) > MIX_MAX_RECTS:
                raise ValueError(f"model output: frame {j}: {len(e)} erase rectangles (at most {MIX_MAX_RECTS})")
            counts[j] = len(e)
            for r in e:
                if len(r) not in (5, 6):
                    raise ValueError("model output: an erase rectangle is (x, y, w, h, value[, sigma])")
                v = [float(t) for t in r[4]] if hasattr(r[4], "__len__") else [float(r[4])] * 3
                if len(v) != 3:
                    raise ValueError("model output: an erase value is one float or one per channel")
                rects.append((int(r[0]), int(r[1]), int(r[2]), int(r[3]), v, float(r[5]) if len(r) == 6 else 0.0))
    flat = (EraseRect * max(len(rects), 1))()
    for k, (x, y, w, h, v, sigma) in enumerate(rects):
        flat[k] = EraseRect(x, y, w, h, (C.c_float * 3)(*v), sigma)
    if erase_seed is None:
        seeds = np.zeros(n, dtype=np.uint64)
    elif hasattr(erase_seed, "__len__"):
        if len(erase_seed) != n:
            raise ValueError(f"model output: erase_seed takes one int, or one per frame ({n}), got {len(erase_seed)}")
        seeds = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in erase_seed], dtype=np.uint64)
    else:
        seeds = np.full(n, int(erase_seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    partner = np.full(n, -1, dtype=np.int32)
    lam = np.ones(n, dtype=np.float32)
    box = (Rect * n)()
    if mix is not None:
        entries = list(mix)
        if len(entries) != n:
            raise ValueError(f"model output: mix takes one entry per frame ({n}), got {len(entries)}")
        for j, e in enumerate(entries):
            if e is None:
                continue
            if len(e) != 2:
                raise ValueError("model output: a mix entry is None, (partner, lam) or (partner, (x, y, w, h))")
            partner[j] = int(e[0])
            if hasattr(e[1], "__len__"):
                if len(e[1]) != 4:
                    raise ValueError("model output: a mix box is (x, y, w, h)")
                box[j] = Rect(*[int(t) for t in e[1]])
            else:
                lam[j] = np.float32(e[1])
    mx = Mix(count=counts.ctypes.data, rects=C.addressof(flat), seed=seeds.ctypes.data, partner=partner.ctypes.data,
             lam=lam.ctypes.data, box=C.addressof(box))
    return mx, (counts, flat, seeds, partner, lam, box)


def random_erasing(n: int, size, p: float = 0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0.0, count: int = 1,
                   generator=None):
    """n draws of torchvision's RandomErasing(p, scale, ratio, value) for frames stored at size = (H, W):
    (erase, seeds) for erase= and erase_seed= of the *_model calls.  Per frame, with probability p, `count`
    rectangles (timm's max_count; torchvision has 1), each by RandomErasing.get_params: up to 10 attempts of
    area = H W U[scale], aspect = exp(U[log ratio[0], log ratio[1]]), h = round(sqrt(area aspect)),
    w = round(sqrt(area / aspect)), accepted when h < H and w < W (and neither is 0), then the origin
    uniform over the integers y in [0, H - h], x in [0, W - w]; ten rejections give no rectangle.
    value: one float or three, in the normalised units (sigma 0), or "pixel": value 0, sigma 1 (a unit
    Gaussian per element, as torchvision's value="random" and timm's mode="pixel") with one 63-bit seed
    per frame drawn from the generator; seeds is None otherwise.  A frame consumes a fixed number of
    draws (float64), so frame j's rectangles do not depend on what the frames before it were given.
    generator: a torch.Generator (CPU); the same seed gives the same lists."""
    import math
    import torch
    H, W = int(size[0]), int(size[1])
    if not (0.0 <= p <= 1.0) or not 0 < scale[0] <= scale[1] or not 0 < ratio[0] <= ratio[1]:
        raise ValueError(f"random_erasing: p {p}, scale {scale}, ratio {ratio}")
    if not 1 <= int(count) <= MIX_MAX_RECTS:
        raise ValueError(f"random_erasing: count {count} (1 .. {MIX_MAX_RECTS})")
    pixel = isinstance(value, str)
    if pixel and value != "pixel":
        raise ValueError(f"random_erasing: value {value!r} (a float, three floats or 'pixel')")
    v, sigma = (0.0, 1.0) if pixel else (value, 0.0)
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    erase = []
    for _ in range(n):
        u = torch.rand(1 + 40 * int(count), generator=generator, dtype=torch.float64).tolist()
        rects = []
        for t in range(int(count)):
            for a in range(10):
                ua, ur, uy, ux = u[1 + 40 * t + 4 * a: 5 + 40 * t + 4 * a]
                area = H * W * (scale[0] + (scale[1] - scale[0]) * ua)
                aspect = math.exp(lr0 + (lr1 - lr0) * ur)
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if not (0 < h < H and 0 < w < W):
                    continue
                y, x = min(int(uy * (H - h + 1)), H - h), min(int(ux * (W - w + 1)), W - w)
                rects.append((x, y, w, h, v, sigma))
                break
        erase.append(rects if u[0] < p and rects else None)
    seeds = None
    if pixel:
        seeds = torch.randint(0, 2 ** 63 - 1, (n,), generator=generator, dtype=torch.int64).tolist()
    return erase, seeds


def mixup_cutmix(n: int, size, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0,
                 switch_prob: float = 0.5, pairing: str = "roll", per_frame: bool = False, generator=None):
    """n draws of MixUp / CutMix as timm's Mixup(mixup_alpha, cutmix_alpha, prob, switch_prob) makes them for
    frames stored at size = (H, W): (mix, label_lam) for mix= of the *_model calls.  One decision for the
    whole call, or per_frame=True one per frame (timm's mode="elem"): with probability prob the frame mixes;
    CutMix with probability switch_prob when both alphas are positive (else whichever alpha is positive);
    lam ~ Beta(a, a) as G1 / (G1 + G2) from torch._standard_gamma (float64).  pairing="roll": frame j's
    partner is frame j - 1 mod n (batch.roll(1, 0), torchvision v2's); "flip": frame n - 1 - j (timm's).
    MixUp: the entry is (partner, lam) and label_lam[j] = lam as float32.  CutMix, torchvision v2's box:
    centre (cx, cy) uniform over the integers [0, W) x [0, H), half sides int(0.5 sqrt(1 - lam) W) and
    int(0.5 sqrt(1 - lam) H), clamped to the frame; the entry is (partner, (x, y, w, h)) and
    label_lam[j] = 1 - w h / (H W); an empty box gives None (no mix) and label_lam 1, as does a frame that
    does not mix.  The caller's target is label_lam[j] y_j + (1 - label_lam[j]) y_partner.  Every decision
    consumes a fixed number of draws.  generator: a torch.Generator (CPU); the same seed gives the same
    lists."""
    import math
    import numpy as np
    import torch
    H, W = int(size[0]), int(size[1])
    if pairing not in ("roll", "flip"):
        raise ValueError(f"mixup_cutmix: pairing {pairing!r} ('roll' or 'flip')")
    if mixup_alpha < 0 or cutmix_alpha < 0 or not (0.0 <= prob <= 1.0) or not (0.0 <= switch_prob <= 1.0):
        raise ValueError(f"mixup_cutmix: alphas {mixup_alpha}, {cutmix_alpha}, prob {prob}, switch_prob {switch_prob}")
    draws = n if per_frame else 1
    u = torch.rand(draws, 4, generator=generator, dtype=torch.float64).tolist()
    alphas = torch.tensor([max(mixup_alpha, 1e-30), max(mixup_alpha, 1e-30), max(cutmix_alpha, 1e-30),
                           max(cutmix_alpha, 1e-30)], dtype=torch.float64).repeat(draws, 1)
    g = torch._standard_gamma(alphas, generator=generator).tolist()
    decisions = []
    for k in range(draws):
        if not (u[k][0] < prob) or (mixup_alpha <= 0 and cutmix_alpha <= 0):
            decisions.append(None)
            continue
        cut = cutmix_alpha > 0 and (mixup_alpha <= 0 or u[k][1] < switch_prob)
        g1, g2 = (g[k][2], g[k][3]) if cut else (g[k][0], g[k][1])
        lam = g1 / (g1 + g2) if g1 + g2 > 0 else 0.5
        if not cut:
            lam = float(np.float32(lam))
            decisions.append((lam, lam))
            continue
        cx, cy = min(int(u[k][2] * W), W - 1), min(int(u[k][3] * H), H - 1)
        r = 0.5 * math.sqrt(1.0 - lam)
        hw, hh = int(r * W), int(r * H)
        x1, y1, x2, y2 = max(cx - hw, 0), max(cy - hh, 0), min(cx + hw, W), min(cy + hh, H)
        if x2 <= x1 or y2 <= y1:
            decisions.append(None)
            continue
        decisions.append(((x1, y1, x2 - x1, y2 - y1), 1.0 - (x2 - x1) * (y2 - y1) / float(H * W)))
    mix, label_lam = [], []
    for j in range(n):
        d = decisions[j if per_frame else 0]
        if d is None:
            mix.append(None)
            label_lam.append(1.0)
            continue
        mix.append(((j - 1) % n if pairing == "roll" else n - 1 - j, d[0]))
        label_lam.append(d[1])
    return mix, label_lam


BLEND_MAX_TERMS = 8  # CCMI_BLEND_MAX_TERMS


class Blend(C.Structure):
    """ccmi_blend: per-frame term counts, the flat sources and weights, and the per-frame silent flags."""
    _fields_ = [("count", C.c_void_p), ("source", C.c_void_p), ("weight", C.c_void_p), ("silent", C.c_void_p)]


def _blend(blend, silent, n):
    """blend= / silent= of a *_model call -> (ccmi_blend, what it points to, the silent flags as a list of
    bool), or (None, None, None) with both None.  blend: one entry per frame, None or a list of at most 8
    (source, weight), source a frame of this call; silent: one flag per frame, True: the frame is rendered
    as a source only and has no output.  The library checks the values; the shapes are checked here."""
    import numpy as np
    if blend is None and silent is None:
        return None, None, None
    counts = np.zeros(n, dtype=np.int32)
    src, wgt = [], []
    if blend is not None:
        entries = list(blend)
        if len(entries) != n:
            raise ValueError(f"model output: blend takes one entry per frame ({n}), got {len(entries)}")
        for j, e in enumerate(entries):
            e = [] if e is None else list(e)
            if len(e) > BLEND_MAX_TERMS:
                raise ValueError(f"model output: frame {j}: {len(e)} blend terms (at most {BLEND_MAX_TERMS})")
            counts[j] = len(e)
            for t in e:
                if len(t) != 2:
                    raise ValueError("model output: a blend term is (source, weight)")
                src.append(int(t[0]))
                wgt.append(t[1])
    flags = np.zeros(n, dtype=np.int32)
    if silent is not None:
        quiet = [bool(v) for v in silent]
        if len(quiet) != n:
            raise ValueError(f"model output: silent takes one flag per frame ({n}), got {len(quiet)}")
        flags[:] = quiet
    source = np.array(src + [0], dtype=np.int32)
    weight = np.array(wgt + [0.0], dtype=np.float32)
    bl = Blend(count=counts.ctypes.data, source=source.ctypes.data, weight=weight.ctypes.data, silent=flags.ctypes.data)
    return bl, (counts, source, weight, flags), [bool(v) for v in flags]


def last_tail_groups() -> tuple:
    """(batched tail groups, per-frame tails) this thread's last decode or render call launched
    (ccmi_decode_last_tail_groups): frames that share a group share one launch per tail stage."""
    batched, per_frame = C.c_int(0), C.c_int(0)
    check(_bind().ccmi_decode_last_tail_groups(C.byref(batched), C.byref(per_frame)))
    return batched.value, per_frame.value


def _model_fmt(n, colour, mean, std, dtype, mirror):
    """(ccmi_tensor_fmt without strides, what it points to) of a *_model call."""
    import torch
    elems = {torch.float32: ELEM_F32, torch.float16: ELEM_F16, torch.bfloat16: ELEM_BF16}
    colours = {"rgb": COLOUR_RGB, "asis": COLOUR_ASIS}
    if dtype not in elems:
        raise ValueError(f"model output: dtype {dtype} (torch.float32, torch.float16 or torch.bfloat16)")
    if colour not in colours:
        raise ValueError(f"model output: colour {colour!r} ('rgb' or 'asis')")

    def three(v, default):
        if v is None:
            return [default] * 3
        v = [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * 3
        if len(v) != 3:
            raise ValueError("model output: mean / std take one value per channel")
        return v
    mean, std = three(mean, 0.0), three(std, 1.0)
    fmt = TensorFmt(elem=elems[dtype], colour=colours[colour])
    for c in range(3):
        fmt.scale[c] = 1.0 / std[c]       # Python floats, rounded to float32 by the assignment
        fmt.bias[c] = -mean[c] / std[c]
    flags = None
    if mirror is not None:
        m = [bool(mirror)] * n if isinstance(mirror, (bool, int)) else [bool(v) for v in mirror]
        if len(m) != n:
            raise ValueError(f"model output: mirror takes one flag per frame ({n}), got {len(m)}")
        flags = (C.c_uint8 * n)(*[int(v) for v in m])
        fmt.mirror = C.cast(flags, C.c_void_p)
    return fmt, flags


def _model_outs(geom, fmt, dtype, channels_last, out, dev, silent=None):
    """Destination tensors of a *_model call: fills fmt's strides; returns (result, pointers,
    capacities in bytes, what they point into).  silent: the call's silent flags or None; the result and
    out= then hold the other frames only, in call order, and a silent frame's pointer is NULL."""
    import torch
    emit = [i for i in range(len(geom)) if not (silent and silent[i])]
    if not emit:
        raise ValueError("model output: every frame is silent")
    m, n, g0 = len(geom), len(emit), geom[0]
    h, w = g0.height, g0.width
    if any((g.width, g.height) != (w, h) for g in geom):
        raise ValueError("model output: every region must have one size, since the frames form one [n, 3, h, w] "
                         "tensor; size=(out_h, out_w) resamples regions of different sizes to one")
    if out is None:
        if channels_last:
            res = torch.empty(n, h, w, 3, dtype=dtype, device=dev).permute(0, 3, 1, 2)
        else:
            res = torch.empty(n, 3, h, w, dtype=dtype, device=dev)
        frames = [res[i] for i in range(n)]
    else:
        frames = res = list(out)
        if len(frames) != n:
            raise ValueError(f"model output: out takes one tensor per frame ({n}), got {len(frames)}")
        for t in frames:
            if tuple(t.shape) != (3, h, w) or t.dtype != dtype or not t.is_cuda:
                raise ValueError(f"model output: out tensors must be CUDA {dtype} of shape [3, {h}, {w}], got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
    strides = tuple(int(s) for s in frames[0].stride())
    if any(tuple(int(s) for s in t.stride()) != strides for t in frames):
        raise ValueError("model output: out tensors must share one stride set")
    if strides == (0, 0, 0):  # would read as "planar contiguous" in ccmi_tensor_fmt
        raise ValueError("model output: out tensors with all-zero strides alias")
    fmt.stride_c, fmt.stride_y, fmt.stride_x = strides
    op, cap = (C.c_void_p * m)(), (C.c_size_t * m)()
    for i, t in zip(emit, frames):  # what the tensor's storage holds from its first element on
        st = t.untyped_storage()
        op[i] = t.data_ptr()
        cap[i] = max(st.nbytes() - (t.data_ptr() - st.data_ptr()), 0)
    return res, op, cap, frames


class _Sink:
    """What a formatted call of n frames takes after the format: the ccmi_rect array (None: whole frames,
    and always None with a warp), the ccmi_resample (None without size, or with a warp), the ccmi_warp,
    ccmi_colour, ccmi_tone, ccmi_filter, ccmi_mix and ccmi_blend (each None when absent), keep, what they
    point to, and silent, the blend's silent flags as a list of bool (None: every frame has an output)."""

    def __init__(self, n, rects=None, rs=None, warp=None, col=None, tone=None, flt=None, mx=None, keep=None, bl=None,
                 silent=None):
        self.n, self.rects, self.keep, self.silent = n, rects, keep, silent
        self.rs, self.warp, self.col, self.tone, self.flt, self.mx, self.bl = rs, warp, col, tone, flt, mx, bl
        ref = C.byref  # the seven stage arguments of the *_blend pair, in their order
        self._stages = (None if rs is None else ref(rs), None if warp is None else ref(warp),
                        None if col is None else ref(col), None if tone is None else ref(tone),
                        None if flt is None else ref(flt), None if bl is None else ref(bl),
                        None if mx is None else ref(mx))

    def plan_args(self, output_bitdepth, output_chroma_format, fmt):
        """n .. mix of the *_blend_plan prototypes: what lies between the source's head and geom."""
        return (self.n, self.rects, output_bitdepth, output_chroma_format, C.byref(fmt)) + self._stages

    def run_args(self, op, cap, fmt):
        """n .. mix of the *_blend prototypes: what lies between the source's head and out_bitdepth."""
        return (self.n, self.rects, op, cap, C.byref(fmt)) + self._stages


def _sink(n, rects=None, roi=None, size=None, affine=None, perspective=None, pad="fill", fill=0.0,
          interpolation="bilinear", clamp=False, colour_ops=None, blur=None, solarize=None, tone_ops=None, erase=None,
          erase_seed=None, mix=None, blend=None, silent=None):
    """The _Sink of the keywords of a *_model call of n frames.  rects: the regions' ccmi_rect array, None, or
    a callable that makes either (called after the stages are marshalled, and not with a warp)."""
    interp = _interp(interpolation, clamp)
    warp, keep_w = _warp(affine, n, size, roi, pad, fill, interp, perspective)
    col, keep_c = _colour(colour_ops, n)
    flt, keep_f = _filter(blur, solarize, n)
    tone, keep_t = _tone(tone_ops, n)
    mx, keep_m = _mix(erase, erase_seed, mix, n)
    bl, keep_b, quiet = _blend(blend, silent, n)
    if warp is not None:
        rects = None
    elif callable(rects):
        rects = rects()
    rs = None if size is None or warp is not None else _resample(size, interp)
    return _Sink(n, rects, rs, warp, col, tone, flt, mx, (keep_w, keep_c, keep_f, keep_t, keep_m, keep_b), bl, quiet)


def _stream_source(sp, ln):
    """A source is (plan entry point, run entry point, their first two arguments, the device or None for
    the current one): here of marshalled streams, LatentStore._source() of a store.  Both name the *_blend
    pair, the superset of every formatted call: a stage that is NULL leaves, by ccmi.h, the narrower
    call itself (down to *_fmt), so the absent keywords cost a NULL each and no other entry point."""
    L = _bind()
    return L.ccmi_decode_batch_dev_blend_plan, L.ccmi_decode_batch_dev_blend, (sp, ln), None


def _plain_fmt():
    """The format the header-only calls plan with: the element type, colour and strides do not change a plan."""
    fmt = TensorFmt(elem=ELEM_F32, colour=COLOUR_ASIS)
    for c in range(3):
        fmt.scale[c] = 1.0
    return fmt


def _plan_model(source, sink, fmt, output_bitdepth, output_chroma_format, info=None, window=None):
    """(ccmi_frame_geom array, workspace bytes) of a formatted call.  info / window: the plan's optional
    per-frame outputs; the library takes a window only with a warp."""
    plan, _, head, _ = source
    geom, need = (FrameGeom * sink.n)(), C.c_size_t(0)
    probe = TensorFmt.from_buffer_copy(fmt)  # planar strides: the geometry does not depend on them
    check(plan(*head, *sink.plan_args(output_bitdepth, output_chroma_format, probe), geom, info, window, C.byref(need)))
    return geom, need.value


def _run_model(source, sink, colour, mean, std, dtype, channels_last, mirror, out, output_bitdepth, output_chroma_format,
               workspace, stream_handle):
    """The body of decode_batch_model and LatentStore.render_model: one plan and one run of the source's
    *_blend pair."""
    import torch
    _, run, head, dev = source
    dtype = torch.float32 if dtype is None else dtype
    fmt, keep = _model_fmt(sink.n, colour, mean, std, dtype, mirror)
    geom, need = _plan_model(source, sink, fmt, output_bitdepth, output_chroma_format)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    res, op, cap, frames = _model_outs(geom, fmt, dtype, channels_last, out, dev, sink.silent)
    stream_handle, workspace = _stream_ws(dev, stream_handle, workspace, need)
    check(run(*head, *sink.run_args(op, cap, fmt), output_bitdepth, output_chroma_format, workspace.data_ptr(),
              workspace.numel(), stream_handle))
    del keep, frames
    return res


def decode_batch_model(streams: Sequence[bytes], roi=None, colour: str = "rgb", mean=None, std=None, dtype=None,
                       channels_last: bool = False, mirror=None, out=None, output_bitdepth: int = 0,
                       output_chroma_format: int = 0, workspace=None, stream_handle: int | None = None, size=None,
                       affine=None, pad: str = "fill", fill=0.0, colour_ops=None, blur=None, solarize=None,
                       tone_ops=None, erase=None, erase_seed=None, mix=None, blend=None, silent=None,
                       interpolation: str = "bilinear", clamp: bool = False, perspective=None):
    """Decode .cool streams into the tensor a model takes (ccmi_decode_batch_dev_fmt): one
    [n, 3, h, w] tensor of `dtype` (torch.float32, the default, torch.float16 or torch.bfloat16),
    every channel at full size (420 chroma nearest-upsampled), RGB (colour="rgb": YUV streams go
    through io.yuv2rgb's matrix and are clamped to [0, 1]; "asis" keeps the stream's planes), then
    (v - mean) / std per channel as v * float32(1 / std) + float32(-mean / std), written by the
    decoder's output kernel itself: no float32 frame set and no further pass.  The contract, step
    by step, is ccmi.h's (ccmi_tensor_fmt).

    Whatever the keywords, the call made is ccmi_decode_batch_dev_blend (and its _plan) with every absent
    stage NULL, which the library defines to be the narrower call: the entry point a paragraph below
    names is the one whose contract in ccmi.h the keyword follows, and the one the call then equals.

    roi as for decode_batch_tensors; every region must have one size, and 420 samples need even
    x, y, w and h (output_chroma_format=444 takes any).  channels_last=True: an [n, h, w, 3]
    allocation returned as its permuted [n, 3, h, w] view.  mirror: one flag per frame (or one
    bool): that frame is flipped left to right.  out: a list of n CUDA tensors or views of shape
    [3, h, w] and one stride set (a tile of a larger canvas, NHWC slices, ...), filled in place
    and returned instead of a new tensor.

    size=(out_h, out_w) (ccmi_decode_batch_dev_rs): every region, of any size, is resampled to
    that size by the antialiased triangle filter of interpolate(mode="bilinear", antialias=True)
    between the colour step and the normalisation, in the same output stage (the contract's
    steps 3a-3c); h, w above are then out_h, out_w, the regions may differ in size, and frames
    of one architecture share their launches whatever their regions (last_tail_groups()).

    affine= (ccmi_decode_batch_dev_warp; needs size, excludes roi): [n, 2, 3], or one [2, 3] for
    every frame, as an array, a nested list or a CPU tensor (affine_matrix() makes one).  Every
    output pixel (i, k) is a bilinear sample of the whole frame at xs = m00 (k + 0.5) +
    m01 (i + 0.5) + m02, ys = m10 (k + 0.5) + m11 (i + 0.5) + m12 (pixels; grid_sample with
    align_corners=False, not antialiased), between the colour step and the normalisation: rotation,
    scale, shear and translation in the same output stage.  pad="fill": a tap outside the frame is
    `fill` (one value or one per channel, in [0, 1] colour units, before the normalisation);
    pad="edge": the nearest frame pixel.  The library decodes only the window of each frame its
    matrix reaches.

    colour_ops= (ccmi_decode_batch_dev_col; with or without roi, size and affine): one list of
    (op, value) tuples for every frame, or one list per frame, of at most 8 ops each, applied in
    the list's order to the three channels of every output pixel after the geometry and before the
    normalisation (the contract's step 3z): ('brightness', f), ('saturation', f), ('contrast', f)
    with f >= 0 (at most one contrast op per frame: it blends with the frame's mean grey, which a
    statistics pass of the output stage sums in fixed point), ('matrix', M) with M a [3, 4] matrix
    (hue_matrix(), grey_matrix()).  Every op clamps to [0, 1].  colour_jitter() draws such lists.
    Frames with different ops, or none, share the tail's launches.  None or []: the call without.

    blur= / solarize= (ccmi_decode_batch_dev_flt; with or without everything above): after the colour
    ops and before the normalisation (the contract's steps 3y-0 .. 3y-2), on the frame as it is stored
    (after mirror).  blur: one entry for every frame or one per frame, an entry None or a 1-D float32
    array of half taps w_0 (centre) .. w_r, r <= 15 (gaussian_taps() makes one, gaussian_blur() draws
    them): a separable blur with reflecting borders, clamped to [0, 1].  solarize: None, one threshold
    for every frame or one per frame (None or above 1: off): v >= threshold becomes 1 - v.  The frames
    that take neither go through the kernels of the call without; the others are staged in float32 in
    the workspace and share one launch of the filter kernel per tail group.

    tone_ops= (ccmi_decode_batch_dev_tone; with or without everything above): one list of (op, value)
    tuples for every frame, or one per frame, of at most 8 ops each, applied in the list's order to the
    staged frame after the colour ops and before blur / solarize (the contract's step 3x), each over the
    whole frame before the next: ('brightness', f), ('saturation', f), ('contrast', f), ('matrix', M),
    ('solarize', th), ('posterize', bits 1..8), ('autocontrast', None), ('equalize', None),
    ('sharpness', f).  rand_augment() and trivial_augment_wide() draw such lists (and the matrices for
    affine=).  A frame with a list is staged like a blurred one; the others keep their kernels and bits.

    interpolation="bicubic" (CCMI_FILTER_CUBIC / CCMI_WARP_CUBIC; one value per call, "bilinear" is the
    default and the call as it always was): size= resamples with the antialiased Keys cubic of
    interpolate(mode="bicubic", antialias=True) and of PIL's BICUBIC, affine= samples 16 taps as
    grid_sample(mode="bicubic") does.  A bicubic result may leave [0, 1], as torch's; clamp=True
    (bicubic only) clamps it to [0, 1] before the colour ops and the normalisation, which is what a
    uint8 pipeline gives.  Any other string, and clamp=True with "bilinear", is a ValueError.
    perspective= (CCMI_WARP_PROJECTIVE; needs size, excludes affine and roi): [n, 3, 3], or one [3, 3]
    for every frame: the homography that maps an output position to the frame position, xs = xn / wn,
    ys = yn / wn (torchvision's F.perspective convention; perspective_matrix() makes one,
    random_perspective() draws them).  It composes with pad, fill, interpolation, clamp, mirror,
    colour_ops, tone_ops, blur and solarize exactly as affine= does; rows 0 0 1 give affine='s bits.
    The library refuses a denominator that is not positive over the output and a perspective too
    strong for float32 positions (ccmi.h).

    erase= / erase_seed= / mix= (ccmi_decode_batch_dev_mix; with or without everything above): RandomErasing,
    MixUp and CutMix AFTER the normalisation and before the one rounding to `dtype` (the contract's steps
    4e and 4m), in stored coordinates (after mirror).  erase: one entry per frame, None or a list of at
    most 4 rectangles (x, y, w, h, value[, sigma]), value one float or three in the normalised units, a
    later rectangle winning; sigma > 0 adds a Gaussian of that sigma per element from the counter-based
    generator of ccmi.h, keyed by erase_seed (one int, or one per frame) and the element's stored position
    alone: a frame gives the same bits alone or anywhere in any batch.  mix: one entry per frame, None,
    (partner, lam): lam * frame + (1 - lam) * partner, or (partner, (x, y, w, h)): the partner's pixels
    inside the box; the partner enters erased but unmixed (batch.roll() / flip() of the erased batch) and
    must be stored at the frame's size.  random_erasing() and mixup_cutmix() draw such lists.  The frames
    concerned are staged in float32 like blurred ones and formatted by one launch per call; the others
    keep their kernels and bits.

    blend= / silent= (ccmi_decode_batch_dev_blend; with or without everything above): weighted sums of
    staged frames of this call BEFORE the normalisation (the contract's step 3b).  blend: one entry per
    frame, None or a list of at most 8 (source, weight): the frame becomes w_0 * source_0 + w_1 * source_1
    + ..., each source as staged (after its own geometry, colour, tone ops and filter; its own blend list
    does not enter), at the frame's stored size; erase and mix then apply to the sum, and a partner enters
    with its own sum.  silent: one flag per frame, True: the frame is rendered as a source only; the
    returned tensor, and out=, then hold the other frames only, in call order.  aug_mix() draws such
    lists.  With streams every repeat of a stream is decoded again: build a LatentStore for AugMix."""
    n = len(streams)
    keep, sp, ln = _marshal(streams)
    sink = _sink(n, lambda: _rects(roi, streams, n), roi, size, affine, perspective, pad, fill, interpolation, clamp,
                 colour_ops, blur, solarize, tone_ops, erase, erase_seed, mix, blend, silent)
    return _run_model(_stream_source(sp, ln), sink, colour, mean, std, dtype, channels_last, mirror, out, output_bitdepth,
                      output_chroma_format, workspace, stream_handle)


def weights_i32(stream: bytes):
    """(arm, ups, syn) fixed-point network integers of a stream's intra frame, as the
    decoder uses them (ccmi_decode_weights_i32; cc-frame-decoder.cpp:201-353)."""
    import numpy as np
    L = _bind()
    buf = C.create_string_buffer(stream, len(stream))
    cnt = (C.c_size_t * 3)()
    check(L.ccmi_decode_weights_i32(C.cast(buf, C.c_void_p), len(stream), None, 0, None, 0, None, 0, cnt))
    arr = [np.zeros(max(int(c), 1), dtype=np.int32) for c in cnt]
    check(L.ccmi_decode_weights_i32(C.cast(buf, C.c_void_p), len(stream), arr[0].ctypes.data, arr[0].size,
                                    arr[1].ctypes.data, arr[1].size, arr[2].ctypes.data, arr[2].size, cnt))
    return tuple(a[: int(c)] for a, c in zip(arr, cnt))


def ups_forward_i32(latent, sizes, kernels, ups_k: int, n_ups: int, pre_k: int, n_pre: int):
    """Integer upsampling on the GPU (ccmi_ups_forward_i32): latent int32 [N] (value << 8,
    grids flat in order), kernels int32 (weights_i32()[1]) -> int32 [L, H, W]."""
    import torch
    from . import require_cuda
    require_cuda(latent, kernels)
    L = _bind()
    n = len(sizes)
    h = (C.c_int * MAX_GRIDS)(*[s[0] for s in sizes])
    w = (C.c_int * MAX_GRIDS)(*[s[1] for s in sizes])
    if latent.dtype != torch.int32 or latent.numel() < sum(a * b for a, b in sizes):
        raise ValueError("latent: int32 with sum(h * w) elements expected")
    if kernels.dtype != torch.int32:
        raise ValueError("kernels: int32 expected (weights_i32()[1])")
    latent, kernels = latent.contiguous(), kernels.contiguous()  # held until after the launch
    out = torch.empty(n, sizes[0][0], sizes[0][1], dtype=torch.int32, device=latent.device)
    nws = L.ccmi_ups_workspace_bytes_i32(n, h, w)
    ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=latent.device)
    a = UpsI32Args(latent=latent.data_ptr(), n_grids=n, h=h, w=w, kernels=kernels.data_ptr(), ups_k=ups_k,
                   n_ups=n_ups, pre_k=pre_k, n_pre=n_pre, out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nws)
    check(L.ccmi_ups_forward_i32(C.byref(a), torch.cuda.current_stream(latent.device).cuda_stream))
    return out


def syn_forward_i32(x, layers, params):
    """Integer synthesis of one branch on the GPU (ccmi_syn_forward_i32): x int32 [C, H, W]
    at precision 12, layers [(n_out, ks, residual, relu)], params int32 -> int32 [n_out, H, W]."""
    import torch
    from . import require_cuda
    require_cuda(x, params)
    L = _bind()
    c, hh, ww = x.shape
    arr = (SynLayer * MAX_SYN_LAYERS)()
    for i, (n_out, ks, res, relu) in enumerate(layers):
        arr[i] = SynLayer(int(n_out), int(ks), int(res), int(relu))
    if x.dtype != torch.int32 or params.dtype != torch.int32:
        raise ValueError("syn_forward_i32: int32 input and params expected")
    x, params = x.contiguous(), params.contiguous()  # held until after the launch
    out = torch.empty(layers[-1][0], hh, ww, dtype=torch.int32, device=x.device)
    a = SynI32Args(in_=x.data_ptr(), c_in=c, h=hh, w=ww, n_layers=len(layers), layers=arr,
                   params=params.data_ptr(), out=out.data_ptr(), workspace=None, workspace_bytes=0)
    nws = L.ccmi_syn_workspace_bytes_i32(C.byref(a))
    ws = None
    if nws:
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nws
    check(L.ccmi_syn_forward_i32(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream))
    return out


def decode_latents(stream: bytes, stream_handle: int | None = None) -> list:
    """Integer latents of an intra .cool stream, decoded on the GPU (one np.int32 array
    per grid, row-major)."""
    import numpy as np
    from . import encode
    fr = encode.parse(stream)
    n = sum(h * w for h, w in fr.grid_sizes)
    out = np.zeros(n, dtype=np.int32)
    buf = C.create_string_buffer(stream, len(stream))
    L = _bind()
    if stream_handle is None:
        import torch
        stream_handle = torch.cuda.current_stream().cuda_stream
    check(L.ccmi_decode_latents(C.cast(buf, C.c_void_p), len(stream), out.ctypes.data, n, stream_handle))
    res, p = [], 0
    for h, w in fr.grid_sizes:
        res.append(out[p: p + h * w].copy())
        p += h * w
    return res


def last_timing() -> dict:
    """Device stage times (ms) of this thread's last decode: upload, arm_cabac, ups_syn_out, download."""
    ms = (C.c_float * 4)()
    check(lib().ccmi_decode_last_timing(ms))
    return dict(zip(("upload", "arm_cabac", "ups_syn_out", "download"), list(ms)))


# CCMI_ARM_FLAG_* (include/ccmi.h): what the latent decode of a stream did
ARM_FLAG_TIMEOUT, ARM_FLAG_Q32, ARM_FLAG_W32, ARM_FLAG_PRE32, ARM_FLAG_BIG = 1, 2, 4, 8, 16
ARM_FLAG_NARROW = 32  # LatentStore build: a latent does not fit the store's element type


def last_arm_flags() -> list[int]:
    """Per stream of this thread's last decode call: the OR of its latent grids'
    CCMI_ARM_FLAG_* bits (which multiply forms the ARM kernels ran; TIMEOUT = the call failed)."""
    L = lib()
    n = C.c_int(0)
    check(L.ccmi_decode_last_arm_flags(None, 0, C.byref(n)))
    out = (C.c_uint32 * max(n.value, 1))()
    check(L.ccmi_decode_last_arm_flags(out, n.value, C.byref(n)))
    return [int(v) for v in out[: n.value]]


LATENT_I8, LATENT_I16, LATENT_I32, LATENT_SEG = 0, 1, 2, 3  # CCMI_LATENT_*; SEG by LatentStore.compact() only


class LatentStore:
    """Decode once, render often (ccmi_latents_*): the ARM + CABAC decode of `streams` runs
    once, and its output -- the integer latents, packed, with the upsampling and synthesis
    integers -- stays in one device tensor owned by this object.  render() then produces any
    region of any of the streams, in any output format, at the cost of the decoder tail alone;
    its result is exactly what decode_batch_tensors returns for the same streams and arguments.

    dtype None: int16 latents, rebuilt as int32 if a stream reports ARM_FLAG_NARROW (a latent
    outside -32768..32767); torch.int8 / torch.int16 / torch.int32: exactly that type, and a
    latent that does not fit it is a CcmiError (ERR_UNSUPPORTED; last_arm_flags() shows which
    streams).  arm_flags: the build's CCMI_ARM_FLAG_* bits per stream.  workspace: a uint8 CUDA tensor for the build (else torch's allocator).  The
    Python bytes are not referred to after the constructor returns.

    compact() makes a store of the same streams with per-segment bit widths (dtype "seg", several
    times smaller), LatentStore.concat() one store object over the streams of several (a set built
    chunk by chunk, of any mix of types); both render exactly as the stores they were made from.
    nbytes, stream_nbytes and stream_dtypes: the store bytes, in all and per stream, and each
    stream's type."""

    def __init__(self, streams: Sequence[bytes], dtype=None, workspace=None, stream_handle: int | None = None):
        import torch
        self._h = None
        L = _bind()
        table = {torch.int8: LATENT_I8, torch.int16: LATENT_I16, torch.int32: LATENT_I32}
        if dtype is not None and dtype not in table:
            raise ValueError(f"LatentStore: dtype {dtype} (torch.int8, torch.int16, torch.int32 or None)")
        m = _marshal(streams)
        n = len(streams)
        dev = torch.device("cuda", torch.cuda.current_device())
        for t in ([torch.int16, torch.int32] if dtype is None else [dtype]):
            nstore, nws = C.c_size_t(0), C.c_size_t(0)
            check(L.ccmi_latents_plan(m[1], m[2], n, table[t], C.byref(nstore), None, C.byref(nws)))
            store = torch.empty(max(nstore.value, 256), dtype=torch.uint8, device=dev)
            stream_handle, ws = _stream_ws(dev, stream_handle, workspace, nws.value)
            h = C.c_void_p(None)
            rc = L.ccmi_latents_decode(m[1], m[2], n, table[t], store.data_ptr(), store.numel(), ws.data_ptr(),
                                       ws.numel(), stream_handle, C.byref(h))
            if rc == 0:
                break
            if not (dtype is None and t == torch.int16 and any(f & ARM_FLAG_NARROW for f in last_arm_flags())):
                check(rc)
        flags = last_arm_flags()  # of the build; the planning and render calls clear the thread's record
        self._adopt(h, [store], flags)

    def _adopt(self, h, stores, arm_flags):
        """Takes the handle h over the device tensors `stores`; the facts come from the handle."""
        import torch
        L = _bind()
        self._h, self._stores, self._store, self.arm_flags = h, list(stores), stores[0], arm_flags
        names = {LATENT_I8: torch.int8, LATENT_I16: torch.int16, LATENT_I32: torch.int32, LATENT_SEG: "seg"}
        self.stream_nbytes, self.stream_dtypes = [], []
        for i in range(len(self)):
            t, nb = C.c_int(0), C.c_size_t(0)
            check(L.ccmi_latents_stream_info(h, i, C.byref(t), C.byref(nb)))
            self.stream_nbytes.append(nb.value)
            self.stream_dtypes.append(names[t.value])
        self.nbytes = sum(self.stream_nbytes)
        self.dtype = self.stream_dtypes[0] if len(set(self.stream_dtypes)) == 1 else "mixed"
        geom, _ = self.render_geometry()
        self.geometry = [{k: g[k] for k in ("width", "height", "bitdepth", "chroma", "frame_data_type")} for g in geom]

    def compact(self, workspace=None, stream_handle: int | None = None) -> "LatentStore":
        """A new store of the same streams in the segmented form (ccmi_latents_compact: runs of 64
        latents at the narrowest of 0, 2, 4, 8, 16, 32 bits), measured, allocated exactly and
        packed on the GPU.  This store is untouched and may be closed; the new one renders the
        same samples.  workspace: a uint8 CUDA tensor (else torch's allocator)."""
        import torch
        L = _bind()
        dev = self._store.device
        bound, nws, exact = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(L.ccmi_latents_compact_plan(self._handle(), C.byref(bound), C.byref(nws)))
        stream_handle, ws = _stream_ws(dev, stream_handle, workspace, nws.value)
        check(L.ccmi_latents_compact_measure(self._handle(), ws.data_ptr(), ws.numel(), stream_handle, C.byref(exact), None))
        store = torch.empty(max(exact.value, 256), dtype=torch.uint8, device=dev)
        h = C.c_void_p(None)
        check(L.ccmi_latents_compact(self._handle(), store.data_ptr(), store.numel(), ws.data_ptr(), ws.numel(),
                                     stream_handle, C.byref(h)))
        out = LatentStore.__new__(LatentStore)
        out._adopt(h, [store], list(self.arm_flags))
        return out

    @classmethod
    def concat(cls, stores) -> "LatentStore":
        """One store object over the streams of `stores`, in order (ccmi_latents_concat): host
        only, nothing is copied.  The parts may be closed afterwards: the new object keeps their
        device tensors alive.  dtype is the parts' common type, or "mixed"."""
        stores = list(stores)
        if not stores:
            raise ValueError("LatentStore.concat: no stores")
        parts = (C.c_void_p * len(stores))(*[s._handle() for s in stores])
        h = C.c_void_p(None)
        check(_bind().ccmi_latents_concat(parts, len(stores), C.byref(h)))
        out = cls.__new__(cls)
        out._adopt(h, [t for s in stores for t in s._stores], [f for s in stores for f in s.arm_flags])
        return out

    def save(self, path, index=None, workspace=None, stream_handle: int | None = None) -> int:
        """Writes streams `index` of this store (None: all, in order; repeats and any order allowed)
        as a latent file (ccmi_latents_export; the file form is in include/ccmi.h): any store, a
        concat of mixed types included.  The file is a function of the streams alone, byte for
        byte.  arm_flags travel with the streams.  Written under a temporary name in the same
        directory, then renamed.  Returns the file's bytes."""
        import os
        import torch
        L = _bind()
        idx = None if index is None else [int(i) for i in index]
        m = len(self) if idx is None else len(idx)
        arr = None if idx is None else (C.c_int * max(m, 1))(*idx)
        nmeta, nfile, nws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(L.ccmi_latents_export_plan(self._handle(), arr, m, C.byref(nmeta), C.byref(nfile), C.byref(nws)))
        src = range(m) if idx is None else idx
        flags = (C.c_uint32 * m)(*[int(self.arm_flags[i]) if i < len(self.arm_flags) else 0 for i in src])
        host = torch.empty(nfile.value, dtype=torch.uint8, pin_memory=True)
        stream_handle, ws = _stream_ws(self._store.device, stream_handle, workspace, nws.value)
        check(L.ccmi_latents_export(self._handle(), arr, m, flags, host.data_ptr(), host.numel(), ws.data_ptr(),
                                    ws.numel(), stream_handle))
        path = os.fspath(path)
        tmp = "%s.tmp.%d" % (path, os.getpid())
        try:
            with open(tmp, "wb") as f:
                f.write(memoryview(host.numpy()))
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return nfile.value

    @staticmethod
    def _read_meta(f):
        """(stream count, META bytes, file bytes) of the open latent file f."""
        L = _bind()
        head = f.read(64)
        n, nmeta, nfile = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        check(L.ccmi_latents_file_head(head, len(head), C.byref(n), C.byref(nmeta), C.byref(nfile)))
        f.seek(0)
        return n.value, f.read(nmeta.value), nfile.value

    @classmethod
    def load(cls, path, first: int = 0, count=None, workspace=None, stream_handle: int | None = None) -> "LatentStore":
        """Streams [first, first + count) (count None: to the end) of a latent file as a store
        (ccmi_latents_import).  Only META and those streams' part of the file are read, so a rank's
        shard of a big file costs that shard's I/O.  The file is untrusted input: it is validated on
        the host, checksummed and its descriptor tables verified on the GPU before the store exists;
        a CcmiError (ERR_BITSTREAM) names the stream.  Loaded stores compact(), concat(), render and
        latents() like any other: LatentStore.concat([LatentStore.load(p) for p in chunks]) reopens a
        data set built chunk by chunk."""
        import torch
        L = _bind()
        with open(path, "rb") as f:
            n, meta, _ = cls._read_meta(f)
            cnt = -1 if count is None else int(count)
            off, nbytes, nws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
            check(L.ccmi_latents_import_plan(meta, len(meta), int(first), cnt, C.byref(off), C.byref(nbytes), None,
                                             C.byref(nws)))
            host = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, pin_memory=True)
            view = memoryview(host.numpy())[: nbytes.value]
            f.seek(off.value)
            got = 0
            while got < nbytes.value:
                k = f.readinto(view[got:])
                if not k:
                    raise CcmiError(ERR_IO, f"LatentStore.load: {path} ends {nbytes.value - got} bytes short of its DATA")
                got += k
        m = n - int(first) if count is None else int(count)
        dev = torch.device("cuda", torch.cuda.current_device())
        store = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=dev)
        stream_handle, ws = _stream_ws(dev, stream_handle, workspace, nws.value)
        flags, h = (C.c_uint32 * max(m, 1))(), C.c_void_p(None)
        check(L.ccmi_latents_import(meta, len(meta), int(first), cnt, host.data_ptr(), nbytes.value, store.data_ptr(),
                                    store.numel(), ws.data_ptr(), ws.numel(), stream_handle, flags, C.byref(h)))
        out = cls.__new__(cls)
        out._adopt(h, [store], [int(v) for v in flags[:m]])
        return out

    @staticmethod
    def file_info(path) -> dict:
        """What a latent file holds, from META alone (no GPU): {'n_streams', 'meta_bytes',
        'file_bytes', 'streams': [{'width', 'height', 'bitdepth', 'chroma', 'frame_data_type',
        'dtype', 'nbytes', 'arm_flags'}]}."""
        L = _bind()
        with open(path, "rb") as f:
            n, meta, nfile = LatentStore._read_meta(f)
        flags, h = (C.c_uint32 * n)(), C.c_void_p(None)
        check(L.ccmi_latents_import(meta, len(meta), 0, -1, None, 0, None, 0, None, 0, None, flags, C.byref(h)))
        st = LatentStore.__new__(LatentStore)
        st._adopt(h, [None], [int(v) for v in flags])  # plan-only: no store behind it
        try:
            streams = [dict(g, dtype=t, nbytes=nb, arm_flags=fl)
                       for g, t, nb, fl in zip(st.geometry, st.stream_dtypes, st.stream_nbytes, st.arm_flags)]
        finally:
            st.close()
        return {"n_streams": n, "meta_bytes": len(meta), "file_bytes": nfile, "streams": streams}

    def __len__(self):
        return _bind().ccmi_latents_count(self._handle())

    def _handle(self):
        if self._h is None:
            raise ValueError("LatentStore: closed")
        return self._h

    def close(self):
        """Frees the handle and drops the store tensor."""
        if getattr(self, "_h", None) is not None:
            _bind().ccmi_latents_free(self._h)
            self._h = None
            self._store = None
            self._stores = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _frames(self, index, roi):
        """(m, index array or None, rect array or None)"""
        n = len(self)
        idx = list(range(n)) if index is None else [int(i) for i in index]
        m = len(idx)
        if m < 1:
            raise ValueError("LatentStore: no frames")

        def whole(j):  # of that frame's stream (an index out of range is the library's error)
            g = self.geometry[idx[j]] if 0 <= idx[j] < n else {"width": 1, "height": 1}
            return 0, 0, g["width"], g["height"]
        rects = _roi_rects(roi, m, whole, "frame")
        return m, (None if index is None else (C.c_int * m)(*idx)), rects

    def _source(self, idx):
        """This store as the source of a formatted call (see _stream_source); idx: _frames()'s index array."""
        L = _bind()
        return (L.ccmi_latents_render_blend_plan, L.ccmi_latents_render_blend, (self._handle(), idx),
                getattr(self._store, "device", None))

    def _plan(self, index, roi, output_bitdepth, output_chroma_format, dtype, info=None):
        L = _bind()
        m, idx, rects = self._frames(index, roi)
        geom, need = (FrameGeom * m)(), C.c_size_t(0)

        def plan(sample):
            check(L.ccmi_latents_render_plan(self._handle(), idx, m, rects, output_bitdepth, output_chroma_format, sample,
                                             geom, info(m) if callable(info) else None, C.byref(need)))
        sample = _pick_sample(plan, geom, dtype, "LatentStore")
        return m, idx, rects, sample, geom, need.value

    def render_geometry(self, index=None, roi=None, output_bitdepth: int = 0, output_chroma_format: int = 0,
                        dtype=None) -> tuple:
        """Header-only, like decode_batch_geometry: ([geometry per output frame], render workspace bytes)."""
        _, _, _, _, geom, need = self._plan(index, roi, output_bitdepth, output_chroma_format, dtype)
        return [{k: int(getattr(g, k)) for k, _ in FrameGeom._fields_} for g in geom], need

    def roi_plan(self, index, roi, output_bitdepth: int = 0, output_chroma_format: int = 0, dtype=None) -> list:
        """Like decode.roi_plan, per output frame: arm_rows = the latent rows the tail's planes hold."""
        box = []

        def info(m):
            box.append((RoiInfo * m)())
            return box[-1]
        self._plan(index, roi, output_bitdepth, output_chroma_format, dtype, info)
        return [{"arm_rows": [int(v) for v in i.arm_rows[: i.n_grids]], "windowed": bool(i.windowed)} for i in box[-1]]

    def render(self, index=None, roi=None, output_bitdepth: int = 0, output_chroma_format: int = 0, dtype=None,
               stack: bool = False, workspace=None, stream_handle: int | None = None):
        """Frame j = stream index[j] of the store (None: every stream in order; repeats and any
        order allowed), region roi[j] (one (x, y, w, h) for every frame, a sequence with one
        entry per frame, None entries or None: whole frames).  Returns exactly what
        decode_batch_tensors returns for those streams: tensors, {'y', 'u', 'v'} dicts, or with
        stack=True one stacked tensor / dict.  workspace: a uint8 CUDA tensor of at least
        render_geometry(...)[1] bytes."""
        m, idx, rects, sample, geom, need = self._plan(index, roi, output_bitdepth, output_chroma_format, dtype)
        dev = self._store.device
        flat, outs, op, cap = _alloc_outs(geom, sample, stack, dev)
        stream_handle, workspace = _stream_ws(dev, stream_handle, workspace, need)
        check(_bind().ccmi_latents_render(self._handle(), idx, m, rects, op, cap, sample, output_bitdepth,
                                          output_chroma_format, workspace.data_ptr(), workspace.numel(), stream_handle))
        return _shape_outs(flat, outs, geom, stack)

    def render_model(self, index=None, roi=None, colour: str = "rgb", mean=None, std=None, dtype=None,
                     channels_last: bool = False, mirror=None, out=None, output_bitdepth: int = 0,
                     output_chroma_format: int = 0, workspace=None, stream_handle: int | None = None, size=None,
                     affine=None, pad: str = "fill", fill=0.0, colour_ops=None, blur=None, solarize=None,
                     tone_ops=None, erase=None, erase_seed=None, mix=None, blend=None, silent=None,
                     interpolation: str = "bilinear", clamp: bool = False, perspective=None):
        """render() into the tensor a model takes: frames and regions as for
        render(), the result and every other argument as for decode_batch_model, whose output for
        the same streams and arguments it equals bit for bit.  The call made is ccmi_latents_render_blend
        (and its _plan) with every absent stage NULL, which the library defines to be the narrower call:
        ccmi_latents_render_fmt; with size ccmi_latents_render_rs; with affine ccmi_latents_render_warp;
        with colour_ops ccmi_latents_render_col, with blur or solarize ccmi_latents_render_flt, with
        tone_ops ccmi_latents_render_tone.  workspace with a size or an affine:
        at least what render_model_workspace_bytes() reports (the resample's intermediate and a
        warp's windows are not part of render_geometry()'s figure);
        render_model_workspace_bytes() takes the same arguments.  interpolation= / clamp= as for
        decode_batch_model (a bicubic warp's windows, and so its workspace, are a tap wider);
        perspective= as for decode_batch_model, in place of affine=; erase= / erase_seed= / mix= as for
        decode_batch_model (ccmi_latents_render_mix), partners being frames of this call; blend= / silent= as
        for decode_batch_model (ccmi_latents_render_blend), sources being frames of this call: see aug_mix()."""
        m, idx, rects = self._frames(index, None if affine is not None or perspective is not None else roi)
        sink = _sink(m, rects, roi, size, affine, perspective, pad, fill, interpolation, clamp, colour_ops, blur, solarize,
                     tone_ops, erase, erase_seed, mix, blend, silent)
        return _run_model(self._source(idx), sink, colour, mean, std, dtype, channels_last, mirror, out, output_bitdepth,
                          output_chroma_format, workspace, stream_handle)

    def warp_plan(self, index, affine, size, pad: str = "fill", fill=0.0, output_bitdepth: int = 0,
                  output_chroma_format: int = 0, interpolation: str = "bilinear", clamp: bool = False,
                  perspective=None) -> list:
        """What render_model(affine=...) will do, per output frame (header-only: ccmi_latents_render_blend_plan
        with a warp alone, by ccmi.h the ccmi_latents_render_warp_plan call), like roi_plan: {'window':
        (x, y, w, h), the rectangle of the frame the tail renders for that frame's matrix, 'windowed',
        'arm_rows'}.  interpolation="bicubic": the window
        of the 16 taps, one pixel wider on every side the frame allows.  perspective= (with affine=None):
        the plan of render_model(perspective=...)."""
        m, idx, _ = self._frames(index, None)
        if affine is None and perspective is None:
            raise ValueError("LatentStore.warp_plan: affine is None")
        sink = _sink(m, size=size, affine=affine, perspective=perspective, pad=pad, fill=fill, interpolation=interpolation,
                     clamp=clamp)
        info, window = (RoiInfo * m)(), (Rect * m)()
        _plan_model(self._source(idx), sink, _plain_fmt(), output_bitdepth, output_chroma_format, info, window)
        return [{"window": (r.x, r.y, r.w, r.h), "windowed": bool(i.windowed),
                 "arm_rows": [int(v) for v in i.arm_rows[: i.n_grids]]} for i, r in zip(info, window)]

    def render_model_workspace_bytes(self, index=None, roi=None, size=None, output_bitdepth: int = 0,
                                     output_chroma_format: int = 0, affine=None, pad: str = "fill", fill=0.0,
                                     colour_ops=None, blur=None, solarize=None, tone_ops=None, erase=None,
                                     erase_seed=None, mix=None, blend=None, silent=None,
                                     interpolation: str = "bilinear", clamp: bool = False, perspective=None) -> int:
        """Header-only: the workspace render_model needs, from render_model's own plan call
        (ccmi_latents_render_blend_plan with the absent stages NULL: by ccmi.h the narrower plan named with
        each figure here), for these frames, regions and size, or
        these frames, matrices and size (ccmi_latents_render_rs_plan / _warp_plan; the element type,
        colour and strides do not change it), these colour ops (ccmi_latents_render_col_plan:
        the op tables and the contrast ops' accumulators) and this blur and solarize
        (ccmi_latents_render_flt_plan: a float32 staging frame and 256 bytes of tables per frame
        that takes the stage) and these tone ops (ccmi_latents_render_tone_plan: ccmi.h's formula).
        perspective= in place of affine=: the same plans with CCMI_WARP_PROJECTIVE.  erase= / mix=
        (ccmi_latents_render_mix_plan): 256 bytes per mix-staged frame and a second float32 frame for
        those with a blur or a solarize, on top of their staging (ccmi.h's formula).  blend= / silent=
        (ccmi_latents_render_blend_plan): the blend-staged frames counted as mix-staged, and 64 bytes for
        each mix-staged frame, rounded up to 256 as a whole."""
        m, idx, rects = self._frames(index, None if affine is not None or perspective is not None else roi)
        sink = _sink(m, rects, roi, size, affine, perspective, pad, fill, interpolation, clamp, colour_ops, blur, solarize,
                     tone_ops, erase, erase_seed, mix, blend, silent)
        return _plan_model(self._source(idx), sink, _plain_fmt(), output_bitdepth, output_chroma_format)[1]

    def latents(self, i: int) -> list:
        """Stream i's integer latents: one int32 device tensor [h_l, w_l] per grid."""
        import torch
        g = self.geometry[i]
        sizes, h, w = [], g["height"], g["width"]
        n_grids = len(self.roi_plan([i], None)[0]["arm_rows"])
        for _ in range(n_grids):
            sizes.append((h, w))
            h, w = (h + 1) // 2, (w + 1) // 2
        flat = torch.empty(sum(a * b for a, b in sizes), dtype=torch.int32, device=self._store.device)
        check(_bind().ccmi_latents_values(self._handle(), int(i), flat.data_ptr(), flat.numel(),
                                          torch.cuda.current_stream(flat.device).cuda_stream))
        out, p = [], 0
        for a, b in sizes:
            out.append(flat[p: p + a * b].view(a, b))
            p += a * b
        return out


__all__ = ["last_timing", "LatentStore", "last_arm_flags", "decode_latents", "decode_file", "decode_batch", "decode_batch_workspace_bytes", "output_size",
           "decode_batch_tensors", "decode_batch_geometry", "roi_plan", "decode_batch_model", "last_tail_groups",
           "affine_matrix", "perspective_matrix", "random_perspective", "hue_matrix", "grey_matrix", "colour_jitter",
           "gaussian_taps", "gaussian_blur", "random_solarize", "rand_augment", "trivial_augment_wide",
           "aug_mix", "auto_augment",
           "weights_i32", "ups_forward_i32", "syn_forward_i32", "CcmiError"]
