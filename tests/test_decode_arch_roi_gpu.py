"""Regions and latent stores on generated architectures (tests/test_decode_arch_gpu.py's ROI
lists: upsampling 4/3, 6/5 and 10/7 with 0, 1 and 3 spatial synthesis layers, one stream whose
synthesis leaves the 24-bit multiplies, one that takes the per-frame tail; 34 x 66 yuv420 and
45 x 83 rgb).

decode_batch_tensors(roi=...) must give, sample for sample, the numpy crop of decode_batch's
bytes, which test_generated_streams_decode_to_the_oracle[roi-*] shows to be the oracle's; so must
LatentStore.render from an int16 store and from its compact() form.  The rect recipe is
tests/test_decode_roi_gpu.py's (corners, strips, the whole frame, 24 seeded rects; even origins
for 420), and every region call gets a workspace filled with 0xA5."""
import numpy as np
import pytest

import test_decode_arch_gpu as A
from test_decode_roi_gpu import _planes, _roi_tensors, _same, _small_rects

pytestmark = pytest.mark.gpu


def _whole_planes(data, fr):
    """[3 planes] of decode_batch's bytes in the stream's own format: .yuv 420, or a PPM."""
    from ccmi import decode
    h, w = fr.desc.h, fr.desc.w
    if fr.desc.frame_data_type == 1:
        b, = decode.decode_batch([data])
        return _planes(b, h, w, 8, 420), 420
    b, = decode.decode_batch([data], as_yuv=False)
    head = f"P6\n{w} {h}\n255\n".encode()
    assert b.startswith(head) and len(b) == len(head) + 3 * h * w
    return list(np.frombuffer(b[len(head):], dtype="u1").reshape(h, w, 3).transpose(2, 0, 1)), 444


@pytest.mark.parametrize("key", sorted(k for k in A.LISTS if k.startswith("roi-")))
def test_generated_architectures_every_rect_is_the_crop(key, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    frames, datas = A.made(key), A.written(key)
    for i, ((fr, _), data) in enumerate(zip(frames, datas)):
        h, w = fr.desc.h, fr.desc.w
        planes, chroma = _whole_planes(data, fr)
        rects = _small_rects(h, w, chroma, 300 + i)
        windowed = i != len(datas) - 1  # the last stream of a list has a generic synthesis
        plan = decode.roi_plan([data] * len(rects), rects)
        assert all(p["windowed"] == windowed for p in plan), (key, i)
        outs = _roi_tensors([data] * len(rects), rects)
        for r, o in zip(rects, outs):
            _same(o, planes, r, chroma, f"{key}[{i}] in one call")
        for r in (rects[4], rects[7], rects[20]):
            o, = _roi_tensors([data], [r])
            _same(o, planes, r, chroma, f"{key}[{i}] alone")
        # decode once, render regions: int16 latents and their segmented form
        eight = rects[:1] + rects[3:6] + rects[12:16]
        store = decode.LatentStore([data], dtype=torch.int16)
        small = store.compact()
        for st, what in ((store, "store"), (small, "compact store")):
            assert all(p["windowed"] == windowed for p in st.roi_plan([0] * len(eight), eight))
            ws = torch.full((max(st.render_geometry([0] * len(eight), eight)[1], 256),), 0xA5, dtype=torch.uint8, device=gpu)
            for r, o in zip(eight, st.render([0] * len(eight), eight, workspace=ws)):
                _same(o, planes, r, chroma, f"{key}[{i}] {what}")
        small.close()
        store.close()


def test_all_architectures_of_a_size_in_one_region_call(gpu, ccmi_lib):
    """The ten window-form architectures of one size and the per-frame-tail one in ONE region call
    with one rect each: window groups of mixed architectures, and both forms side by side."""
    for key in sorted(k for k in A.LISTS if k.startswith("roi-")):
        frames, datas = A.made(key), A.written(key)
        h, w = frames[0][0].desc.h, frames[0][0].desc.w
        chroma = 420 if frames[0][0].desc.frame_data_type == 1 else 444
        rects = _small_rects(h, w, chroma, 77)[10: 10 + len(datas)]
        same_size = [rects[0]] * len(datas)
        for rr in (rects, same_size):
            outs = _roi_tensors(datas, rr)
            for (fr, _), data, r, o in zip(frames, datas, rr, outs):
                _same(o, _whole_planes(data, fr)[0], r, chroma, key)
