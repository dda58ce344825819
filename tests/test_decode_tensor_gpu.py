"""Path B device sink: ccmi_decode_batch_dev / decode.decode_batch_tensors leave the decoded
frames on the GPU as planar tensors.  The reference is always code that existed before this
path and is itself pinned to the reference decoder: tests/golden/ref_md5.json, the bytes of
decode.decode_batch, the C oracle's cco_decode_file -- never the tensor path itself.

Generated streams (tests/synth_streams.py's recipe: the networks of a committed class-D
stream, another frame size, seeded N(0, 2) integer latents, written by the GPU writer):
(21, 37), (19, 64), (34, 66) -- W mod 4 = 1, 0, 2, two odd heights, every plane a few
samples long, so the output kernel's partial first / last groups and the groups that cross
from the luma into the chroma planes are a large share of each frame.  One more (21, 37)
stream has its third synthesis layer turned from 3x3 into 1x1: dec_tail.hip's syn_fast()
refuses it, so it is the one stream here that takes the per-frame decoder tail
(dec_output_tensor, dec_out.hip); every other stream, committed or generated, alone or in a
batch, has a fused-synthesis architecture with one branch and takes the batched tail
(dec_output_tensor_batch, a group per geometry and chunk, dec_host.cpp)."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import synth_streams as S

GOLDEN = Path(__file__).resolve().parent / "golden"
MD5 = json.loads((GOLDEN / "ref_md5.json").read_text())
FILES = sorted((GOLDEN / "cool").glob("*.cool"))
CLIC = sorted((GOLDEN / "cool" / "clic").glob("*.cool"))
DE8 = [f for f in FILES if f.name[:2] in ("D-", "E-")][:8]
SMALL = ((21, 37), (19, 64), (34, 66))

pytestmark = pytest.mark.gpu


def _key(f):
    if f.parent.name == "clic":
        return "clic20-pro-valid/" + f.name
    return ("kodak/" if f.name.startswith("kodim") else "jvet/") + f.name


def _np(t):
    return t.cpu().numpy()


def _flat(item):
    """One decode_batch_tensors item -> its samples in memory order (1-D numpy)."""
    if isinstance(item, dict):
        return np.concatenate([_np(item[k]).reshape(-1) for k in "yuv"])
    return _np(item).reshape(-1)


def _from_bytes(b, bitdepth):
    return np.frombuffer(b, dtype="u1" if bitdepth <= 8 else "<u2")


@pytest.fixture(scope="module")
def small(gpu, ccmi_lib):
    """The generated streams: [(21, 37), (19, 64), (34, 66), (21, 37) with a generic synthesis]."""
    import torch
    from ccmi import encode

    def build(h, w, seed, generic=False):
        fr = encode.parse(S.BASE.read_bytes())
        d = fr.desc
        d.h, d.w = h, w
        if generic:
            # layer 2 (3 -> 3, 3x3, after the fused 1x1 pair) keeps its centre taps only
            c_in, p, parts = d.n_grids, 0, []
            assert d.n_syn_layers >= 3 and d.syn_ks[2] == 3 and d.n_branches == 1
            for l in range(d.n_syn_layers):
                n = d.syn_out[l] * c_in * d.syn_ks[l] ** 2
                wl = fr.nn["syn_w"][p: p + n]
                if l == 2:
                    wl = wl.reshape(d.syn_out[l], c_in, 3, 3)[:, :, 1, 1].reshape(-1)
                parts.append(wl)
                p, c_in = p + n, d.syn_out[l]
            assert p == fr.nn["syn_w"].size
            fr.nn["syn_w"] = np.concatenate(parts)
            d.syn_ks[2] = 1
        g = torch.Generator().manual_seed(seed)
        lat = [torch.round(2.0 * torch.randn(hh * ww, generator=g)).to(torch.int32) for hh, ww in fr.grid_sizes]
        d.ac_max_val_latent = min(65535, max(int(a.abs().max()) for a in lat) + 2)
        return encode.encode_frame(fr, torch.cat(lat).to(gpu), search_counts=True)

    return [build(h, w, 7 + i) for i, (h, w) in enumerate(SMALL)] + [build(21, 37, 11, generic=True)]


@pytest.fixture(scope="module")
def odd_clic():
    """(stream, H, W) of the committed CLIC stream whose width and height are both odd."""
    from ccmi import encode
    hit = []
    for f in CLIC:
        d = encode.parse(f.read_bytes()).desc
        if d.h % 2 == 1 and d.w % 2 == 1:
            hit.append((f, d.h, d.w))
    assert hit, "no committed CLIC stream with odd width and height left"
    f, h, w = hit[0]
    assert h % 2 == 1 and w % 2 == 1 and (h, w) == (1725, 1145)
    return f, h, w


@pytest.fixture(scope="module")
def odd_444_16(odd_clic, gpu, ccmi_lib):
    """The odd CLIC stream at 444 / 16 bits as a tensor (numpy [3, H, W], uint16): checked
    against the PPM bytes in one test and the structural reference of 420 / 16 in another."""
    from ccmi import decode
    t, = decode.decode_batch_tensors([odd_clic[0].read_bytes()], output_bitdepth=16, output_chroma_format=444)
    return _np(t)


def test_pinned_md5_yuv420(gpu, ccmi_lib):
    """Planar u8 420 is the .yuv file layout: the md5 goes straight to the reference decoder's."""
    import torch
    from ccmi import decode
    assert len(DE8) == 8
    outs = decode.decode_batch_tensors([f.read_bytes() for f in DE8])
    for f, o in zip(DE8, outs):
        assert set(o) == {"y", "u", "v"} and o["y"].dtype == torch.uint8 and o["y"].is_cuda
        e = MD5[_key(f)]
        assert tuple(o["y"].shape) == (e["h"], e["w"]) and tuple(o["u"].shape) == (e["h"] // 2, e["w"] // 2)
        got = torch.cat([o["y"].flatten(), o["u"].flatten(), o["v"].flatten()]).cpu().numpy().tobytes()
        assert len(got) == e["bytes"]
        assert hashlib.md5(got).hexdigest() == e["md5"], f.name


def test_pinned_md5_rgb444(odd_clic, gpu, ccmi_lib):
    """Two Kodak streams and the odd-sized CLIC stream: [3, H, W] u8, interleaved behind the
    P6 header, has the reference decoder's PPM md5."""
    import torch
    from ccmi import decode
    fs = [f for f in FILES if f.name.startswith("kodim")][:2] + [odd_clic[0]]
    outs = decode.decode_batch_tensors([f.read_bytes() for f in fs])
    for f, o in zip(fs, outs):
        e = MD5[_key(f)]
        assert o.dtype == torch.uint8 and tuple(o.shape) == (3, e["h"], e["w"])
        ppm = b"P6\n%d %d\n255\n" % (e["w"], e["h"]) + o.permute(1, 2, 0).contiguous().cpu().numpy().tobytes()
        assert len(ppm) == e["bytes"]
        assert hashlib.md5(ppm).hexdigest() == e["md5"], f.name
    assert tuple(outs[2].shape) == (3, odd_clic[1], odd_clic[2])


@pytest.mark.parametrize("bitdepth", [8, 10])
def test_odd_size_yuv420_matches_byte_path(bitdepth, odd_clic, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    f, H, W = odd_clic
    data = [f.read_bytes()]
    ref, = decode.decode_batch(data, output_bitdepth=bitdepth, output_chroma_format=420, as_yuv=True)
    o, = decode.decode_batch_tensors(data, output_bitdepth=bitdepth, output_chroma_format=420)
    assert o["y"].dtype == (torch.uint8 if bitdepth == 8 else torch.uint16)
    assert tuple(o["y"].shape) == (H, W) and tuple(o["u"].shape) == tuple(o["v"].shape) == (H // 2, W // 2)
    assert np.array_equal(_flat(o), _from_bytes(ref, bitdepth))


def test_odd_size_16_bit_444_matches_ppm(odd_clic, odd_444_16, gpu, ccmi_lib):
    from ccmi import decode
    f, H, W = odd_clic
    ppm, = decode.decode_batch([f.read_bytes()], output_bitdepth=16, as_yuv=False)
    hdr = b"P6\n%d %d\n65535\n" % (W, H)
    assert ppm.startswith(hdr)
    ref = np.frombuffer(ppm[len(hdr):], dtype=">u2").reshape(H, W, 3).transpose(2, 0, 1)
    assert odd_444_16.dtype == np.uint16 and odd_444_16.shape == (3, H, W)
    assert np.array_equal(odd_444_16, ref)


def test_odd_size_16_bit_420_structure(odd_clic, odd_444_16, gpu, ccmi_lib):
    """No byte-path counterpart at 16-bit 420 (the .yuv writer stops at 10 bits): y is plane
    0 of the 444 result, u and v its planes 1 and 2 at the even rows and columns, floor size."""
    from ccmi import decode
    f, H, W = odd_clic
    o, = decode.decode_batch_tensors([f.read_bytes()], output_bitdepth=16, output_chroma_format=420)
    assert np.array_equal(_np(o["y"]), odd_444_16[0])
    assert np.array_equal(_np(o["u"]), odd_444_16[1][::2, ::2][: H // 2, : W // 2])
    assert np.array_equal(_np(o["v"]), odd_444_16[2][::2, ::2][: H // 2, : W // 2])


@pytest.mark.parametrize("bitdepth,chroma", [(8, 420), (8, 444), (10, 420), (10, 444)])
def test_small_geometries_head_and_tail_stores(bitdepth, chroma, small, gpu, ccmi_lib, oracle_c, tmp_path):
    """(21, 37), (19, 64), (34, 66) and the generic-synthesis (21, 37) stream, each alone and
    all in one call: the tensors hold decode_batch's samples, which first are shown to be the
    oracle's."""
    import torch
    from ccmi import decode
    refs = decode.decode_batch(small, output_bitdepth=bitdepth, output_chroma_format=chroma, as_yuv=True)
    for i, (d, r) in enumerate(zip(small, refs)):
        (tmp_path / "s.cool").write_bytes(d)
        assert oracle_c.cco_decode_file(str(tmp_path / "s.cool").encode(), str(tmp_path / "o.yuv").encode(), bitdepth,
                                        chroma, 0) == 0
        assert (tmp_path / "o.yuv").read_bytes() == r, f"decode_batch differs from the oracle on generated stream {i}"
    dt = torch.uint8 if bitdepth == 8 else torch.uint16
    geo = list(SMALL) + [SMALL[0]]
    together = decode.decode_batch_tensors(small, output_bitdepth=bitdepth, output_chroma_format=chroma)
    alone = [decode.decode_batch_tensors([d], output_bitdepth=bitdepth, output_chroma_format=chroma)[0] for d in small]
    for outs in (together, alone):
        for (h, w), o, r in zip(geo, outs, refs):
            if chroma == 420:
                assert tuple(o["y"].shape) == (h, w) and tuple(o["u"].shape) == (h // 2, w // 2) and o["v"].dtype == dt
            else:
                assert tuple(o.shape) == (3, h, w) and o.dtype == dt
            assert np.array_equal(_flat(o), _from_bytes(r, bitdepth)), (h, w)


def test_stacked_output_at_odd_addresses(small, gpu, ccmi_lib):
    """Four copies of the (21, 37) stream stacked: 1137 (420) and 2331 (444) u8 samples per
    frame, so frames 1 and 3 start at odd addresses; every frame equals the byte path's."""
    from ccmi import decode
    d = small[0]
    ref420, = decode.decode_batch([d])
    ref444, = decode.decode_batch([d], output_chroma_format=444)
    o = decode.decode_batch_tensors([d] * 4, stack=True)
    assert tuple(o["y"].shape) == (4, 21, 37) and tuple(o["u"].shape) == tuple(o["v"].shape) == (4, 10, 18)
    base = o["y"].data_ptr()
    assert o["u"].data_ptr() == base + 21 * 37 and o["v"].data_ptr() == base + 21 * 37 + 180
    assert o["y"].stride(0) == 1137 and o["y"][1].data_ptr() % 2 == 1 and o["y"][3].data_ptr() % 2 == 1
    rows = np.concatenate([_np(o[k]).reshape(4, -1) for k in "yuv"], axis=1)
    assert rows.shape == (4, 1137)
    for i in range(4):
        assert rows[i].tobytes() == ref420, i
    t = decode.decode_batch_tensors([d] * 4, output_chroma_format=444, stack=True)
    assert tuple(t.shape) == (4, 3, 21, 37) and t[1].data_ptr() % 2 == 1
    for i in range(4):
        assert _np(t[i]).tobytes() == ref444, i


@pytest.mark.parametrize("sample,chroma", [(0, 420), (1, 420), (2, 420), (1, 444)])
def test_c_abi_any_sample_alignment_and_no_stray_writes(sample, chroma, small, gpu, ccmi_lib):
    """ccmi_decode_batch_dev itself with output pointers 0..3 samples past a 16-byte boundary,
    the per-frame tail (generic stream) and the batched tail side by side: the frames are the
    byte path's and the bytes before and after each frame keep their fill pattern."""
    import torch
    from ccmi import decode
    bitdepth = 8 if sample == 0 else 10
    streams = [small[0], small[3]] * 2
    refs = decode.decode_batch(streams[:2], output_bitdepth=bitdepth, output_chroma_format=chroma, as_yuv=True) * 2
    ssize = (1, 2, 4)[sample]
    elems = 21 * 37 + 2 * 10 * 18 if chroma == 420 else 3 * 21 * 37
    slot = (elems * ssize + 64 + 15) // 16 * 16 + 16
    buf = torch.full((4 * slot,), 0xA5, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    offs = [i * slot + 32 + i * ssize for i in range(4)]
    L = decode._bind_dev()
    keep = [C.create_string_buffer(s, len(s)) for s in streams]
    sp = (C.c_void_p * 4)(*[C.cast(b, C.c_void_p) for b in keep])
    ln = (C.c_size_t * 4)(*[len(s) for s in streams])
    op = (C.c_void_p * 4)(*[buf.data_ptr() + o for o in offs])
    cap = (C.c_size_t * 4)(*[elems * ssize] * 4)
    rc = L.ccmi_decode_batch_dev(sp, ln, 4, op, cap, sample, bitdepth, chroma, None, 0,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, decode.lib().ccmi_last_error()
    host = buf.cpu().numpy()
    maxv = np.float32((1 << bitdepth) - 1)
    for i, (o, r) in enumerate(zip(offs, refs)):
        got = host[o: o + elems * ssize]
        want = _from_bytes(r, bitdepth)
        if sample == 2:
            want = want.astype(np.float32) / maxv
            assert got.view(np.float32).tobytes() == want.tobytes(), i
        else:
            assert got.tobytes() == want.tobytes(), i
        lo = offs[i - 1] + elems * ssize if i else 0
        assert (host[lo: o] == 0xA5).all() and (host[o + elems * ssize: (i + 1) * slot] == 0xA5).all(), i


def test_float32_is_one_rounded_division(small, gpu, ccmi_lib):
    """dtype=torch.float32 equals u.to(float32) / maxv of the integer output bit for bit."""
    import torch
    from ccmi import decode
    data = [f.read_bytes() for f in DE8]
    for streams, bitdepth in ((data, 0), ([small[0], small[3]], 10)):
        ints = decode.decode_batch_tensors(streams, output_bitdepth=bitdepth)
        flts = decode.decode_batch_tensors(streams, output_bitdepth=bitdepth, dtype=torch.float32)
        maxv = float((1 << (bitdepth or 8)) - 1)
        for a, b in zip(ints, flts):
            for k in "yuv":
                assert b[k].dtype == torch.float32 and b[k].shape == a[k].shape
                assert torch.equal(b[k].cpu(), a[k].cpu().to(torch.float32) / maxv)
    # 444, 16 bits: every code of the widest sample range that the stream reaches
    a, = decode.decode_batch_tensors([small[1]], output_bitdepth=16, output_chroma_format=444)
    b, = decode.decode_batch_tensors([small[1]], output_bitdepth=16, output_chroma_format=444, dtype=torch.float32)
    assert torch.equal(b.cpu(), a.cpu().to(torch.float32) / 65535.0)


def test_both_tails_and_both_chunks(small, gpu, ccmi_lib):
    """>= 64 streams in one call take dec_host.cpp's two-chunk path (frames split by coded
    size, each chunk's ARM launches and tail on a stream of its own).  The committed class-D
    (416 x 240, twice) and class-E (1280 x 720) streams mixed with the generated ones (three
    times): the cheap chunk holds the generated geometries and the low-rate D / E streams, the
    expensive one the high-rate D and E streams.  All of them take the batched tail, one group
    per (chunk, geometry), except the generic-synthesis (21, 37) stream, which takes the
    per-frame tail in the cheap chunk.  Every output equals the reference decoder's md5
    (committed) or decode_batch's bytes (generated)."""
    from ccmi import decode
    d_e = [f for f in FILES if f.name[:2] in ("D-", "E-")]
    committed = [f for f in d_e if f.name.startswith("D-")] * 2 + [f for f in d_e if f.name.startswith("E-")]
    gen_ref = decode.decode_batch(small)
    items = [("c", f) for f in committed]
    for k in range(3):  # spread the generated streams through the call
        for j in range(len(small)):
            items.insert((k * 17 + j * 5) % len(items), ("g", j))
    assert len(items) >= 64
    blobs = {f: f.read_bytes() for f in set(committed)}
    outs = decode.decode_batch_tensors([blobs[x] if t == "c" else small[x] for t, x in items])
    tm = decode.last_timing()
    assert tm["download"] == 0 and tm["arm_cabac"] > 0 and tm["ups_syn_out"] > 0
    assert decode.last_arm_flags() == [0] * len(items)
    for (t, x), o in zip(items, outs):
        got = _flat(o).tobytes()
        if t == "c":
            assert hashlib.md5(got).hexdigest() == MD5[_key(x)]["md5"], x.name
        else:
            assert got == gen_ref[x], x


def test_caller_workspace_and_errors(small, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    data = [f.read_bytes() for f in DE8[:3]] + [small[3]]
    geom, need = decode.decode_batch_geometry(data)
    assert [(g["height"], g["width"], g["chroma"], g["bitdepth"]) for g in geom][-1] == (21, 37, 420, 8)
    assert geom[0]["elems"] == MD5[_key(DE8[0])]["bytes"] and need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    outs = decode.decode_batch_tensors(data, workspace=ws)
    for f, o in zip(DE8[:3], outs):
        assert hashlib.md5(_flat(o).tobytes()).hexdigest() == MD5[_key(f)]["md5"], f.name
    assert _flat(outs[3]).tobytes() == decode.decode_batch([small[3]])[0]
    with pytest.raises(decode.CcmiError):
        decode.decode_batch_tensors(data, workspace=ws[: need // 2])
    with pytest.raises(decode.CcmiError):
        decode.decode_batch_tensors(data, output_bitdepth=10, dtype=torch.uint8)
    with pytest.raises(ValueError):
        decode.decode_batch_tensors(data, stack=True)  # 416 x 240 and 21 x 37
    with pytest.raises(ValueError):
        decode.decode_batch_tensors(data, dtype=torch.float16)
    with pytest.raises(ValueError):
        decode.decode_batch_tensors([])
    with pytest.raises(decode.CcmiError):
        decode.decode_batch_tensors([data[0][:60]])


def test_byte_path_unchanged_after_a_tensor_decode(gpu, ccmi_lib):
    from ccmi import decode
    data = [f.read_bytes() for f in DE8]
    decode.decode_batch_tensors(data)
    for f, o in zip(DE8, decode.decode_batch(data)):
        assert hashlib.md5(o).hexdigest() == MD5[_key(f)]["md5"], f.name
    assert decode.last_timing()["download"] > 0
