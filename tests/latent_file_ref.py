"""numpy reader and writer of the latent-file form (include/ccmi.h, "Latent stores as files"),
written from the contract's text; shares no code with the library.  SEG grids come from
tests/latent_seg_ref.py.

A stream is a dict:
  type        CCMI_LATENT_* (0 I8, 1 I16, 2 I32, 3 SEG)
  user_flags  u32
  hdr         the 14 header fields by name (HDR)
  layers      [(n_out, ks, residual, relu), ...]
  lat_n       per grid
  seg_words   per grid
  blend       the blend integers
  part        the stream's part of DATA (bytes); part_bytes / part_sum are taken from it unless the
              dict carries them (the tests' corrupt files do)
and may carry record_bytes / n_blend to override what the writer would derive."""
import struct

import numpy as np

import latent_seg_ref as R

MAGIC = b"CCMILAT1"
HDR = ("h", "w", "bitdepth", "frame_data_type", "intra_period", "dim_arm", "n_hidden", "n_ups", "ups_ks", "n_pre", "pre_ks",
       "n_branches", "sig_blk", "n_layers")
I8, I16, I32, SEG = 0, 1, 2, 3
ELEM = {I8: np.int8, I16: np.int16, I32: np.int32}
M64 = (1 << 64) - 1


def align(v, a):
    return (v + a - 1) // a * a


def checksum(b):
    """(sum of w_i, sum of (i + 1) w_i) mod 2^64 over the bytes as little-endian u32 words, zero-extended."""
    b = bytes(b) + b"\0" * (-len(b) % 4)
    w = np.frombuffer(b, dtype="<u4").astype(np.uint64)
    i = np.arange(1, w.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(w.sum(dtype=np.uint64)) & M64, int((w * i).sum(dtype=np.uint64)) & M64


def grid_sizes(h, w, n):
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def net_counts(hdr, layers):
    """(upsampling integers, synthesis integers) of a stream."""
    n_ups = hdr["n_ups"] * hdr["ups_ks"] + hdr["n_pre"] * hdr["pre_ks"]
    per, c = 0, hdr["n_layers"]
    for n_out, ks, _, _ in layers:
        per += n_out * c * ks * ks + n_out
        c = n_out
    return n_ups, per * hdr["n_branches"]


def part_ranges(ltype, hdr, layers, lat_n, seg_words):
    """[(name, offset, bytes)] of the defined ranges of a stream's part, and the part's size."""
    n_ups, n_syn = net_counts(hdr, layers)
    out, pos = [("ups", 0, 4 * n_ups)], align(4 * n_ups, 16)
    out.append(("syn", pos, 4 * n_syn))
    pos += align(4 * n_syn, 16)
    for l, ((h, w), nb) in enumerate(zip(grid_sizes(hdr["h"], hdr["w"], hdr["n_layers"]), lat_n)):
        if not nb:
            continue
        if ltype == SEG:
            nd = h * ((w + 63) // 64)
            out.append(("desc%d" % l, pos, 4 * nd))
            pos += align(4 * nd, 16)
            out.append(("payload%d" % l, pos, 4 * seg_words[l]))
            pos += align(4 * seg_words[l], 16)
        else:
            nbytes = h * w * np.dtype(ELEM[ltype]).itemsize
            out.append(("grid%d" % l, pos, nbytes))
            pos += align(nbytes, 16)
    return out, align(pos, 256)


def part_image(ltype, hdr, layers, lat_n, ups, syn, grids):
    """The part of DATA of one stream and its seg_words.  grids: per grid None (empty) or the [h, w]
    integers.  -> (bytes, mask of the defined bytes, seg_words)."""
    sizes = grid_sizes(hdr["h"], hdr["w"], hdr["n_layers"])
    packed, seg_words = {}, [0] * hdr["n_layers"]
    for l, g in enumerate(grids):
        if g is None or not lat_n[l]:
            continue
        g = np.asarray(g).reshape(sizes[l])
        if ltype == SEG:
            packed[l] = R.pack_grid(g)
            seg_words[l] = len(packed[l][1])
        else:
            assert np.array_equal(g.astype(ELEM[ltype]), g), "a latent does not fit the type"
            packed[l] = g.astype(ELEM[ltype])
    ranges, size = part_ranges(ltype, hdr, layers, lat_n, seg_words)
    img, mask = np.zeros(size, dtype=np.uint8), np.zeros(size, dtype=bool)
    for name, off, nb in ranges:
        if name == "ups":
            raw = np.asarray(ups, dtype="<i4").tobytes()
        elif name == "syn":
            raw = np.asarray(syn, dtype="<i4").tobytes()
        elif name.startswith("desc"):
            raw = packed[int(name[4:])][0].astype("<u4").tobytes()
        elif name.startswith("payload"):
            raw = packed[int(name[7:])][1].astype("<u4").tobytes()
        else:
            raw = np.ascontiguousarray(packed[int(name[4:])]).tobytes()
        assert len(raw) == nb, (name, len(raw), nb)
        img[off: off + nb] = np.frombuffer(raw, dtype=np.uint8)
        mask[off: off + nb] = True
    return img.tobytes(), mask, seg_words


def record(s):
    """One INDEX record."""
    part = s.get("part", b"")
    sums = s.get("part_sum", checksum(part))
    body = struct.pack("<IQQQI", s["type"], s.get("part_bytes", len(part)), sums[0], sums[1], s.get("user_flags", 0))
    body += struct.pack("<14i", *[s["hdr"][k] for k in HDR])
    body += struct.pack("<I", len(s["layers"]))
    for L in s["layers"]:
        body += struct.pack("<4i", *L)
    body += struct.pack("<%dI" % len(s["lat_n"]), *s["lat_n"])
    body += struct.pack("<%dI" % len(s["seg_words"]), *s["seg_words"])
    body += struct.pack("<I", s.get("n_blend", len(s["blend"])))
    body += struct.pack("<%di" % len(s["blend"]), *s["blend"])
    n = align(4 + len(body), 8)
    body += b"\0" * (n - 4 - len(body))
    return struct.pack("<I", s.get("record_bytes", n)) + body


def head(count, index, data_bytes, **over):
    index_bytes = over.get("index_bytes", len(index))
    data_off = over.get("data_off", align(64 + len(index), 256))
    sums = over.get("index_sum", checksum(index))
    return (over.get("magic", MAGIC) + struct.pack("<IIQQQQQQ", over.get("version", 1), over.get("n_streams", count),
                                                   index_bytes, data_off, data_bytes, sums[0], sums[1], 0))


def write_meta(streams, **over):
    index = b"".join(record(s) for s in streams)
    data_bytes = over.pop("data_bytes", sum(s.get("part_bytes", len(s.get("part", b""))) for s in streams))
    return head(len(streams), index, data_bytes, **over) + index


def write_file(streams, **over):
    meta = write_meta(streams, **over)
    return meta + b"\0" * (align(len(meta), 256) - len(meta)) + b"".join(s["part"] for s in streams)


def with_index_sum(meta):
    """META with index_sum recomputed over its INDEX bytes."""
    meta = bytearray(meta)
    meta[40:56] = struct.pack("<QQ", *checksum(bytes(meta[64:])))
    return bytes(meta)


def read_meta(b):
    """HEAD and INDEX -> dict; asserts the form."""
    assert b[:8] == MAGIC
    version, n, index_bytes, data_off, data_bytes, s0, s1, zero = struct.unpack_from("<IIQQQQQQ", b, 8)
    assert version == 1 and n >= 1 and zero == 0 and index_bytes % 8 == 0
    assert data_off == align(64 + index_bytes, 256)
    index = b[64: 64 + index_bytes]
    assert len(index) == index_bytes and checksum(index) == (s0, s1)
    streams, pos, at = [], 64, data_off
    for _ in range(n):
        start = pos
        nb, ltype, part_bytes, p0, p1, flags = struct.unpack_from("<IIQQQI", b, pos)
        pos += 36
        hdr = dict(zip(HDR, struct.unpack_from("<14i", b, pos)))
        pos += 56
        n_syn, = struct.unpack_from("<I", b, pos)
        pos += 4
        layers = [struct.unpack_from("<4i", b, pos + 16 * k) for k in range(n_syn)]
        pos += 16 * n_syn
        L = hdr["n_layers"]
        lat_n = list(struct.unpack_from("<%dI" % L, b, pos))
        seg_words = list(struct.unpack_from("<%dI" % L, b, pos + 4 * L))
        pos += 8 * L
        n_blend, = struct.unpack_from("<I", b, pos)
        blend = list(struct.unpack_from("<%di" % n_blend, b, pos + 4))
        pos += 4 + 4 * n_blend
        pos = start + align(pos - start, 8)
        assert nb == pos - start and nb % 8 == 0
        assert n_blend == (hdr["n_branches"] if hdr["n_branches"] > 1 else 0)
        ranges, size = part_ranges(ltype, hdr, layers, lat_n, seg_words)
        assert part_bytes == size and size % 256 == 0
        streams.append(dict(type=ltype, user_flags=flags, hdr=hdr, layers=layers, lat_n=lat_n, seg_words=seg_words, blend=blend,
                            part_bytes=part_bytes, part_sum=(p0, p1), record_bytes=nb, data_at=at, ranges=ranges))
        at += part_bytes
    assert pos == 64 + index_bytes and at == data_off + data_bytes
    return dict(n_streams=n, index_bytes=index_bytes, data_off=data_off, data_bytes=data_bytes, streams=streams)


def read_file(b):
    """The whole file: read_meta plus each stream's part, its checksum checked, its defined-byte
    mask, and its padding checked to be 0."""
    b = bytes(b)
    f = read_meta(b)
    assert len(b) == f["data_off"] + f["data_bytes"]
    assert not any(b[64 + f["index_bytes"]: f["data_off"]])
    for s in f["streams"]:
        part = b[s["data_at"]: s["data_at"] + s["part_bytes"]]
        assert checksum(part) == s["part_sum"]
        mask = np.zeros(len(part), dtype=bool)
        for _, off, nb in s["ranges"]:
            mask[off: off + nb] = True
        assert not np.frombuffer(part, dtype=np.uint8)[~mask].any(), "undefined bytes of a part are not 0"
        s["part"], s["mask"] = part, mask
    return f


def stream_of_cool(fr, ltype, seg_words=None, user_flags=0):
    """A stream dict (without its part) from encode.parse's facts of a .cool stream."""
    d = fr.desc
    hdr = dict(h=d.h, w=d.w, bitdepth=d.bitdepth, frame_data_type=d.frame_data_type, intra_period=d.intra_period,
               dim_arm=d.dim_arm, n_hidden=d.n_hidden_arm, n_ups=d.n_ups, ups_ks=d.ups_k, n_pre=d.n_pre, pre_ks=d.pre_k,
               n_branches=d.n_branches, sig_blk=d.hls_sig_blksize, n_layers=d.n_grids)
    layers = [(d.syn_out[l], d.syn_ks[l], int((d.syn_type[l] >> 4) != 0), int((d.syn_type[l] & 15) != 0))
              for l in range(d.n_syn_layers)]
    lat_n = [int(v) for v in d.n_bytes_latent[: d.n_grids]]
    sw = [0] * d.n_grids if seg_words is None else [w if nb else 0 for w, nb in zip(seg_words, lat_n)]
    blend = [0] * d.n_branches if d.n_branches > 1 else []
    s = dict(type=ltype, user_flags=user_flags, hdr=hdr, layers=layers, lat_n=lat_n, seg_words=sw, blend=blend)
    _, s["part_bytes"] = part_ranges(ltype, hdr, layers, lat_n, sw)
    s["part_sum"] = (0, 0)
    return s
