"""numpy restatement of the segmented latent-store form (CCMI_LATENT_SEG, include/ccmi.h):
one grid of integer latents -> (descriptors, payload words), and back.  Written from the
contract's text, value by value; shares no code with the library."""
import numpy as np

SEG = 64
WIDTHS = (0, 2, 4, 8, 16, 32)


def code_of(values) -> int:
    """The smallest code k whose width b holds every value in [-2^(b-1), 2^(b-1) - 1]; b = 0: all zero."""
    lo, hi = int(np.min(values)), int(np.max(values))
    for k, b in enumerate(WIDTHS):
        if b == 0:
            if lo == 0 and hi == 0:
                return k
        elif -(1 << (b - 1)) <= lo and hi <= (1 << (b - 1)) - 1:
            return k
    raise ValueError("a latent outside int32")


def pack_grid(grid):
    """grid [h, w] of integers -> (desc uint32 [h * nseg], payload uint32 [words])."""
    grid = np.asarray(grid, dtype=np.int64)
    h, w = grid.shape
    nseg = (w + SEG - 1) // SEG
    desc = np.zeros(h * nseg, dtype=np.uint32)
    words = []
    for r in range(h):
        for s in range(nseg):
            vals = grid[r, SEG * s: min(SEG * s + SEG, w)]
            k = code_of(vals)
            b = WIDTHS[k]
            off = len(words)
            if off >= 1 << 29:
                raise ValueError("a segment's word offset does not fit 29 bits")
            desc[r * nseg + s] = (off << 3) | k
            bits = 0  # the segment's words as one little-endian bit string, held as a Python int
            for j, v in enumerate(vals):
                bits |= (int(v) & ((1 << b) - 1)) << (j * b)
            for t in range((len(vals) * b + 31) // 32):
                words.append((bits >> (32 * t)) & 0xFFFFFFFF)
    return desc, np.array(words, dtype=np.uint32)


def unpack_grid(desc, payload, h, w):
    """The inverse: (desc, payload) -> int32 grid [h, w]."""
    nseg = (w + SEG - 1) // SEG
    out = np.zeros((h, w), dtype=np.int32)
    for r in range(h):
        for s in range(nseg):
            d = int(desc[r * nseg + s])
            b, off = WIDTHS[d & 7], d >> 3
            c = min(SEG * s + SEG, w) - SEG * s
            n = (c * b + 31) // 32
            bits = 0
            for t in range(n):
                bits |= int(payload[off + t]) << (32 * t)
            for j in range(c):
                f = (bits >> (j * b)) & ((1 << b) - 1) if b else 0
                if b and f >> (b - 1):
                    f -= 1 << b
                out[r, SEG * s + j] = f
    return out


def align(v, a):
    return (v + a - 1) // a * a


def grid_bytes(desc, payload) -> int:
    """Store bytes of one non-empty grid: the descriptor table, then the payload, each 16-byte aligned."""
    return align(4 * len(desc), 16) + align(4 * len(payload), 16)


def stream_bytes(n_ups, n_syn, grids) -> int:
    """Store bytes of one stream: upsampling and synthesis integers, then the grids ((desc, payload),
    or None for a grid whose coded substream is empty), rounded up to 256."""
    pos = align(4 * n_ups, 16) + align(4 * n_syn, 16)
    for g in grids:
        if g is not None:
            pos += grid_bytes(*g)
    return align(pos, 256)


def stream_image(ups, syn, grids) -> bytes:
    """The stream's part of a store, byte for byte, padding as zeros; with the mask of the bytes the
    contract defines (padding is not defined): (bytes, bool mask)."""
    out, mask = bytearray(), bytearray()

    def part(a):
        raw = np.ascontiguousarray(a).tobytes()
        pad = align(len(raw), 16) - len(raw)
        out.extend(raw + b"\0" * pad)
        mask.extend(b"\1" * len(raw) + b"\0" * pad)
    part(np.asarray(ups, dtype=np.int32))
    part(np.asarray(syn, dtype=np.int32))
    for g in grids:
        if g is not None:
            part(g[0])
            part(g[1])
    pad = align(len(out), 256) - len(out)
    out.extend(b"\0" * pad)
    mask.extend(b"\0" * pad)
    return bytes(out), np.frombuffer(bytes(mask), dtype=np.uint8).astype(bool)
