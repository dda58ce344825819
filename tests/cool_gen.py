"""Generated .cool streams of any architecture the header can carry (test data, not product
code).  Nothing is taken from a committed stream: make() fills a fresh CoolDesc and seeded
integer networks in the slot layout the writer and the decoder read (enc_host.cpp
slot_lengths / dec_host.cpp decode_frame_weights):

  arm_w   per hidden layer d x d, then the 2 x d output rows      arm_b  the biases alike
  ups_w   n_ups half kernels of (ups_k + 1) / 2 taps, then n_pre of (pre_k + 1) / 2; the
          decoder mirrors the first nw / 2 * 2 taps of a half onto the kernel's tail
  syn_w   n_branches blend weights (only when n_branches > 1), then per branch, per layer
          [n_out][c_in][ks][ks]                                    syn_b  per branch, per layer
  decoded integer = coded << q_step_index[slot]

The networks are drawn so that the decoded picture is not flat.  A float restatement of the
decoder tail (real(): refine, 2x upsampling, synthesis, blend; no rounding) runs on the case's
own latents while the synthesis is drawn, and every layer is scaled on what it would see:
wide hidden layers to unit spread, layers of up to 8 planes to mean 1/2 and spread 0.3 of
full scale (residual ones add a spread of 0.08), so that most samples end inside (0, 1) and
both output clamps act.  Blend weights alternate in sign (1.3, -0.5, 0.2, -0.2, ...): a sum of
clamped branches with positive weights could never go below 0.

big_syn_weight=v plants ONE synthesis weight of decoded value exactly v (the synthesis q-step
is then 0, so that odd values exist) where the picture survives it:
  layer 0      hidden unit 0 <- coarsest grid; unit 0's weights into layer 1 are 1, -2, 3 (/4096)
  layer 1      output plane 1 <- hidden unit 0, which is made sparse and small (weights of +-3,
               a negative bias), so the weight acts on a few percent of the pixels
  layer l >= 2 output plane 2 <- input plane 0, tap (0, 2); sums wrap (the reference's int32),
               plane 2 turns to noise and clamps, planes 0 and 1 stay
"""
from __future__ import annotations

import numpy as np

UNIT = 1 << 12
FRAME_TYPES = {"rgb": 0, "yuv420": 1, "yuv444": 2}


def grid_sizes(H, W, n_grids):
    out = []
    for _ in range(n_grids):
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def slot_lengths(desc) -> dict:
    """Integers per network slot, from the header fields alone."""
    d, nh = desc.dim_arm, desc.n_hidden_arm
    nw = desc.n_branches if desc.n_branches > 1 else 0
    nb, c = 0, desc.n_grids
    for l in range(desc.n_syn_layers):
        nw += desc.n_branches * c * desc.syn_ks[l] ** 2 * desc.syn_out[l]
        nb += desc.n_branches * desc.syn_out[l]
        c = desc.syn_out[l]
    return {"arm_w": nh * d * d + 2 * d, "arm_b": nh * d + 2,
            "ups_w": desc.n_ups * ((desc.ups_k + 1) // 2) + desc.n_pre * ((desc.pre_k + 1) // 2), "ups_b": 0,
            "syn_w": nw, "syn_b": nb}


def layers_of(desc) -> list:
    return [(int(desc.syn_out[i]), int(desc.syn_ks[i]), int(desc.syn_type[i]) // 16 == 1, int(desc.syn_type[i]) % 16 == 1)
            for i in range(desc.n_syn_layers)]


def _mirror(half, ks):
    """Full kernel the decoder builds of a coded half (decode_upsweights_qi)."""
    nw = (ks + 1) // 2
    k = np.zeros(ks, dtype=np.int64)
    k[:nw] = half
    for i in range(nw // 2 * 2):
        k[ks - 1 - i] = k[i]
    return k


def decoded_nets(frame) -> dict:
    """The decoder's integers of a frame (coded << q-step), in the layout ccmi_decode_weights_i32
    reports: 'ups' n_ups full kernels then n_pre, 'syn' per branch and layer W then b, flat;
    and by parts: 'ups_k' / 'pre_k' lists, 'branches' [[(W [o, c, ks, ks], b [o])]], 'blend'."""
    d = frame.desc
    q = [int(v) for v in d.q_step_index]
    uw = frame.nn["ups_w"].astype(np.int64) << q[2]
    nu, npre = (d.ups_k + 1) // 2, (d.pre_k + 1) // 2
    ups = [_mirror(uw[i * nu: (i + 1) * nu], d.ups_k) for i in range(d.n_ups)]
    off = d.n_ups * nu
    pre = [_mirror(uw[off + i * npre: off + (i + 1) * npre], d.pre_k) for i in range(d.n_pre)]
    sw = frame.nn["syn_w"].astype(np.int64) << q[4]
    sb = frame.nn["syn_b"].astype(np.int64) << q[5]
    pw = pb = 0
    blend = None
    if d.n_branches > 1:
        blend, pw = sw[: d.n_branches].copy(), d.n_branches
    branches, flat = [], []
    for _ in range(d.n_branches):
        c, br = d.n_grids, []
        for n_out, ks, _, _ in layers_of(d):
            nw = n_out * c * ks * ks
            br.append((sw[pw: pw + nw].reshape(n_out, c, ks, ks), sb[pb: pb + n_out]))
            flat += [sw[pw: pw + nw], sb[pb: pb + n_out]]
            pw, pb, c = pw + nw, pb + n_out, n_out
        branches.append(br)
    return {"ups": np.concatenate(ups + pre).astype(np.int32), "syn": np.concatenate(flat).astype(np.int32),
            "ups_k": ups, "pre_k": pre, "branches": branches, "blend": blend}


# ---------------------------------------------------------------- the tail in floats
def _refine(v, k):
    """out = in + separable zero-padded filter (ups_refine), k in real units."""
    ks, pad = len(k), len(k) // 2
    h, w = v.shape
    p = np.pad(v, ((0, 0), (pad, pad)))
    t = sum(p[:, i: i + w] * k[i] for i in range(ks))
    p = np.pad(t, ((pad, pad), (0, 0)))
    return v + sum(p[i: i + h, :] * k[i] for i in range(ks))


def _up2(v, k, ho, wo):
    """2x polyphase upsampling with replicate padding (ups_up2), cropped to ho x wo."""
    ks = len(k) // 2
    pad = ks // 2

    def axis(a):  # along the last axis
        n = a.shape[-1]
        idx = np.arange(n)
        e = sum(a[..., np.clip(idx - pad + i, 0, n - 1)] * k[2 * i] for i in range(ks))
        o = sum(a[..., np.clip(idx - pad + 1 + i, 0, n - 1)] * k[2 * i + 1] for i in range(ks))
        return np.stack([e, o], axis=-1).reshape(*a.shape[:-1], 2 * n)
    return axis(axis(v)[:, :wo].T).T[:ho]


def real_ups(nets, latents, sizes, n_ups, n_pre):
    """[L, H, W] float synthesis input in units of 1.0, as run_ups orders the kernels."""
    L = len(sizes)
    out = []
    for l in range(L):
        v = np.asarray(latents[l], dtype=np.float64).reshape(sizes[l])
        if l < L - 1 or l == 0:
            v = _refine(v, nets["pre_k"][(L - 2 - l) % n_pre] / UNIT)
        for t in range(l - 1, -1, -1):
            v = _up2(v, nets["ups_k"][(L - 2 - t) % n_ups] / UNIT, *sizes[t])
        out.append(v)
    return np.stack(out)


def _conv(x, wt, b, res, relu):
    o, _, ks, _ = wt.shape
    p, (_, h, w) = ks // 2, x.shape
    xp = np.pad(x, ((0, 0), (p, p), (p, p)), mode="edge")
    y = np.zeros((o, h, w)) + np.asarray(b, dtype=np.float64)[:, None, None]
    for a in range(ks):
        for c in range(ks):
            y += np.tensordot(wt[:, :, a, c], xp[:, a: a + h, c: c + w], axes=1)
    if res:
        y += x[:o]
    return np.maximum(y, 0) if relu else y


def _flags(layers):
    """(residual, relu) the decoder applies per layer: a leading pair of 1x1 layers is the fused
    form, ReLU then linear whatever their flags say (synfused_cpu.hpp)."""
    f = [(bool(r), bool(a)) for _, _, r, a in layers]
    if len(layers) >= 2 and layers[0][1] == 1 and layers[1][1] == 1:
        f[0], f[1] = (False, True), (False, False)
    return f


# ---------------------------------------------------------------- the draw
def make(H, W, *, n_grids, dim_arm, n_hidden, ups_k, pre_k, n_ups, n_pre, layers, n_branches=1, frame_type,
         bitdepth=8, hls_sig_blksize=-16, big_syn_weight=None, big_layer=0, seed):
    """(CoolFrame, [int32 latent grid arrays]) of one intra frame.  layers: [(n_out, ks, residual,
    relu)]; frame_type 'rgb' / 'yuv420' / 'yuv444'; big_syn_weight / big_layer: see the module."""
    from ccmi.encode import CoolDesc, CoolFrame
    rng = np.random.default_rng(seed)
    sizes = grid_sizes(H, W, n_grids)
    d = CoolDesc()
    d.h, d.w, d.bitdepth, d.frame_data_type = H, W, bitdepth, FRAME_TYPES[frame_type]
    d.intra_period = d.p_period = d.display_index = 0
    d.dim_arm, d.n_hidden_arm = dim_arm, n_hidden
    d.n_ups, d.ups_k, d.n_pre, d.pre_k = n_ups, ups_k, n_pre, pre_k
    d.n_branches, d.n_syn_layers, d.n_grids = n_branches, len(layers), n_grids
    for i, (n, k, res, relu) in enumerate(layers):
        d.syn_out[i], d.syn_ks[i], d.syn_type[i] = int(n), int(k), 16 * int(bool(res)) + int(bool(relu))
    d.flow_gain, d.hls_sig_blksize = 1, hls_sig_blksize
    big = big_syn_weight is not None
    q = [int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(0, 3)), -1,
         0 if big else int(rng.integers(0, 3)), int(rng.integers(10, 14))]
    for k in range(6):
        d.q_step_index[k], d.expgol_count[k] = q[k], -1

    def coded(x, k):  # real units of 1 << 12 (weights) -> the integers the stream carries
        return np.round(np.asarray(x, dtype=np.float64) / (1 << q[k])).astype(np.int64)

    # ---- latents: round(N(0, 2)); every third seed sends the coarsest grid empty
    lat = [np.round(2.0 * rng.standard_normal(h * w)).astype(np.int32) for h, w in sizes]
    for a in lat[:2]:
        if not a.any():
            a[0] = 1
    if seed % 3 == 0 and n_grids >= 3:
        lat[-1][:] = 0
    d.ac_max_val_latent = int(max(np.abs(a).max() for a in lat)) + 2

    # ---- ARM: hidden weights of +-24, output rows of +-6 (small mu), biases of +-4
    dd = dim_arm
    nn = {"arm_w": np.concatenate([rng.integers(-24, 25, n_hidden * dd * dd), rng.integers(-6, 7, 2 * dd)]).astype(np.int64),
          "arm_b": rng.integers(-4, 5, n_hidden * dd + 2).astype(np.int64), "ups_b": np.zeros(0, np.int64)}

    # ---- upsampling: ramps of gain 1 per phase with 6 % noise, one per index; small refine filters
    nu, npre = (ups_k + 1) // 2, (pre_k + 1) // 2
    halves = []
    for _ in range(n_ups):
        r = np.arange(1, nu + 1, dtype=np.float64) ** 1.5 * (1 + 0.06 * rng.standard_normal(nu))
        if nu >= 4:
            r[0] = -0.3 * abs(r[0])
        halves.append(coded(r * UNIT / r.sum(), 2))
    for _ in range(n_pre):
        halves.append(coded(0.08 * UNIT * rng.standard_normal(npre) / np.sqrt(pre_k), 2))
    nn["ups_w"] = np.concatenate(halves)

    # ---- synthesis, layer by layer on what the layer sees
    frame = CoolFrame(desc=d, nn=nn)
    nn["syn_w"], nn["syn_b"] = np.zeros(0, np.int64), np.zeros(0, np.int64)
    ups_nets = {"ups_k": [_mirror(h << q[2], ups_k) for h in halves[:n_ups]],
                "pre_k": [_mirror(h << q[2], pre_k) for h in halves[n_ups:]]}
    x0 = real_ups(ups_nets, lat, sizes, n_ups, n_pre)
    flags = _flags(layers)
    sw, sb = [], []
    if n_branches > 1:
        bl = [1.3, -0.5] + [0.2 * (-1) ** i for i in range(n_branches - 2)]
        sw.append(coded(np.array(bl) * UNIT, 4))
    for _ in range(n_branches):
        # draw: every layer scaled on what it sees
        x, c, wts, bs = x0, n_grids, [], []
        for l, (n_out, ks, _, _) in enumerate(layers):
            res, relu = flags[l]
            wt = rng.standard_normal((n_out, c, ks, ks))
            pre = _conv(x, wt, np.zeros(n_out), False, False)
            g = (0.08 if res else 0.3 if n_out <= 8 else 1.0) / max(pre.std(), 1e-9)
            b = 0.02 * rng.standard_normal(n_out) if res else \
                (0.5 if n_out <= 8 else 0.0) - g * pre.mean(axis=(1, 2)) + 0.05 * rng.standard_normal(n_out)
            wt *= g
            if big and big_layer == 1 and l == 0:  # hidden unit 0 sparse and small
                wt[0] = rng.choice([-3.0, 3.0], size=wt[0].shape) / UNIT
                b[0] = -1.5 * _conv(x, wt[:1], [0.0], False, False).std()
            wts.append(wt)
            bs.append(b)
            x, c = _conv(x, wt, b, res, relu), n_out
        _calibrate(x0, wts, bs, flags)
        # quantise, then plant
        for l, (wt, b) in enumerate(zip(wts, bs)):
            cw, cb = coded(wt * UNIT, 4), coded(b * UNIT * UNIT, 5)
            if big and big_layer == 0 and l == 1:
                cw[:, 0] = np.array([1, -2, 3] * cw.shape[0])[: cw.shape[0], None, None]
            if big and big_layer == l:
                cw[_PLANT[min(l, 2)]] = int(big_syn_weight)
            sw.append(cw.reshape(-1))
            sb.append(cb)
    nn["syn_w"], nn["syn_b"] = np.concatenate(sw), np.concatenate(sb)
    if big:  # Exp-Golomb codes stay within 32 bins only from a count that grows with the value
        d.expgol_count[4] = max(0, 2 * int(abs(int(big_syn_weight))).bit_length() - 30)
    d.ac_max_val_nn = min(65535, int(max(np.abs(v).max(initial=0) for v in nn.values())) + 2)
    return frame, lat


_PLANT = ((0, -1, 0, 0), (1, 0, 0, 0), (2, 0, 0, 2))  # [o, c, ky, kx] of the planted weight in layer 0, 1, >= 2


def _calibrate(x0, wts, bs, flags):
    """Stretch the first three output planes over the clamps: the last non-residual layer (every
    layer after it keeps its planes) gets an affine map per plane, in place, that puts the 3 % and
    97 % quantiles of the stack's last pre-activation at -0.04 and 1.04."""
    plain = [l for l, (res, _) in enumerate(flags) if not res]
    if not plain:
        return
    ls, n = plain[-1], len(wts)
    x = x0
    for l in range(ls):
        x = _conv(x, wts[l], bs[l], *flags[l])
    for _ in range(4):
        y = x
        for l in range(ls, n):
            y = _conv(y, wts[l], bs[l], flags[l][0], flags[l][1] and l < n - 1)
        for o in range(min(3, y.shape[0], wts[ls].shape[0])):
            lo, hi = np.quantile(y[o], [0.03, 0.97])
            if hi - lo < 1e-6:
                continue
            a = float(np.clip(1.08 / (hi - lo), 0.5, 2.0))
            wts[ls][o] *= a
            bs[ls][o] = a * bs[ls][o] - 0.04 - a * lo


def planted_at(frame, big_layer) -> int:
    """Decoded value at the slot big_syn_weight goes to."""
    return int(decoded_nets(frame)["branches"][0][big_layer][0][_PLANT[min(big_layer, 2)]])


def real(frame, latents):
    """Float restatement of the decoder tail on a frame: [n_out, H, W] in units of 1.0 (before the
    output clamp; multi-branch: the blended sum).  What make() tunes against; not a reference."""
    d = frame.desc
    nets = decoded_nets(frame)
    x0 = real_ups(nets, latents, frame.grid_sizes, d.n_ups, d.n_pre)
    layers = layers_of(d)
    outs = []
    for br in nets["branches"]:
        x = x0
        for (wt, b), (res, relu) in zip(br, _flags(layers)):
            x = _conv(x, wt / UNIT, b / (UNIT * UNIT), res, relu)
        outs.append(x)
    if nets["blend"] is None:
        return outs[0]
    return sum(np.clip(o[:3], 0, 1) * (w / UNIT) for o, w in zip(outs, nets["blend"]))


def write(frame, latents, gpu) -> bytes:
    """The stream bytes: GPU ARM contexts + host CABAC.  Every network slot's Exp-Golomb count is
    searched (encode_frame's search_counts), but a slot make() gave a count (a planted big
    weight, whose code would not fit from the searched range 0..12) keeps it."""
    import torch
    from ccmi import encode
    flat = torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in latents])).to(gpu)
    fixed = any(int(c) >= 0 for c in frame.desc.expgol_count)
    copy = encode.CoolFrame(desc=encode.CoolDesc.from_buffer_copy(frame.desc), nn=frame.nn)  # the writer fills its desc in
    return encode.encode_frame(copy, flat.contiguous(), search_counts=not fixed)
