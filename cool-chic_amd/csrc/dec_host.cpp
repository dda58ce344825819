// dec_host.cpp -- path B host side: .cool parsing, network weight decoding (CABAC
// Exp-Golomb, tiny), the execution of a decode plan (decode_run; the plan itself is
// dec_plan.cpp) and the decode C-ABI entry points.
//
// Reference: cc-bitstream.cpp:58-275 (headers, chunking), cc-frame-decoder.cpp:157-353
// (read_arm / read_ups / read_syn and the Q_STEP_*_SHIFT tables :28-108), ccdecapi.cpp
// :673-857 (cc_decode_* driver, output formats).  All latent-layer decoding, upsampling,
// synthesis and output conversion run on the GPU (dec_arm.hip, dec_tail.hip).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "ccmi_cabac.h"
#include "dec_plan.h"

namespace ccmi {

namespace {

struct Reader {
    const uint8_t *p;
    size_t n, pos;
    bool err;
    int u(int nb)
    {
        if (pos + (size_t)nb > n) {
            err = true;
            return 0;
        }
        int v = 0;
        for (int i = 0; i < nb; ++i) v = (v << 8) | p[pos++];
        return v;
    }
    const uint8_t *take(int nb)
    {
        if (nb < 0 || pos + (size_t)nb > n) {
            err = true;
            return nullptr;
        }
        const uint8_t *q = p + pos;
        pos += (size_t)nb;
        return q;
    }
};

struct Lqi {
    int qw, qb, sw, sb, nw, nb;
};

// Exp-Golomb magnitude + EP sign, then << (precision - q_step_shift)  (decode_weights_qi)
bool read_weights(Cabac<HostBytes> &c, int k, int n, int shift, int prec, int32_t *dst)
{
    if (prec < shift) return false;
    for (int i = 0; i < n; ++i) {
        int32_t v = c.expgolomb(k);
        if (v != 0 && c.ep()) v = -v;
        dst[i] = (int32_t)((uint32_t)v << (prec - shift));
    }
    return true;
}

Cabac<HostBytes> cabac_on(const uint8_t *p, int n)
{
    Cabac<HostBytes> c;
    c.src = HostBytes{p, (uint32_t)(n > 0 ? n : 0), 0};
    c.start();
    return c;
}

} // namespace

int parse_frame_header(const uint8_t *bs, size_t n, FrameHost &f)
{
    Reader r{bs, n, 0, false};
    r.u(2);
    f.h = r.u(2);
    f.w = r.u(2);
    int raw = r.u(1);
    f.bitdepth = (raw >> 4) + 8;
    f.frame_data_type = raw & 0xF;
    f.intra_period = r.u(1);
    r.u(1); // p_period
    if (r.err || f.h < 1 || f.w < 1) return ccmi_set_error(CCMI_ERR_BITSTREAM, "truncated GOP header");
    if (f.intra_period != 0)
        return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "inter (P/B) frames are outside the decoded hot path");
    r.u(2); // frame header size
    r.u(1); // display index
    raw = r.u(1);
    f.dim_arm = 8 * (raw >> 4);
    f.n_hidden = raw & 0xF;
    raw = r.u(1);
    f.n_ups = raw >> 4;
    f.ups_ks = raw & 0xF;
    raw = r.u(1);
    f.n_pre = raw >> 4;
    f.pre_ks = raw & 0xF;
    f.n_branches = r.u(1);
    const int n_syn = r.u(1);
    if (r.err || n_syn < 1 || n_syn > CCMI_MAX_SYN_LAYERS)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "bad synthesis layer count %d", n_syn);
    f.layers.resize(n_syn);
    for (auto &L : f.layers) {
        L.n_out = r.u(1);
        L.ks = r.u(1);
        raw = r.u(1);
        L.residual = (raw >> 4) != 0;
        L.relu = (raw & 0xF) != 0;
    }
    r.u(1); // flow gain
    r.u(2); // ac_max_val_nn
    r.u(2); // ac_max_val_latent
    f.sig_blk = (signed char)r.u(1);
    Lqi arm{}, ups{}, syn{};
    Lqi *q[3] = {&arm, &ups, &syn};
    static_assert(sizeof(Lqi) == sizeof(f.lqi[0]), "Lqi layout");
    for (auto *x : q) {
        x->qw = r.u(1);
        x->qb = r.u(1);
        if (x->qb == 255) x->qb = -1;
    }
    for (auto *x : q) {
        x->sw = r.u(1);
        x->sb = x->qb < 0 ? -1 : r.u(1);
    }
    for (auto *x : q) {
        x->nw = r.u(2);
        x->nb = x->qb < 0 ? -1 : r.u(2);
    }
    f.n_layers = r.u(1);
    const int n_grid = r.u(1);
    if (r.err || f.n_layers < 2 || f.n_layers > CCMI_MAX_GRIDS || n_grid != f.n_layers)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "bad latent layer count %d/%d", f.n_layers, n_grid);
    for (int i = 0; i < f.n_layers; ++i)
        if (r.u(1) != 1) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "only 1 feature per latent resolution");
    for (int i = 0; i < f.n_layers; ++i) f.lat_n[i] = (uint32_t)r.u(3);
    if (r.err) return ccmi_set_error(CCMI_ERR_BITSTREAM, "truncated frame header");
    f.wbytes[0] = r.take(arm.nw);
    f.wbytes[1] = r.take(arm.nb < 0 ? 0 : arm.nb);
    f.wbytes[2] = r.take(ups.nw);
    r.take(ups.nb < 0 ? 0 : ups.nb);
    f.wbytes[3] = r.take(syn.nw);
    f.wbytes[4] = r.take(syn.nb < 0 ? 0 : syn.nb);
    for (int i = 0; i < f.n_layers; ++i) f.lat_bytes[i] = r.take((int)f.lat_n[i]);
    if (r.err) return ccmi_set_error(CCMI_ERR_BITSTREAM, "truncated stream (payload shorter than the header says)");
    for (int l = 0, hh = f.h, ww = f.w; l < f.n_layers; ++l, hh = (hh + 1) / 2, ww = (ww + 1) / 2) {
        f.lh[l] = hh;
        f.lw[l] = ww;
    }
    for (int i = 0; i < 3; ++i) memcpy(f.lqi[i], q[i], sizeof(Lqi));
    const int d = f.dim_arm;
    if (d != 8 && d != 16 && d != 24 && d != 32) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "dim_arm %d", d);
    if (f.n_hidden > 4) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "%d ARM hidden layers", f.n_hidden);
    if (arm.qw > 8 || arm.qb < 0 || arm.qb > 16) return ccmi_set_error(CCMI_ERR_BITSTREAM, "ARM q-step index");
    if (ups.qw > 12 || f.n_ups < 1 || f.n_pre < 1 || f.ups_ks < 2 || f.pre_ks < 1)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "upsampling header");
    if (syn.qw > 12 || syn.qb < 0 || syn.qb > 24 || f.n_branches < 1 || f.n_branches > 8)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "synthesis header");
    size_t per_branch = 0;
    {
        int c = f.n_layers;
        for (auto &L : f.layers) {
            if (L.n_out < 1 || L.ks < 1 || (L.ks & 1) == 0) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "syn layer ks %d", L.ks);
            per_branch += (size_t)L.n_out * c * L.ks * L.ks + L.n_out;
            c = L.n_out;
        }
    }
    if (f.layers.back().n_out < 3) return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "synthesis must output >= 3 planes");
    f.arm.assign((size_t)f.n_hidden * (d * d + d) + 2 * d + 2, 0);
    f.ups.assign((size_t)f.n_ups * f.ups_ks + (size_t)f.n_pre * f.pre_ks, 0);
    f.syn.assign(per_branch * f.n_branches, 0);
    if (f.n_branches > 1) f.blend.assign(f.n_branches, 0);
    return CCMI_OK;
}

int decode_frame_weights(FrameHost &f)
{
    Lqi arm{}, ups{}, syn{};
    memcpy(&arm, f.lqi[0], sizeof(Lqi));
    memcpy(&ups, f.lqi[1], sizeof(Lqi));
    memcpy(&syn, f.lqi[2], sizeof(Lqi));
    const uint8_t *arm_w = f.wbytes[0], *arm_b = f.wbytes[1], *ups_w = f.wbytes[2], *syn_w = f.wbytes[3],
                  *syn_b = f.wbytes[4];
    // ---- ARM (read_arm, cc-frame-decoder.cpp:201-258)
    const int d = f.dim_arm;
    {
        auto cw = cabac_on(arm_w, arm.nw), cb = cabac_on(arm_b, arm.nb);
        const int ws = 8 - arm.qw, bsh = 16 - arm.qb;
        int32_t *p = f.arm.data();
        for (int l = 0; l < f.n_hidden; ++l, p += d * d + d)
            if (!read_weights(cw, arm.sw, d * d, ws, kArmPrec, p) || !read_weights(cb, arm.sb, d, bsh, 2 * kArmPrec, p + d * d))
                return ccmi_set_error(CCMI_ERR_BITSTREAM, "ARM weights");
        if (!read_weights(cw, arm.sw, 2 * d, ws, kArmPrec, p) || !read_weights(cb, arm.sb, 2, bsh, 2 * kArmPrec, p + 2 * d))
            return ccmi_set_error(CCMI_ERR_BITSTREAM, "ARM weights");
    }
    // ---- upsampling (read_ups :261-300): half kernels mirrored (decode_upsweights_qi)
    {
        auto cw = cabac_on(ups_w, ups.nw);
        int32_t *p = f.ups.data();
        auto sym = [&](int ks) {
            const int nw = (ks + 1) / 2;
            if (!read_weights(cw, ups.sw, nw, 12 - ups.qw, kUpsPrec, p)) return false;
            for (int i = 0; i < nw / 2 * 2; ++i) p[ks - 1 - i] = p[i];
            p += ks;
            return true;
        };
        for (int l = 0; l < f.n_ups; ++l)
            if (!sym(f.ups_ks)) return ccmi_set_error(CCMI_ERR_BITSTREAM, "upsampling weights");
        for (int l = 0; l < f.n_pre; ++l)
            if (!sym(f.pre_ks)) return ccmi_set_error(CCMI_ERR_BITSTREAM, "upsampling weights");
    }
    // ---- synthesis (read_syn :302-353)
    {
        auto cw = cabac_on(syn_w, syn.nw), cb = cabac_on(syn_b, syn.nb);
        const int ws = 12 - syn.qw, bsh = 24 - syn.qb;
        if (f.n_branches > 1) {
            if (!read_weights(cw, syn.sw, f.n_branches, ws, kSynPrec, f.blend.data()))
                return ccmi_set_error(CCMI_ERR_BITSTREAM, "blend weights");
        }
        int32_t *p = f.syn.data();
        for (int b = 0; b < f.n_branches; ++b) {
            int c = f.n_layers;
            for (auto &L : f.layers) {
                const int nw = c * L.ks * L.ks * L.n_out;
                if (!read_weights(cw, syn.sw, nw, ws, kSynPrec, p) || !read_weights(cb, syn.sb, L.n_out, bsh, 2 * kSynPrec, p + nw))
                    return ccmi_set_error(CCMI_ERR_BITSTREAM, "synthesis weights");
                p += nw + L.n_out;
                c = L.n_out;
            }
        }
    }
    return CCMI_OK;
}

int parse_and_decode_frame(const uint8_t *bs, size_t n, FrameHost &f)
{
    if (int rc = parse_frame_header(bs, n, f)) return rc;
    return decode_frame_weights(f);
}

} // namespace ccmi

using namespace ccmi;

namespace {

thread_local float g_last_ms[4] = {0, 0, 0, 0};
thread_local std::vector<uint32_t> g_last_flags; // per stream: OR of its grids' CCMI_ARM_FLAG_* bits
thread_local int g_last_tails[2] = {0, 0};       // batched tail groups, per-frame tails of the last call

// what every decode, render and planning call clears first: a call that fails, or only plans,
// reports nothing, not the previous call's
void clear_last()
{
    g_last_flags.clear();
    g_last_tails[0] = g_last_tails[1] = 0;
}

// polls per two-wave wait of the chain kernel before it gives up (ArmStreamDesc::spin_cap)
int arm_spin_cap()
{
    const char *e = getenv("CCMI_DEC_SPIN_CAP");
    if (!e || !*e) return 1 << 24;
    const long v = strtol(e, nullptr, 10);
    return v < 0 ? 0 : v > (1L << 30) ? (1 << 30) : (int)v;
}

struct EventSet {
    hipEvent_t e[5] = {};
    bool ok = true;
    EventSet()
    {
        for (auto &x : e)
            if (hipEventCreate(&x) != hipSuccess) ok = false;
    }
    ~EventSet()
    {
        for (auto &x : e)
            if (x) (void)hipEventDestroy(x);
    }
    void rec(int i, hipStream_t s)
    {
        if (ok) (void)hipEventRecord(e[i], s);
    }
};

// every synthesis weight (not the biases) of every branch fits 24 signed bits: the fused
// integer synthesis then multiplies with v_mul_i32_i24 (DecSynArgs::f24)
bool syn_weights_fit24(const FrameHost &f)
{
    const size_t per_branch = f.syn.size() / (size_t)std::max(1, f.n_branches);
    for (int b = 0; b < f.n_branches; ++b) {
        size_t q = per_branch * (size_t)b;
        int c = f.n_layers;
        for (const SynLayerDesc &L : f.layers) {
            const size_t nw = (size_t)L.n_out * c * L.ks * L.ks;
            if (q + nw > f.syn.size()) return false;
            for (size_t i = 0; i < nw; ++i) {
                const int32_t v = f.syn[q + i];
                if (v < -(1 << 23) || v >= (1 << 23)) return false;
            }
            q += nw + (size_t)L.n_out;
            c = L.n_out;
        }
    }
    return true;
}

// every ARM weight fits 24 signed bits (ArmStreamDesc::flags bit 0); biases sit between
// weight blocks, checking them too is conservative
bool arm_weights_fit24(const FrameHost &f)
{
    for (const int32_t v : f.arm)
        if (v >= (1 << 23) || v < -(1 << 23)) return false;
    return true;
}

// CABAC decode of every frame's network weights: host threads over the frames (each
// stream's weights are an independent few-hundred-symbol decode, ~50-100 us)
int decode_weights_all(std::vector<FramePlan> &fr)
{
    const int n = (int)fr.size();
    const int T = n >= 32 ? std::max(1, std::min({8, n / 16, (int)std::thread::hardware_concurrency()})) : 1;
    std::vector<int> rc(n, 0);
    std::vector<std::string> msg(n);
    auto work = [&](int t) {
        for (int i = t; i < n; i += T)
            if ((rc[i] = decode_frame_weights(fr[i].f)) != CCMI_OK) msg[i] = ccmi_last_error();
    };
    if (T == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
    }
    for (int i = 0; i < n; ++i)
        if (rc[i]) return ccmi_set_error(rc[i], "stream %d: %s", i, msg[i].c_str());
    return CCMI_OK;
}

// ARM + CABAC streams that share one launch: the non-empty latent grids of a chunk's frames
// with one (d, nh)
struct ArmGroup {
    int chunk, d, nh;
    std::vector<ArmStreamDesc> streams;
    size_t first; // index of streams[0] in the uploaded descriptor array
};

// frames of one chunk and one geometry that share one launch per tail stage
struct TailGroup {
    int chunk;
    std::vector<const DecTailFrame *> frames; // table order
    size_t off;                               // of the group's table, from DecodePlan::tail_off
    // ccmi_filter: the group's last n_flt frames take the stage; their tables, from DecodePlan::flt_tab_off
    int n_flt = 0;
    size_t flt_off = 0;
};

// State of one decode_run.  The host vectors are what the asynchronous uploads read.
struct Run {
    const DecodeRequest &rq;
    DecodePlan &pl;
    hipStream_t s;          // the caller's stream
    uint8_t *dev = nullptr; // workspace base
    int spin_cap = 0;
    int K = 1;              // chunks
    std::vector<int> chunk_of;
    std::vector<uint8_t> host; // the constant part
    std::vector<ArmGroup> arm;
    std::vector<ArmStreamDesc> descs; // every group's streams, in launch order
    int max_w = 0, max_blocks = 1;
    std::vector<TailGroup> tails;
    std::vector<uint8_t> tab; // the tail groups' tables, then the latent store's job table
    size_t tab_used = 0;      // bytes of `tab` to upload
    // latent store: a launch's part of the job table.  Sink: one per chunk, then the copy of the
    // networks' integers; source: one unpack per storage type among the frames' streams.
    struct LatLaunch {
        size_t first;
        int n;
        uint32_t blocks;
        int type; // CCMI_LATENT_*
    };
    std::vector<LatLaunch> lat;
    size_t lat_tab() const { return pl.lat_tab_off - pl.tail_off; } // of the job table in `tab`
    size_t flt_tab() const { return pl.flt_tab_off - pl.tail_off; } // of the filter stage's tables in `tab`
    size_t mix_tab() const { return pl.mix_tab_off - pl.tail_off; } // of the mix table in `tab`
    size_t blend_tab() const { return pl.blend_tab_off - pl.tail_off; } // of the blend table in `tab`
    uint32_t *status() const { return reinterpret_cast<uint32_t *>(dev + pl.status_off); }
};

// the decoded weights' 24-bit facts, and the host image of the constant part
void stage_constants(Run &r)
{
    r.host.assign(r.pl.cst, 0);
    for (FramePlan &p : r.pl.fr) {
        const FrameHost &f = p.f;
        p.arm24 = arm_weights_fit24(f);
        p.tail.syn.f24 = syn_weights_fit24(f) ? 1 : 0;
        for (int l = 0; l < f.n_layers; ++l)
            if (f.lat_n[l]) memcpy(&r.host[p.bytes_off[l]], f.lat_bytes[l], f.lat_n[l]);
        memcpy(&r.host[p.arm_off], f.arm.data(), f.arm.size() * 4);
        memcpy(&r.host[p.ups_off], f.ups.data(), f.ups.size() * 4);
        memcpy(&r.host[p.syn_off], f.syn.data(), f.syn.size() * 4);
    }
}

// Frames in K chunks by decode cost (coded bytes of their latent layers), cheapest first.
// Each chunk's ARM launch and decoder tail run on a stream of their own, so the tails of the
// early chunks overlap the long ARM chains of the later ones: a batch's ARM stage is the
// slowest layer-0 chain, and most CUs sit idle once the short streams are done.
// K = 2: the caller's stream and one more (GPU_MAX_HW_QUEUES is 4 per process; streams
// beyond the hardware queues share one and serialise)
#ifndef CCMI_DEC_CHUNKS
#define CCMI_DEC_CHUNKS 2
#endif
void assign_chunks(Run &r)
{
    const std::vector<FramePlan> &fr = r.pl.fr;
    const int n = (int)fr.size();
    r.K = n >= 64 && !r.rq.src ? CCMI_DEC_CHUNKS : 1; // a render has no ARM chain to hide a tail under
    r.chunk_of.assign(n, 0);
    if (r.K == 1) return;
    std::vector<int> order(n);
    std::vector<size_t> cost(n, 0);
    for (int i = 0; i < n; ++i) {
        order[i] = i;
        for (int l = 0; l < fr[i].f.n_layers; ++l) cost[i] += fr[i].f.lat_n[l];
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] < cost[b]; });
    for (int k = 0; k < n; ++k) r.chunk_of[order[k]] = (int)((int64_t)k * r.K / n);
}

// ARM + CABAC: every non-empty latent layer of every frame, one launch per (chunk, d, nh);
// zero layers are cleared here.  Uploads the descriptors in launch order.
int build_arm_groups(Run &r)
{
    for (size_t i = 0; i < r.pl.fr.size(); ++i) {
        const FramePlan &p = r.pl.fr[i];
        const FrameHost &f = p.f;
        int32_t *lat = reinterpret_cast<int32_t *>(r.dev + p.lat_off);
        for (int l = 0; l < f.n_layers; ++l) {
            int32_t *plane = lat + p.tail.ups.off[l]; // the planes follow one another (a store build pads them to 16 bytes)
            const int rows = p.tail.roi.arm_rows[l]; // == lh[l] unless a region decode stops early
            if (f.lat_n[l] == 0) { // zero layer (cc-frame-decoder.cpp:479-484)
                CCMI_HIP_CHECK(hipMemsetAsync(plane, 0, (size_t)rows * f.lw[l] * 4, r.s));
                continue;
            }
            ArmStreamDesc a{};
            a.bytes = reinterpret_cast<const uint32_t *>(r.dev + p.bytes_off[l]);
            a.nbytes = f.lat_n[l];
            a.h = f.lh[l];
            a.rows = rows;
            a.w = f.lw[l];
            a.sig_blk = f.sig_blk;
            a.d = f.dim_arm;
            a.nh = f.n_hidden;
            a.weights = reinterpret_cast<const int32_t *>(r.dev + p.arm_off);
            a.flags = p.arm24 ? 1 : 0;
            a.dbg = nullptr;
            a.status = r.status() + i * CCMI_MAX_GRIDS + l;
            a.spin_cap = r.spin_cap;
#if defined(CCMI_ARM_STAMPS)
            size_t made = 0;
            for (const ArmGroup &g : r.arm) made += g.streams.size();
            a.dbg = reinterpret_cast<uint64_t *>(r.dev + r.pl.dbg_off) + 16 * made;
#endif
            a.out = plane;
            r.max_w = std::max(r.max_w, a.w);
            const int blk = std::abs(a.sig_blk);
            if (blk > 0) {
                int sh = 0;
                while ((1 << sh) < blk) ++sh;
                r.max_blocks = std::max(r.max_blocks, ((a.h + blk - 1) >> sh) * ((a.w + blk - 1) >> sh));
            }
            const int c = r.chunk_of[i];
            auto it = std::find_if(r.arm.begin(), r.arm.end(),
                                   [&](const ArmGroup &g) { return g.chunk == c && g.d == a.d && g.nh == a.nh; });
            if (it == r.arm.end()) {
                r.arm.push_back(ArmGroup{c, a.d, a.nh, {}, 0});
                it = r.arm.end() - 1;
            }
            it->streams.push_back(a);
        }
    }
    std::stable_sort(r.arm.begin(), r.arm.end(), [](const ArmGroup &x, const ArmGroup &y) { return x.chunk < y.chunk; });
    for (ArmGroup &g : r.arm) {
        // longest streams first: they bound the launch
        std::stable_sort(g.streams.begin(), g.streams.end(),
                         [](const ArmStreamDesc &x, const ArmStreamDesc &y) { return x.rows * x.w > y.rows * y.w; });
        g.first = r.descs.size();
        r.descs.insert(r.descs.end(), g.streams.begin(), g.streams.end());
    }
    if (!r.descs.empty())
        CCMI_HIP_CHECK(hipMemcpyAsync(r.dev + r.pl.desc_off, r.descs.data(), r.descs.size() * sizeof(ArmStreamDesc),
                                      hipMemcpyHostToDevice, r.s));
    return CCMI_OK;
}

// Decoder tail: every frame's device pointers; frames of one geometry with a fused synthesis
// (single branch) share one launch per stage (960 class-E frames: 134 ms against 264 ms with
// per-frame launches).  Fills and uploads the groups' argument tables.
int build_tail_groups(Run &r)
{
    for (size_t i = 0; i < r.pl.fr.size(); ++i) {
        FramePlan &p = r.pl.fr[i];
        DecTailFrame &t = p.tail;
        t.ups.lat = reinterpret_cast<const int32_t *>(r.dev + p.lat_off);
        t.ups.kernels = reinterpret_cast<const int32_t *>(r.dev + p.ups_off);
        t.syn.params = reinterpret_cast<const int32_t *>(r.dev + p.syn_off);
        if (r.rq.src) { // the networks' integers stay in the store
            const LatentStream &S = r.rq.src->s[p.src];
            t.ups.kernels = reinterpret_cast<const int32_t *>(S.base + S.ups_off);
            t.syn.params = reinterpret_cast<const int32_t *>(S.base + S.syn_off);
        }
        t.ups.workspace = reinterpret_cast<int32_t *>(r.dev + p.ws_off);
        t.ups.out = reinterpret_cast<int32_t *>(r.dev + p.dense_off);
        t.syn.in = t.ups.out;
        t.syn.out = reinterpret_cast<int32_t *>(r.dev + p.synout_off);
        t.syn.workspace = reinterpret_cast<int32_t *>(r.dev + p.synws_off);
        t.dst = r.rq.device() ? static_cast<uint8_t *>(r.rq.dev[i]) : r.dev + p.out_off;
        // ccmi_blend: whatever out_dev holds for a silent frame is not looked at.  No tail kernel writes a
        // mix-staged frame's dst, and its table entry gets none (dec_blend_fill): the staging frame stands in
        if (p.silent) t.dst = r.dev + p.flt_off;
        t.rs_tmp = p.rs_elems ? reinterpret_cast<float *>(r.dev + p.rs_off) : nullptr;
        if (t.fmt.col && r.pl.cols[i].contrast >= 0)
            r.pl.cols[i].acc = reinterpret_cast<unsigned long long *>(r.dev + r.pl.col_off) + i;
        t.flt_tmp = p.flt_elems ? reinterpret_cast<float *>(r.dev + p.flt_off) : nullptr;
        if (t.tone) { // the device pointers of the frame's tone entry, before the tables are filled
            DecTone &e = r.pl.tones[i];
            e.buf[0] = t.flt_tmp;
            e.buf[1] = p.tone2_off ? reinterpret_cast<float *>(r.dev + p.tone2_off) : nullptr;
            e.acc = dec_tone_stats(e) ? r.dev + p.tone_acc_off : nullptr;
        }
        t.mix_buf = p.mix2_off ? reinterpret_cast<float *>(r.dev + p.mix2_off) : nullptr;
        if (!p.batchable) continue;
        const int c = r.chunk_of[i];
        auto it = std::find_if(r.tails.begin(), r.tails.end(), [&](const TailGroup &g) {
            return g.frames.size() < 65535 && g.chunk == c && dec_tail_same_group(*g.frames[0], t);
        });
        if (it == r.tails.end()) {
            r.tails.push_back(TailGroup{c, {}, 0});
            it = r.tails.end() - 1;
        }
        it->frames.push_back(&t);
    }
    if (r.tab.size() < r.pl.tail_cap + 1) r.tab.resize(r.pl.tail_cap + 1);
    size_t tpos = 0, fpos = 0;
    for (TailGroup &g : r.tails) {
        const int m = (int)g.frames.size();
        g.off = tpos;
        if (r.pl.n_flt) { // the frames that take the filter stage last, in their order: they run as their own launches
            auto staged = std::stable_partition(g.frames.begin(), g.frames.end(), [](const DecTailFrame *f) { return !f->flt; });
            g.n_flt = (int)(g.frames.end() - staged);
            if (r.pl.n_mix) // ... and among them the mix-staged ones last (dec_flt_class)
                std::stable_sort(staged, g.frames.end(),
                                 [](const DecTailFrame *a, const DecTailFrame *b) { return dec_flt_class(*a) < dec_flt_class(*b); });
            g.flt_off = fpos;
            fpos += dec_flt_table_bytes(!r.pl.tones.empty()) * (size_t)g.n_flt;
        }
        dec_tail_fill(g.frames.data(), m, r.tab.data() + tpos, g.n_flt, r.tab.data() + r.flt_tab() + g.flt_off);
        tpos += dec_tail_table_bytes(g.frames[0]->ups.n_layers, m, g.frames[0]->windowed, dec_out_form(g.frames[0]->fmt),
                                     g.frames[0]->fmt.col != 0);
    }
    r.tab_used = tpos;
    return CCMI_OK;
}

// ccmi_mix: the entries of the mix-staged frames, once every frame has its device pointers
void build_mix_table(Run &r, int &max_oh, int &max_ow)
{
    max_oh = max_ow = 0;
    for (const FramePlan &p : r.pl.fr) {
        const DecTailFrame &t = p.tail;
        if (!t.mix) continue;
        const bool sized = t.fmt.rs || t.fmt.warp;
        const int oh = sized ? t.fmt.out_h : t.roi.rect.h(), ow = sized ? t.fmt.out_w : t.roi.rect.w();
        dec_mix_fill(r.tab.data() + r.mix_tab(), t, oh, ow, t.mix->partner >= 0 ? r.pl.mixes[t.mix->partner].entry : -1);
        max_oh = std::max(max_oh, oh), max_ow = std::max(max_ow, ow);
    }
    for (size_t i = 0; i < r.pl.blends.size(); ++i) { // ccmi_blend: the terms, by the sources' entries
        const DecBlend &b = r.pl.blends[i];
        if (!b.count && !b.silent) continue;
        int src[CCMI_BLEND_MAX_TERMS] = {};
        for (int t = 0; t < b.count; ++t) src[t] = r.pl.mixes[b.src[t]].entry;
        dec_blend_fill(r.tab.data() + r.mix_tab(), r.tab.data() + r.blend_tab(), r.pl.mixes[i].entry, b, src);
    }
}

// Latent-store sink: a pack job per non-empty grid, chunk by chunk, then two copy jobs per
// stream for the upsampling and synthesis integers (from the uploaded constant part).
void build_pack_jobs(Run &r)
{
    const ccmi_latents &h = *r.rq.lat_store;
    uint8_t *store = const_cast<uint8_t *>(h.s[0].base); // a build has one store and one type
    const int type = h.s[0].type;
    DecLatPackJob *jobs = reinterpret_cast<DecLatPackJob *>(r.tab.data() + r.lat_tab());
    size_t nj = 0;
    for (int c = 0; c < r.K; ++c) {
        Run::LatLaunch L{nj, 0, 0, type};
        for (size_t i = 0; i < r.pl.fr.size(); ++i) {
            if (r.chunk_of[i] != c) continue;
            const FramePlan &p = r.pl.fr[i];
            for (int l = 0; l < p.f.n_layers; ++l) {
                if (p.f.lat_n[l] == 0) continue;
                const uint32_t n = (uint32_t)p.f.lh[l] * (uint32_t)p.f.lw[l];
                jobs[nj++] = DecLatPackJob{reinterpret_cast<const int32_t *>(r.dev + p.lat_off) + p.tail.ups.off[l],
                                           store + h.s[i].grid_off[l],
                                           r.status() + i * CCMI_MAX_GRIDS + l,
                                           n,
                                           L.blocks,
                                           kArmPrec,
                                           0};
                L.blocks += dec_lat_pack_blocks(n, type);
                ++L.n;
            }
        }
        r.lat.push_back(L);
    }
    Run::LatLaunch N{nj, 0, 0, CCMI_LATENT_I32};
    for (size_t i = 0; i < r.pl.fr.size(); ++i) {
        const FramePlan &p = r.pl.fr[i];
        const size_t src[2] = {p.ups_off, p.syn_off}, dst[2] = {h.s[i].ups_off, h.s[i].syn_off};
        const size_t cnt[2] = {p.f.ups.size(), p.f.syn.size()};
        for (int k = 0; k < 2; ++k) {
            if (!cnt[k]) continue;
            jobs[nj++] = DecLatPackJob{reinterpret_cast<const int32_t *>(r.dev + src[k]), store + dst[k], nullptr,
                                       (uint32_t)cnt[k], N.blocks, 0, 0};
            N.blocks += dec_lat_pack_blocks((uint32_t)cnt[k], CCMI_LATENT_I32);
            ++N.n;
        }
    }
    r.lat.push_back(N);
    r.tab_used = r.lat_tab() + nj * sizeof(DecLatPackJob);
}

// Latent-store source: an unpack job per grid of every output frame, over the rectangle of
// the plane the frame's tail reads (whole planes unless the tail runs on windows).  The jobs of
// one storage type follow each other and share a launch: a handle over stores of several types
// (ccmi_latents_concat) costs one launch per type present, whatever the order of the frames.
void build_unpack_jobs(Run &r)
{
    const ccmi_latents &h = *r.rq.src;
    DecLatUnpackJob *jobs = reinterpret_cast<DecLatUnpackJob *>(r.tab.data() + r.lat_tab());
    size_t nj = 0;
    for (int type = CCMI_LATENT_I8; type <= CCMI_LATENT_SEG; ++type) {
        Run::LatLaunch L{nj, 0, 0, type};
        for (const FramePlan &p : r.pl.fr) {
            const LatentStream &S = h.s[p.src];
            if (S.type != type) continue;
            for (int l = 0; l < p.f.n_layers; ++l) {
                const DecWindow &w = p.tail.roi.lat[l];
                const uint32_t blocks = dec_lat_unpack_blocks(w);
                if (!blocks) continue;
                jobs[nj++] = DecLatUnpackJob{p.f.lat_n[l] ? S.base + S.grid_off[l] : nullptr,
                                             reinterpret_cast<int32_t *>(r.dev + p.lat_off) + p.tail.ups.off[l],
                                             p.f.lw[l], w.y0, w.y1, w.x0, w.x1, L.blocks, kArmPrec, p.f.lh[l]};
                L.blocks += blocks;
                ++L.n;
            }
        }
        if (L.n) r.lat.push_back(L);
    }
    r.tab_used = r.lat_tab() + nj * sizeof(DecLatUnpackJob);
}

int launch_lat(const Run &r, const Run::LatLaunch &L, hipStream_t cs)
{
    const uint8_t *tab = r.dev + r.pl.lat_tab_off;
    if (r.rq.src)
        return launch_dec_lat_unpack(reinterpret_cast<const DecLatUnpackJob *>(tab) + L.first, L.n, L.blocks, L.type, cs);
    return launch_dec_lat_pack(reinterpret_cast<const DecLatPackJob *>(tab) + L.first, L.n, L.blocks, L.type, cs);
}

// the per-frame tail of a frame the batched tail does not take: pyramid, synthesis per
// branch with the blend, output
int launch_frame_tail(const Run &r, const FramePlan &p, hipStream_t cs)
{
    const FrameHost &f = p.f;
    const DecTailFrame &t = p.tail;
    if (int rc = launch_dec_ups(t.ups, cs)) return rc;
    const int nout = f.layers.back().n_out;
    const int64_t plane = (int64_t)f.h * f.w;
    const size_t per_branch = f.syn.size() / f.n_branches;
    int32_t *synout = t.syn.out;
    for (int b = 0; b < f.n_branches; ++b) {
        DecSynArgs sa = t.syn;
        sa.params += per_branch * b;
        sa.out = synout + (size_t)b * nout * plane;
        if (int rc = launch_dec_syn(sa, cs)) return rc;
        if (b >= 1) // run_syn (cc-frame-decoder.cpp:1044-1149): blends on 3 planes
            if (int rc = launch_dec_blend(synout, synout + (size_t)b * nout * plane, 3 * plane, f.blend[0], f.blend[b],
                                          b == 1, cs))
                return rc;
    }
    if (t.flt) return launch_dec_out_frame_flt(t, synout, f.h, f.w, cs); // staged, then the filter kernel
    return launch_dec_out_frame(t, synout, f.h, f.w, p.mode == kTailCrop, r.rq.device(), cs);
}

// one chunk's ARM launches, then its decoder tail (batched groups, then the rest per frame)
int launch_chunk(const Run &r, int c, hipStream_t cs, hipEvent_t arm_done)
{
    const ArmStreamDesc *descs = reinterpret_cast<const ArmStreamDesc *>(r.dev + r.pl.desc_off);
    for (const ArmGroup &g : r.arm)
        if (g.chunk == c)
            if (int rc = launch_dec_arm(descs + g.first, (int)g.streams.size(), r.max_w, r.max_blocks, g.d, g.nh, cs))
                return rc;
    // a render's planes come from the store: the unpack stands where the ARM stage does
    if (r.rq.src)
        for (const Run::LatLaunch &L : r.lat)
            if (int rc = launch_lat(r, L, cs)) return rc;
    if (arm_done) CCMI_HIP_CHECK(hipEventRecord(arm_done, cs));
    if (r.rq.lat_store) // a store build has no tail: the chunk's planes are packed instead
        return launch_lat(r, r.lat[c], cs);
    for (const TailGroup &g : r.tails)
        if (g.chunk == c)
            if (int rc = launch_dec_tail_batch(g.frames.data(), (int)g.frames.size(), r.dev + r.pl.tail_off + g.off, cs,
                                               g.n_flt, r.dev + r.pl.flt_tab_off + g.flt_off))
                return rc;
    for (size_t i = 0; i < r.pl.fr.size(); ++i)
        if (!r.pl.fr[i].batchable && r.chunk_of[i] == c)
            if (int rc = launch_frame_tail(r, r.pl.fr[i], cs)) return rc;
    return CCMI_OK;
}

// The decoded bytes of chunk c: headers on the host, payloads copied back on the chunk's
// own stream right after its tail, so one chunk's download overlaps the other chunk's
// ARM chains (pinned output buffers make these real DMA copies; pageable ones are staged
// by the runtime).  A device sink has nothing to download: its frames are where they belong.
int download_chunk(const Run &r, int c, hipStream_t cs)
{
    if (!r.rq.outs || r.rq.device()) return CCMI_OK;
    for (size_t i = 0; i < r.pl.fr.size(); ++i) {
        if (r.chunk_of[i] != c) continue;
        const FramePlan &p = r.pl.fr[i];
        if (p.of.header) memcpy(r.rq.outs[i], p.of.hdr, p.of.header);
        CCMI_HIP_CHECK(hipMemcpyAsync(r.rq.outs[i] + p.of.header, r.dev + p.out_off, p.of.payload, hipMemcpyDeviceToHost, cs));
    }
    return CCMI_OK;
}

// A chunk's events: its start (recorded here only when the chunk streams were forked), ARM
// done, tail done, and done (what the caller's stream waits for, chunks >= 1).  One chunk:
// the call's own events, on the caller's stream between [1] uploads done and [4] all done.
// Forked: the lease's events, [0] fork, then four per chunk.
struct ChunkEvents {
    hipEvent_t start, arm_done, tail_done, done;
};

ChunkEvents chunk_events(const EventSet &ev, const StreamSet *fk, int c)
{
    if (fk) return ChunkEvents{fk->ev[1 + 4 * c], fk->ev[2 + 4 * c], fk->ev[3 + 4 * c], fk->ev[4 + 4 * c]};
    if (!ev.ok) return ChunkEvents{};
    return ChunkEvents{nullptr, ev.e[2], ev.e[3], nullptr};
}

// The caller's stream waits for the `started` forked chunks (K-1 downwards).  Also the way
// out of an error after some chunks were queued: s waits for them before the caller can
// reuse or free the workspace (the chunks' own streams never outlive it unjoined).
void join_chunks(const Run &r, const EventSet &ev, const StreamSet *fk, int started)
{
    for (int c = r.K - 1; c > r.K - 1 - started && c >= 1; --c) {
        const ChunkEvents e = chunk_events(ev, fk, c);
        (void)hipEventRecord(e.done, fk->st[c]);
        (void)hipStreamWaitEvent(r.s, e.done, 0);
    }
}

// Every chunk's ARM -> tail -> download, the most expensive chunk first.  Chunk 0 runs on the
// caller's stream; chunks >= 1 on streams forked from it after the uploads, leased with their
// events from the process-wide pool (ccmi_api.cpp) for this call.  One chunk: no lease, no fork.
int run_chunks(const Run &r, const EventSet &ev, StreamSetLease &lease)
{
    const StreamSet *fk = nullptr;
    if (r.K > 1) {
        lease.set = ccmi_streamset_acquire(r.K, 1 + 4 * r.K, true);
        if (!lease.set) return CCMI_ERR_HIP;
        fk = lease.set;
        CCMI_HIP_CHECK(hipEventRecord(fk->ev[0], r.s));
    }
    int started = 0;
    for (int c = r.K - 1; c >= 0; --c) {
        const hipStream_t cs = c == 0 ? r.s : fk->st[c];
        const ChunkEvents e = chunk_events(ev, fk, c);
        if (c > 0) {
            if (hipStreamWaitEvent(cs, fk->ev[0], 0) != hipSuccess) {
                join_chunks(r, ev, fk, started);
                return ccmi_set_error(CCMI_ERR_HIP, "decode: stream fork failed");
            }
            ++started;
        }
        if (e.start) (void)hipEventRecord(e.start, cs);
        int rc = launch_chunk(r, c, cs, e.arm_done);
        if (!rc) {
            if (e.tail_done) (void)hipEventRecord(e.tail_done, cs);
            rc = download_chunk(r, c, cs);
        }
        if (rc) {
            join_chunks(r, ev, fk, started);
            return rc;
        }
    }
    join_chunks(r, ev, fk, started);
    return CCMI_OK;
}

// latents (when asked for) and the ARM kernels' status words, then the one synchronisation
int read_back(const Run &r)
{
    const DecodePlan &pl = r.pl;
    const int n = (int)pl.fr.size();
    if (r.rq.src) { // no ARM ran: no status words, and the flag record stays empty
        CCMI_HIP_CHECK(hipStreamSynchronize(r.s));
        return CCMI_OK;
    }
    int32_t *const *lat_out = r.rq.lat_out;
    for (int i = 0; i < n && lat_out; ++i)
        CCMI_HIP_CHECK(hipMemcpyAsync(lat_out[i], r.dev + pl.fr[i].lat_off, pl.fr[i].lat_elems * 4, hipMemcpyDeviceToHost, r.s));
    std::vector<uint32_t> st(pl.n_status());
    CCMI_HIP_CHECK(hipMemcpyAsync(st.data(), r.status(), 4 * st.size(), hipMemcpyDeviceToHost, r.s));
    CCMI_HIP_CHECK(hipStreamSynchronize(r.s));
    g_last_flags.assign(n, 0u);
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < CCMI_MAX_GRIDS; ++l) g_last_flags[i] |= st[(size_t)i * CCMI_MAX_GRIDS + l];
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < CCMI_MAX_GRIDS; ++l)
            if (st[(size_t)i * CCMI_MAX_GRIDS + l] & CCMI_ARM_FLAG_TIMEOUT)
                // the two waves of a stream lost their hand-off: the latents cannot be trusted
                return ccmi_set_error(CCMI_ERR_HIP,
                                      "decode: stream %d, latent grid %d: the ARM decode's wave hand-off gave up "
                                      "after %d polls; output discarded",
                                      i, l, r.spin_cap);
    for (int i = 0; i < n && r.rq.lat_store; ++i)
        for (int l = 0; l < CCMI_MAX_GRIDS; ++l)
            if (st[(size_t)i * CCMI_MAX_GRIDS + l] & CCMI_ARM_FLAG_NARROW) {
                static const char *const kName[] = {"int8", "int16", "int32"};
                return ccmi_set_error(CCMI_ERR_UNSUPPORTED,
                                      "latents: stream %d, latent grid %d: a latent does not fit %s; build the store "
                                      "with a wider element type",
                                      i, l, kName[r.rq.lat_store->s[0].type]);
            }
    for (int i = 0; i < n && lat_out; ++i)
        for (size_t k = 0; k < pl.fr[i].lat_elems; ++k) lat_out[i][k] >>= kArmPrec;
#if defined(CCMI_ARM_STAMPS)
    {
        std::vector<uint64_t> dbg(16 * r.descs.size());
        CCMI_HIP_CHECK(hipMemcpy(dbg.data(), r.dev + pl.dbg_off, dbg.size() * 8, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < r.descs.size(); ++j) {
            const size_t k = (size_t)(reinterpret_cast<uint8_t *>(r.descs[j].dbg) - (r.dev + pl.dbg_off)) / 128;
            fprintf(stderr, "STAMPS stream %zu (%dx%d):", k, r.descs[j].h, r.descs[j].w);
            for (int c = 0; c < 16; ++c) fprintf(stderr, " %llu", (unsigned long long)dbg[16 * k + c]);
            fprintf(stderr, "\n");
        }
    }
#endif
    return CCMI_OK;
}

// ccmi_decode_last_timing: upload, ARM, tail, download
void store_timing(const Run &r, const EventSet &ev, const StreamSet *fk)
{
    if (!ev.ok) return;
    if (!fk) {
        for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&g_last_ms[k], ev.e[k], ev.e[k + 1]);
    } else {
        // overlapped stages: ARM = the longest chunk's ARM (its start to its ARM end, events
        // of one stream), tail = from the uploads to the last chunk's tail minus that ARM,
        // download = what is left after the last tail (the part not hidden under kernels)
        float span = 0.f, arm = 0.f, all = 0.f;
        (void)hipEventElapsedTime(&g_last_ms[0], ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&all, ev.e[1], ev.e[4]);
        for (int c = 0; c < r.K; ++c) {
            const ChunkEvents e = chunk_events(ev, fk, c);
            float t = 0.f;
            if (hipEventElapsedTime(&t, e.start, e.arm_done) == hipSuccess) arm = std::max(arm, t);
            if (hipEventElapsedTime(&t, ev.e[1], e.tail_done) == hipSuccess) span = std::max(span, t);
        }
        // ccmi_mix: the call's one mix launch runs on the caller's stream after the join and ends the tail
        float t = 0.f;
        if (r.pl.n_mix && hipEventElapsedTime(&t, ev.e[1], ev.e[3]) == hipSuccess) span = std::max(span, t);
        g_last_ms[1] = arm;
        g_last_ms[2] = span - arm;
        g_last_ms[3] = all - span;
        (void)hipGetLastError(); // a timing query that failed must not surface in the next call
    }
    if (r.rq.device()) g_last_ms[3] = 0.f; // nothing was downloaded (the status words are not frame data)
}

// Executes a plan on stream s: weight decode, uploads, launches, downloads, status words.
int decode_run(const DecodeRequest &rq, DecodePlan &pl, hipStream_t s)
{
    Run r{rq, pl, s};
    const bool render = rq.src != nullptr;
    if (!render) { // a render takes the decoded networks and their 24-bit facts from the handle
        if (int rc = decode_weights_all(pl.fr)) return rc;
        stage_constants(r);
    }
    r.dev = static_cast<uint8_t *>(rq.ws);
    if (r.dev) {
        if (rq.ws_bytes < pl.total)
            return ccmi_set_error(CCMI_ERR_ARG, "decode: workspace of %zu bytes, need %zu", rq.ws_bytes, pl.total);
        if (reinterpret_cast<uintptr_t>(r.dev) % 256)
            return ccmi_set_error(CCMI_ERR_ARG, "decode: workspace must be 256-byte aligned");
    } else {
        CCMI_HIP_CHECK(hipMalloc(&r.dev, pl.total));
    }
    struct Free {
        uint8_t *p;
        ~Free() { if (p) (void)hipFree(p); }
    } guard{rq.ws ? nullptr : r.dev};
    EventSet ev;
    StreamSetLease lease;
    ev.rec(0, s);
    if (!render) {
        CCMI_HIP_CHECK(hipMemcpyAsync(r.dev, r.host.data(), pl.cst, hipMemcpyHostToDevice, s));
        CCMI_HIP_CHECK(hipMemsetAsync(r.status(), 0, 4 * pl.n_status(), s));
    }
    r.spin_cap = arm_spin_cap();
    assign_chunks(r);
    if (!render)
        if (int rc = build_arm_groups(r)) return rc;
    // the tables of the call: the tail groups', then the latent store's jobs, in one copy
    r.tab.assign(std::max(r.lat_tab() + pl.lat_tab_cap, r.blend_tab() + pl.blend_table_bytes()) + 1, 0);
    if (!rq.lat_store)
        if (int rc = build_tail_groups(r)) return rc;
    if (rq.lat_store) build_pack_jobs(r);
    if (render) build_unpack_jobs(r);
    if (pl.n_flt) r.tab_used = r.flt_tab() + pl.flt_table_bytes(); // the filter stage's tables end the image ...
    int mix_oh = 0, mix_ow = 0;
    if (pl.n_mix) { // ... or the mix table after them
        build_mix_table(r, mix_oh, mix_ow);
        r.tab_used = r.blend_tab() + pl.blend_table_bytes(); // ... and the blend table after it
    }
    if (r.tab_used)
        CCMI_HIP_CHECK(hipMemcpyAsync(r.dev + pl.tail_off, r.tab.data(), r.tab_used, hipMemcpyHostToDevice, s));
    if (rq.lat_store) // the networks' integers: constant part -> store, before the chunks fork
        if (int rc = launch_lat(r, r.lat[r.K], s)) return rc;
    if (pl.col_stat) // the contrast ops' accumulators, cleared in stream before any chunk's statistics pass
        CCMI_HIP_CHECK(hipMemsetAsync(r.dev + pl.col_off, 0, sizeof(unsigned long long) * pl.fr.size(), s));
    if (pl.tone_acc_bytes) // the tone stage's accumulator blocks likewise (the minima are kept complemented)
        CCMI_HIP_CHECK(hipMemsetAsync(r.dev + pl.tone_acc_off, 0, pl.tone_acc_bytes, s));
    ev.rec(1, s);
    if (int rc = run_chunks(r, ev, lease)) return rc;
    if (pl.n_mix) { // every chunk is joined: a partner may sit in any chunk, tail group or per-frame tail
        const FramePlan *m0 = nullptr;
        for (const FramePlan &p : pl.fr)
            if (p.tail.mix && !m0) m0 = &p;
        if (int rc = pl.blends.empty() ? launch_dec_mix(r.dev + pl.mix_tab_off, pl.n_mix, mix_oh, mix_ow, m0->tail.fmt, s)
                                       : launch_dec_blend(r.dev + pl.mix_tab_off, r.dev + pl.blend_tab_off, pl.n_mix, mix_oh,
                                                          mix_ow, m0->tail.fmt, s))
            return rc;
        ev.rec(3, s); // the mix launch ends the tail (store_timing; forked chunks record their own tail ends)
    }
    if (!rq.lat_store) { // what launch_chunk ran: every group, and a tail of its own per other frame
        g_last_tails[0] = (int)r.tails.size();
        for (const FramePlan &p : pl.fr) g_last_tails[1] += p.batchable ? 0 : 1;
    }
    ev.rec(4, s);
    if (int rc = read_back(r)) return rc;
    store_timing(r, ev, lease.set);
    return CCMI_OK;
}

// The thread-local ARM flags are cleared first: a call that fails, or only plans, reports no
// stream, not the previous call's.
int plan_only(const DecodeRequest &rq, size_t *workspace_bytes)
{
    clear_last();
    DecodePlan pl;
    if (int rc = decode_plan(rq, pl)) return rc;
    *workspace_bytes = pl.total;
    return CCMI_OK;
}

int decode_many(const DecodeRequest &rq, void *stream)
{
    clear_last();
    DecodePlan pl;
    if (int rc = decode_plan(rq, pl)) return rc;
    return decode_run(rq, pl, static_cast<hipStream_t>(stream));
}

DecodeRequest request(const uint8_t *const *streams, const size_t *lens, int n, int out_bitdepth, int out_chroma)
{
    DecodeRequest rq;
    rq.streams = streams;
    rq.lens = lens;
    rq.n = n;
    rq.out_bitdepth = out_bitdepth;
    rq.out_chroma = out_chroma;
    return rq;
}

} // namespace

extern "C" int ccmi_decode_last_timing(float *ms4)
{
    if (!ms4) return ccmi_set_error(CCMI_ERR_ARG, "decode_last_timing: null argument");
    for (int k = 0; k < 4; ++k) ms4[k] = g_last_ms[k];
    return CCMI_OK;
}

extern "C" int ccmi_decode_last_arm_flags(uint32_t *flags, int cap, int *n)
{
    if (!n || (cap > 0 && !flags)) return ccmi_set_error(CCMI_ERR_ARG, "decode_last_arm_flags: null argument");
    const int m = std::min(cap, (int)g_last_flags.size());
    for (int i = 0; i < m; ++i) flags[i] = g_last_flags[i];
    *n = (int)g_last_flags.size();
    return CCMI_OK;
}

extern "C" int ccmi_decode_output_size(const uint8_t *stream, size_t len, int out_bitdepth, int out_chroma, int as_yuv,
                                       size_t *size)
{
    if (!stream || !size) return ccmi_set_error(CCMI_ERR_ARG, "decode_output_size: null argument");
    FrameHost f;
    if (int rc = parse_frame_header(stream, len, f)) return rc;
    OutFmt o;
    if (int rc = out_format(f, out_bitdepth, out_chroma, as_yuv, o)) return rc;
    *size = o.header + o.payload;
    return CCMI_OK;
}

extern "C" int ccmi_decode_batch(const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *out,
                                 const size_t *out_caps, size_t *out_sizes, int out_bitdepth, int out_chroma,
                                 int as_yuv, void *stream)
{
    if (!streams || !lens || !out || !out_caps) return ccmi_set_error(CCMI_ERR_ARG, "decode_batch: null argument");
    DecodeRequest rq = request(streams, lens, n, out_bitdepth, out_chroma);
    rq.as_yuv = as_yuv;
    rq.outs = out;
    rq.caps = out_caps;
    rq.sizes = out_sizes;
    return decode_many(rq, stream);
}

extern "C" int ccmi_decode_batch_workspace_bytes(const uint8_t *const *streams, const size_t *lens, int n,
                                                 int out_bitdepth, int out_chroma, int as_yuv, size_t *bytes)
{
    if (!streams || !lens || !bytes) return ccmi_set_error(CCMI_ERR_ARG, "decode_batch_workspace_bytes: null argument");
    DecodeRequest rq = request(streams, lens, n, out_bitdepth, out_chroma);
    rq.as_yuv = as_yuv;
    return plan_only(rq, bytes);
}

extern "C" int ccmi_decode_batch_plan(const uint8_t *const *streams, const size_t *lens, int n, int out_bitdepth,
                                      int out_chroma, int as_yuv, size_t *out_sizes, size_t *workspace_bytes)
{
    if (!streams || !lens || !out_sizes || !workspace_bytes) return ccmi_set_error(CCMI_ERR_ARG, "decode_batch_plan: null argument");
    DecodeRequest rq = request(streams, lens, n, out_bitdepth, out_chroma);
    rq.as_yuv = as_yuv;
    rq.sizes = out_sizes;
    return plan_only(rq, workspace_bytes);
}

extern "C" int ccmi_decode_batch_ws(const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *out,
                                    const size_t *out_caps, size_t *out_sizes, int out_bitdepth, int out_chroma,
                                    int as_yuv, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!streams || !lens || !out || !out_caps || !workspace)
        return ccmi_set_error(CCMI_ERR_ARG, "decode_batch_ws: null argument");
    DecodeRequest rq = request(streams, lens, n, out_bitdepth, out_chroma);
    rq.as_yuv = as_yuv;
    rq.outs = out;
    rq.caps = out_caps;
    rq.sizes = out_sizes;
    rq.ws = workspace;
    rq.ws_bytes = workspace_bytes;
    return decode_many(rq, stream);
}

// ------------------------------------------------------------------ device sinks
// Forty entry points over one table, each a Source, a Sink and one return through sink_plan or
// sink_run:
//   source  the caller's streams (ccmi_decode_batch_dev*)  |  a latent store (ccmi_latents_render*)
//   sink    plain samples of sample_type: whole frames, or regions (_roi; the store's call takes both)
//           formatted ones (fmt; forced to CCMI_SAMPLE_F32, the call whose output kernel the format
//           replaces): _fmt; _rs, with a resample; _warp, with a warp, which takes no region; then _col,
//           _flt, _tone, _mix and _blend, each the superset of all before it with one more stage (colour
//           ops, a filter, tone ops, a mix, a blend).  A stage that is NULL is the call before, itself, under
//           the name it was entered by; what may not go together is the plan's to refuse
//   form    a plan (geom, info, window, workspace_bytes)  |  a run (outputs, workspace, stream)
// `who` is the entry point's name for the error text, `needs` what it requires beyond the source and
// its own outputs: the _warp entry points a warp with its matrices, the supersets only the matrices
// of a warp that is there; a window without a warp is refused by whoever takes a window.
struct Source {
    const uint8_t *const *streams;
    const size_t *lens;
    const ccmi_latents *h;
    const int *index;
    int n;
    bool store;
};

static Source from_streams(const uint8_t *const *streams, const size_t *lens, int n)
{
    return Source{streams, lens, nullptr, nullptr, n, false};
}

static Source from_store(const ccmi_latents *h, const int *index, int m) { return Source{nullptr, nullptr, h, index, m, true}; }

struct Sink { // in the entry points' argument order; an entry point writes the members it has
    const ccmi_rect *roi = nullptr;
    int sample = CCMI_SAMPLE_F32;
    const ccmi_tensor_fmt *fmt = nullptr;
    const ccmi_resample *rs = nullptr;
    const ccmi_warp *warp = nullptr;
    const ccmi_colour *colour = nullptr;
    const ccmi_tone *tone = nullptr;
    const ccmi_filter *filter = nullptr;
    const ccmi_mix *mix = nullptr;
    const ccmi_blend *blend = nullptr; // the prototypes take it before mix
};

enum Needs { PLAIN, FMT, FMT_WARP };
constexpr int F32 = CCMI_SAMPLE_F32;

static bool absent(const Sink &k, Needs needs)
{
    if (needs == PLAIN) return false;
    return !k.fmt || (needs == FMT_WARP ? !k.warp || !k.warp->matrix : k.warp && !k.warp->matrix);
}

// streams: null arguments, then the sample type; a store: the handle and the sample type, then (a run)
// a plan-only handle, then null arguments; then, for both, the plan's own errors
static int sink_request(const char *who, const Source &src, const Sink &k, int out_bitdepth, int out_chroma, bool run,
                        bool missing, DecodeRequest &rq)
{
    clear_last();
    if (src.store && !src.h) return ccmi_set_error(CCMI_ERR_ARG, "render: the handle is NULL (no frame 0)");
    if (!src.store && (!src.streams || !src.lens || missing)) return ccmi_set_error(CCMI_ERR_ARG, "%s: null argument", who);
    if (k.sample < 0) return ccmi_set_error(CCMI_ERR_ARG, "decode: unknown sample type %d", k.sample);
    if (src.store && run && !src.h->resident)
        return ccmi_set_error(CCMI_ERR_ARG, "render: the handle is plan-only (built without a store): no frame 0 to render");
    if (missing) return ccmi_set_error(CCMI_ERR_ARG, "%s: null argument", who);
    rq = request(src.streams, src.lens, src.n, out_bitdepth, out_chroma);
    rq.src = src.h;
    rq.index = src.index;
    rq.sample = k.sample;
    rq.roi = k.roi;
    rq.fmt = k.fmt;
    rq.rs = k.rs;
    rq.warp = k.warp;
    rq.colour = k.colour;
    rq.filter = k.filter;
    rq.tone = k.tone;
    rq.mix = k.mix;
    rq.blend = k.blend;
    return CCMI_OK;
}

static int sink_plan(const char *who, const Source &src, const Sink &k, Needs needs, int out_bitdepth, int out_chroma,
                     ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window, size_t *workspace_bytes)
{
    DecodeRequest rq;
    if (int rc = sink_request(who, src, k, out_bitdepth, out_chroma, false,
                              absent(k, needs) || (window && !k.warp) || !geom || !workspace_bytes, rq))
        return rc;
    rq.geom = geom;
    rq.info = info;
    rq.window = window;
    return plan_only(rq, workspace_bytes);
}

static int sink_run(const char *who, const Source &src, const Sink &k, Needs needs, void *const *out_dev,
                    const size_t *out_caps, int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                    void *stream)
{
    DecodeRequest rq;
    if (int rc = sink_request(who, src, k, out_bitdepth, out_chroma, true, !out_dev || !out_caps || absent(k, needs), rq))
        return rc;
    rq.dev = out_dev;
    rq.caps = out_caps;
    rq.ws = workspace;
    rq.ws_bytes = workspace_bytes;
    return decode_many(rq, stream);
}

extern "C" int ccmi_decode_batch_dev_plan(const uint8_t *const *streams, const size_t *lens, int n, int out_bitdepth,
                                          int out_chroma, int sample_type, ccmi_frame_geom *geom,
                                          size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_plan", from_streams(streams, lens, n), Sink{nullptr, sample_type}, PLAIN, out_bitdepth,
                     out_chroma, geom, nullptr, nullptr, workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev(const uint8_t *const *streams, const size_t *lens, int n, void *const *out_dev,
                                     const size_t *out_caps, int sample_type, int out_bitdepth, int out_chroma,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("decode_batch_dev", from_streams(streams, lens, n), Sink{nullptr, sample_type}, PLAIN, out_dev, out_caps,
                    out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_roi_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                              const ccmi_rect *roi, int out_bitdepth, int out_chroma, int sample_type,
                                              ccmi_frame_geom *geom, ccmi_roi_info *info, size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_roi_plan", from_streams(streams, lens, n), Sink{roi, sample_type}, PLAIN, out_bitdepth,
                     out_chroma, geom, info, nullptr, workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_roi(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                         void *const *out_dev, const size_t *out_caps, int sample_type,
                                         int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return sink_run("decode_batch_dev_roi", from_streams(streams, lens, n), Sink{roi, sample_type}, PLAIN, out_dev, out_caps,
                    out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_rs_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                             const ccmi_rect *roi, int out_bitdepth, int out_chroma,
                                             const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, ccmi_frame_geom *geom,
                                             ccmi_roi_info *info, size_t *workspace_bytes)
{
    return sink_plan(rs ? "decode_batch_dev_rs_plan" : "decode_batch_dev_fmt_plan", from_streams(streams, lens, n),
                     Sink{roi, F32, fmt, rs}, FMT, out_bitdepth, out_chroma, geom, info, nullptr, workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_rs(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                        void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                        const ccmi_resample *rs, int out_bitdepth, int out_chroma, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    return sink_run(rs ? "decode_batch_dev_rs" : "decode_batch_dev_fmt", from_streams(streams, lens, n),
                    Sink{roi, F32, fmt, rs}, FMT, out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes,
                    stream);
}

extern "C" int ccmi_decode_batch_dev_fmt_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                              const ccmi_rect *roi, int out_bitdepth, int out_chroma,
                                              const ccmi_tensor_fmt *fmt, ccmi_frame_geom *geom, ccmi_roi_info *info,
                                              size_t *workspace_bytes)
{
    return ccmi_decode_batch_dev_rs_plan(streams, lens, n, roi, out_bitdepth, out_chroma, fmt, nullptr, geom, info,
                                         workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_fmt(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                         void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                         int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return ccmi_decode_batch_dev_rs(streams, lens, n, roi, out_dev, out_caps, fmt, nullptr, out_bitdepth, out_chroma,
                                    workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_warp_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                               int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                               const ccmi_warp *warp, ccmi_frame_geom *geom, ccmi_roi_info *info,
                                               ccmi_rect *window, size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_warp_plan (frame 0)", from_streams(streams, lens, n), Sink{nullptr, F32, fmt, nullptr, warp},
                     FMT_WARP, out_bitdepth, out_chroma, geom, info, window, workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_warp(const uint8_t *const *streams, const size_t *lens, int n,
                                          void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                          const ccmi_warp *warp, int out_bitdepth, int out_chroma, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    return sink_run("decode_batch_dev_warp (frame 0)", from_streams(streams, lens, n), Sink{nullptr, F32, fmt, nullptr, warp},
                    FMT_WARP, out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_col_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                              const ccmi_rect *roi, int out_bitdepth, int out_chroma,
                                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, const ccmi_warp *warp,
                                              const ccmi_colour *colour, ccmi_frame_geom *geom, ccmi_roi_info *info,
                                              ccmi_rect *window, size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_col_plan (frame 0)", from_streams(streams, lens, n), Sink{roi, F32, fmt, rs, warp, colour},
                     FMT, out_bitdepth, out_chroma, geom, info, window, workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_col(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                         void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                         const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                         int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return sink_run("decode_batch_dev_col (frame 0)", from_streams(streams, lens, n), Sink{roi, F32, fmt, rs, warp, colour}, FMT,
                    out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_flt_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                              const ccmi_rect *roi, int out_bitdepth, int out_chroma,
                                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, const ccmi_warp *warp,
                                              const ccmi_colour *colour, const ccmi_filter *filter, ccmi_frame_geom *geom,
                                              ccmi_roi_info *info, ccmi_rect *window, size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_flt_plan (frame 0)", from_streams(streams, lens, n),
                     Sink{roi, F32, fmt, rs, warp, colour, nullptr, filter}, FMT, out_bitdepth, out_chroma, geom, info, window,
                     workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_flt(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                         void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                         const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                         const ccmi_filter *filter, int out_bitdepth, int out_chroma, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    return sink_run("decode_batch_dev_flt (frame 0)", from_streams(streams, lens, n),
                    Sink{roi, F32, fmt, rs, warp, colour, nullptr, filter}, FMT, out_dev, out_caps, out_bitdepth, out_chroma,
                    workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_tone_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                               const ccmi_rect *roi, int out_bitdepth, int out_chroma,
                                               const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, const ccmi_warp *warp,
                                               const ccmi_colour *colour, const ccmi_tone *tone, const ccmi_filter *filter,
                                               ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window,
                                               size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_tone_plan (frame 0)", from_streams(streams, lens, n),
                     Sink{roi, F32, fmt, rs, warp, colour, tone, filter}, FMT, out_bitdepth, out_chroma, geom, info, window,
                     workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_tone(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                          void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                          const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                          const ccmi_tone *tone, const ccmi_filter *filter, int out_bitdepth, int out_chroma,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("decode_batch_dev_tone (frame 0)", from_streams(streams, lens, n),
                    Sink{roi, F32, fmt, rs, warp, colour, tone, filter}, FMT, out_dev, out_caps, out_bitdepth, out_chroma,
                    workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_mix_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                              const ccmi_rect *roi, int out_bitdepth, int out_chroma,
                                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, const ccmi_warp *warp,
                                              const ccmi_colour *colour, const ccmi_tone *tone, const ccmi_filter *filter,
                                              const ccmi_mix *mix, ccmi_frame_geom *geom, ccmi_roi_info *info,
                                              ccmi_rect *window, size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_mix_plan (frame 0)", from_streams(streams, lens, n),
                     Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix}, FMT, out_bitdepth, out_chroma, geom, info, window,
                     workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_mix(const uint8_t *const *streams, const size_t *lens, int n, const ccmi_rect *roi,
                                         void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                         const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                         const ccmi_tone *tone, const ccmi_filter *filter, const ccmi_mix *mix,
                                         int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return sink_run("decode_batch_dev_mix (frame 0)", from_streams(streams, lens, n),
                    Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix}, FMT, out_dev, out_caps, out_bitdepth, out_chroma,
                    workspace, workspace_bytes, stream);
}

extern "C" int ccmi_decode_batch_dev_blend_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                                const ccmi_rect *roi, int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                                const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                                const ccmi_tone *tone, const ccmi_filter *filter, const ccmi_blend *blend,
                                                const ccmi_mix *mix, ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window,
                                                size_t *workspace_bytes)
{
    return sink_plan("decode_batch_dev_blend_plan (frame 0)", from_streams(streams, lens, n),
                     Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix, blend}, FMT, out_bitdepth, out_chroma, geom, info,
                     window, workspace_bytes);
}

extern "C" int ccmi_decode_batch_dev_blend(const uint8_t *const *streams, const size_t *lens, int n,
                                           const ccmi_rect *roi, void *const *out_dev, const size_t *out_caps,
                                           const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, const ccmi_warp *warp,
                                           const ccmi_colour *colour, const ccmi_tone *tone, const ccmi_filter *filter,
                                           const ccmi_blend *blend, const ccmi_mix *mix, int out_bitdepth, int out_chroma,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("decode_batch_dev_blend (frame 0)", from_streams(streams, lens, n),
                    Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix, blend}, FMT, out_dev, out_caps, out_bitdepth,
                    out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_plan(const uint8_t *const *streams, const size_t *lens, int n, int latent_type,
                                 size_t *store_bytes, size_t *store_bytes_each, size_t *workspace_bytes)
{
    clear_last();
    if (!streams || !lens || !store_bytes || !workspace_bytes)
        return ccmi_set_error(CCMI_ERR_ARG, "latents_plan: null argument");
    ccmi_latents h;
    DecodeRequest rq = request(streams, lens, n, 0, 0);
    rq.lat_store = &h;
    DecodePlan pl;
    if (int rc = decode_plan(rq, pl)) return rc;
    if (int rc = latent_store_layout(pl, latent_type, h)) return rc;
    *store_bytes = h.store_bytes;
    *workspace_bytes = pl.total;
    for (int i = 0; i < n && store_bytes_each; ++i) store_bytes_each[i] = h.s[i].bytes;
    return CCMI_OK;
}

extern "C" int ccmi_latents_decode(const uint8_t *const *streams, const size_t *lens, int n, int latent_type,
                                   void *store, size_t store_bytes, void *workspace, size_t workspace_bytes,
                                   void *stream, ccmi_latents **out)
{
    clear_last();
    if (!streams || !lens || !out) return ccmi_set_error(CCMI_ERR_ARG, "latents_decode: null argument");
    *out = nullptr;
    ccmi_latents *h = new ccmi_latents;
    struct Drop {
        ccmi_latents *p;
        ~Drop() { delete p; }
    } drop{h};
    DecodeRequest rq = request(streams, lens, n, 0, 0);
    rq.lat_store = h;
    rq.ws = workspace;
    rq.ws_bytes = workspace_bytes;
    DecodePlan pl;
    if (int rc = decode_plan(rq, pl)) return rc;
    if (int rc = latent_store_layout(pl, latent_type, *h)) return rc;
    if (store) {
        if (store_bytes < h->store_bytes)
            return ccmi_set_error(CCMI_ERR_ARG, "latents_decode: store of %zu bytes, need %zu", store_bytes, h->store_bytes);
        if (reinterpret_cast<uintptr_t>(store) % 256)
            return ccmi_set_error(CCMI_ERR_ARG, "latents_decode: the store must be 256-byte aligned");
        h->resident = true;
        for (LatentStream &S : h->s) S.base = static_cast<const uint8_t *>(store);
        if (int rc = decode_run(rq, pl, static_cast<hipStream_t>(stream))) return rc;
    } else {
        // plan-only handle: the networks are decoded on the host, nothing touches the GPU
        if (int rc = decode_weights_all(pl.fr)) return rc;
        for (FramePlan &p : pl.fr) p.tail.syn.f24 = syn_weights_fit24(p.f) ? 1 : 0;
    }
    for (int i = 0; i < n; ++i) {
        LatentStream &S = h->s[i];
        S.f = std::move(pl.fr[i].f);
        S.f24 = pl.fr[i].tail.syn.f24;
        // nothing of the caller's streams is referred to from here on
        for (auto &p : S.f.lat_bytes) p = nullptr;
        for (auto &p : S.f.wbytes) p = nullptr;
        S.f.arm.clear();
        S.f.arm.shrink_to_fit();
    }
    drop.p = nullptr;
    *out = h;
    return CCMI_OK;
}

extern "C" void ccmi_latents_free(ccmi_latents *h) { delete h; }

extern "C" int ccmi_latents_count(const ccmi_latents *h) { return h ? (int)h->s.size() : 0; }

extern "C" int ccmi_latents_values(const ccmi_latents *h, int i, int32_t *out_dev, size_t cap_elems, void *stream)
{
    if (!h || !out_dev) return ccmi_set_error(CCMI_ERR_ARG, "latents_values: null argument");
    if (!h->resident) return ccmi_set_error(CCMI_ERR_ARG, "latents_values: the handle is plan-only (built without a store)");
    if (i < 0 || i >= (int)h->s.size())
        return ccmi_set_error(CCMI_ERR_ARG, "latents_values: stream %d outside the handle's %zu streams", i, h->s.size());
    const LatentStream &S = h->s[i];
    const FrameHost &f = S.f;
    size_t need = 0;
    for (int l = 0; l < f.n_layers; ++l) need += (size_t)f.lh[l] * f.lw[l];
    if (cap_elems < need) return ccmi_set_error(CCMI_ERR_ARG, "latents_values: buffer of %zu ints, need %zu", cap_elems, need);
    DecLatUnpackJob jobs[CCMI_MAX_GRIDS];
    uint32_t blocks = 0;
    size_t off = 0;
    for (int l = 0; l < f.n_layers; ++l) {
        const DecWindow w{0, f.lh[l], 0, f.lw[l]};
        jobs[l] = DecLatUnpackJob{f.lat_n[l] ? S.base + S.grid_off[l] : nullptr, out_dev + off, f.lw[l], 0, w.y1, 0, w.x1,
                                  blocks, 0, f.lh[l]};
        blocks += dec_lat_unpack_blocks(w);
        off += (size_t)f.lh[l] * f.lw[l];
    }
    // the job table has to sit in device memory; this call has no workspace argument
    const hipStream_t s = static_cast<hipStream_t>(stream);
    void *tab = nullptr;
    CCMI_HIP_CHECK(hipMalloc(&tab, sizeof jobs));
    struct Free {
        void *p;
        ~Free() { (void)hipFree(p); }
    } guard{tab};
    CCMI_HIP_CHECK(hipMemcpyAsync(tab, jobs, sizeof(DecLatUnpackJob) * f.n_layers, hipMemcpyHostToDevice, s));
    if (int rc = launch_dec_lat_unpack(static_cast<const DecLatUnpackJob *>(tab), f.n_layers, blocks, S.type, s)) return rc;
    CCMI_HIP_CHECK(hipStreamSynchronize(s));
    return CCMI_OK;
}

// The device sinks' table (above) over a latent store.
extern "C" int ccmi_latents_render_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                        int out_bitdepth, int out_chroma, int sample_type, ccmi_frame_geom *geom,
                                        ccmi_roi_info *info, size_t *workspace_bytes)
{
    return sink_plan("latents_render_plan", from_store(h, index, m), Sink{roi, sample_type}, PLAIN, out_bitdepth, out_chroma,
                     geom, info, nullptr, workspace_bytes);
}

extern "C" int ccmi_latents_render(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                   void *const *out_dev, const size_t *out_caps, int sample_type, int out_bitdepth,
                                   int out_chroma, void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("latents_render", from_store(h, index, m), Sink{roi, sample_type}, PLAIN, out_dev, out_caps, out_bitdepth,
                    out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_rs_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                           int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                           const ccmi_resample *rs, ccmi_frame_geom *geom, ccmi_roi_info *info,
                                           size_t *workspace_bytes)
{
    return sink_plan(rs ? "latents_render_rs_plan" : "latents_render_fmt_plan", from_store(h, index, m), Sink{roi, F32, fmt, rs},
                     FMT, out_bitdepth, out_chroma, geom, info, nullptr, workspace_bytes);
}

extern "C" int ccmi_latents_render_rs(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                      void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                      const ccmi_resample *rs, int out_bitdepth, int out_chroma, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    return sink_run(rs ? "latents_render_rs" : "latents_render_fmt", from_store(h, index, m), Sink{roi, F32, fmt, rs}, FMT,
                    out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_fmt_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                            int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                            ccmi_frame_geom *geom, ccmi_roi_info *info, size_t *workspace_bytes)
{
    return ccmi_latents_render_rs_plan(h, index, m, roi, out_bitdepth, out_chroma, fmt, nullptr, geom, info,
                                       workspace_bytes);
}

extern "C" int ccmi_latents_render_fmt(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                       void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                       int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return ccmi_latents_render_rs(h, index, m, roi, out_dev, out_caps, fmt, nullptr, out_bitdepth, out_chroma, workspace,
                                  workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_warp_plan(const ccmi_latents *h, const int *index, int m, int out_bitdepth,
                                             int out_chroma, const ccmi_tensor_fmt *fmt, const ccmi_warp *warp,
                                             ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window,
                                             size_t *workspace_bytes)
{
    return sink_plan("latents_render_warp_plan (frame 0)", from_store(h, index, m), Sink{nullptr, F32, fmt, nullptr, warp},
                     FMT_WARP, out_bitdepth, out_chroma, geom, info, window, workspace_bytes);
}

extern "C" int ccmi_latents_render_warp(const ccmi_latents *h, const int *index, int m, void *const *out_dev,
                                        const size_t *out_caps, const ccmi_tensor_fmt *fmt, const ccmi_warp *warp,
                                        int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    return sink_run("latents_render_warp (frame 0)", from_store(h, index, m), Sink{nullptr, F32, fmt, nullptr, warp}, FMT_WARP,
                    out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_col_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                            int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                            const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                            ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window,
                                            size_t *workspace_bytes)
{
    return sink_plan("latents_render_col_plan (frame 0)", from_store(h, index, m), Sink{roi, F32, fmt, rs, warp, colour}, FMT,
                     out_bitdepth, out_chroma, geom, info, window, workspace_bytes);
}

extern "C" int ccmi_latents_render_col(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                       void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                       const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                       int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return sink_run("latents_render_col (frame 0)", from_store(h, index, m), Sink{roi, F32, fmt, rs, warp, colour}, FMT, out_dev,
                    out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_flt_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                            int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                            const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                            const ccmi_filter *filter, ccmi_frame_geom *geom, ccmi_roi_info *info,
                                            ccmi_rect *window, size_t *workspace_bytes)
{
    return sink_plan("latents_render_flt_plan (frame 0)", from_store(h, index, m),
                     Sink{roi, F32, fmt, rs, warp, colour, nullptr, filter}, FMT, out_bitdepth, out_chroma, geom, info, window,
                     workspace_bytes);
}

extern "C" int ccmi_latents_render_flt(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                       void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                       const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                       const ccmi_filter *filter, int out_bitdepth, int out_chroma, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    return sink_run("latents_render_flt (frame 0)", from_store(h, index, m), Sink{roi, F32, fmt, rs, warp, colour, nullptr, filter},
                    FMT, out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_tone_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                             int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                             const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                             const ccmi_tone *tone, const ccmi_filter *filter, ccmi_frame_geom *geom,
                                             ccmi_roi_info *info, ccmi_rect *window, size_t *workspace_bytes)
{
    return sink_plan("latents_render_tone_plan (frame 0)", from_store(h, index, m),
                     Sink{roi, F32, fmt, rs, warp, colour, tone, filter}, FMT, out_bitdepth, out_chroma, geom, info, window,
                     workspace_bytes);
}

extern "C" int ccmi_latents_render_tone(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                        void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                        const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                        const ccmi_tone *tone, const ccmi_filter *filter, int out_bitdepth, int out_chroma,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("latents_render_tone (frame 0)", from_store(h, index, m), Sink{roi, F32, fmt, rs, warp, colour, tone, filter},
                    FMT, out_dev, out_caps, out_bitdepth, out_chroma, workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_mix_plan(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                            int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                            const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                            const ccmi_tone *tone, const ccmi_filter *filter, const ccmi_mix *mix,
                                            ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window,
                                            size_t *workspace_bytes)
{
    return sink_plan("latents_render_mix_plan (frame 0)", from_store(h, index, m),
                     Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix}, FMT, out_bitdepth, out_chroma, geom, info, window,
                     workspace_bytes);
}

extern "C" int ccmi_latents_render_mix(const ccmi_latents *h, const int *index, int m, const ccmi_rect *roi,
                                       void *const *out_dev, const size_t *out_caps, const ccmi_tensor_fmt *fmt,
                                       const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                       const ccmi_tone *tone, const ccmi_filter *filter, const ccmi_mix *mix,
                                       int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("latents_render_mix (frame 0)", from_store(h, index, m),
                    Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix}, FMT, out_dev, out_caps, out_bitdepth, out_chroma,
                    workspace, workspace_bytes, stream);
}

extern "C" int ccmi_latents_render_blend_plan(const ccmi_latents *h, const int *index, int m,
                                              const ccmi_rect *roi, int out_bitdepth, int out_chroma, const ccmi_tensor_fmt *fmt,
                                              const ccmi_resample *rs, const ccmi_warp *warp, const ccmi_colour *colour,
                                              const ccmi_tone *tone, const ccmi_filter *filter, const ccmi_blend *blend,
                                              const ccmi_mix *mix, ccmi_frame_geom *geom, ccmi_roi_info *info, ccmi_rect *window,
                                              size_t *workspace_bytes)
{
    return sink_plan("latents_render_blend_plan (frame 0)", from_store(h, index, m),
                     Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix, blend}, FMT, out_bitdepth, out_chroma, geom, info,
                     window, workspace_bytes);
}

extern "C" int ccmi_latents_render_blend(const ccmi_latents *h, const int *index, int m,
                                         const ccmi_rect *roi, void *const *out_dev, const size_t *out_caps,
                                         const ccmi_tensor_fmt *fmt, const ccmi_resample *rs, const ccmi_warp *warp,
                                         const ccmi_colour *colour, const ccmi_tone *tone, const ccmi_filter *filter,
                                         const ccmi_blend *blend, const ccmi_mix *mix, int out_bitdepth, int out_chroma,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    return sink_run("latents_render_blend (frame 0)", from_store(h, index, m),
                    Sink{roi, F32, fmt, rs, warp, colour, tone, filter, mix, blend}, FMT, out_dev, out_caps, out_bitdepth,
                    out_chroma, workspace, workspace_bytes, stream);
}

namespace ccmi {

bool dec_syn_weights_fit24(const FrameHost &f) { return syn_weights_fit24(f); }

void dec_set_last_call(const float ms[4])
{
    clear_last();
    for (int k = 0; k < 4; ++k) g_last_ms[k] = ms[k];
}

} // namespace ccmi

extern "C" int ccmi_decode_last_tail_groups(int *batched, int *per_frame)
{
    if (!batched || !per_frame) return ccmi_set_error(CCMI_ERR_ARG, "decode_last_tail_groups: null argument");
    *batched = g_last_tails[0];
    *per_frame = g_last_tails[1];
    return CCMI_OK;
}

extern "C" int ccmi_decode_latents(const uint8_t *stream, size_t len, int32_t *out, size_t cap, void *hstream)
{
    if (!stream || !out) return ccmi_set_error(CCMI_ERR_ARG, "decode_latents: null argument");
    FrameHost f;
    if (int rc = parse_and_decode_frame(stream, len, f)) return rc;
    size_t n = 0;
    for (int l = 0; l < f.n_layers; ++l) n += (size_t)f.lh[l] * f.lw[l];
    if (cap < n) return ccmi_set_error(CCMI_ERR_ARG, "decode_latents: buffer of %zu ints, need %zu", cap, n);
    size_t osz = 0;
    if (int rc = ccmi_decode_output_size(stream, len, 0, 0, 1, &osz)) return rc;
    std::vector<uint8_t> tmp(osz);
    uint8_t *op = tmp.data();
    DecodeRequest rq = request(&stream, &len, 1, 0, 0);
    rq.as_yuv = 1;
    rq.outs = &op;
    rq.caps = &osz;
    rq.lat_out = &out;
    return decode_many(rq, hstream);
}

static bool ends_with(const std::string &a, const char *b)
{
    const size_t n = strlen(b);
    return a.size() >= n && a.compare(a.size() - n, n, b) == 0;
}

extern "C" int ccmi_decode_file(const char *in_path, const char *out_path, int out_bitdepth, int out_chroma,
                                int verbosity, int device)
{
    if (!in_path) {
        ccmi_set_error(CCMI_ERR_ARG, "decode: no input bitstream");
        return 1;
    }
    FILE *fi = fopen(in_path, "rb");
    if (!fi) {
        ccmi_set_error(CCMI_ERR_IO, "cannot open %s for reading", in_path);
        return 1;
    }
    std::vector<uint8_t> buf;
    {
        fseek(fi, 0, SEEK_END);
        long n = ftell(fi);
        fseek(fi, 0, SEEK_SET);
        buf.resize(n > 0 ? (size_t)n : 0);
        const bool ok = buf.empty() || fread(buf.data(), 1, buf.size(), fi) == buf.size();
        fclose(fi);
        if (!ok) {
            ccmi_set_error(CCMI_ERR_IO, "cannot read %s", in_path);
            return 1;
        }
    }
    if (hipSetDevice(device) != hipSuccess) {
        ccmi_set_error(CCMI_ERR_HIP, "hipSetDevice(%d) failed", device);
        return 1;
    }
    const std::string out = out_path ? out_path : "";
    const int as_yuv = ends_with(out, ".yuv");
    size_t need = 0;
    if (ccmi_decode_output_size(buf.data(), buf.size(), out_bitdepth, out_chroma, as_yuv, &need)) return 1;
    std::vector<uint8_t> res(need);
    const uint8_t *sp = buf.data();
    const size_t ln = buf.size();
    uint8_t *op = res.data();
    size_t got = 0;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, nullptr);
    DecodeRequest rq = request(&sp, &ln, 1, out_bitdepth, out_chroma);
    rq.as_yuv = as_yuv;
    rq.outs = &op;
    rq.caps = &need;
    rq.sizes = &got;
    if (decode_many(rq, nullptr)) return 1;
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (verbosity >= 1) printf("time: all %g\n", ms * 1e-3);
    if (!out.empty()) {
        FILE *fo = fopen(out.c_str(), "wb");
        if (!fo) {
            ccmi_set_error(CCMI_ERR_IO, "cannot open %s for writing", out.c_str());
            return 1;
        }
        const bool ok = fwrite(res.data(), 1, got, fo) == got;
        fclose(fo);
        if (!ok) {
            ccmi_set_error(CCMI_ERR_IO, "cannot write %s", out.c_str());
            return 1;
        }
    }
    return 0;
}
