// dec_store_file.cpp -- path B: latent stores as files (the file form is the contract in ccmi.h).
// Export: the defined bytes of any resident handle's streams gathered into a zeroed DATA image on
// the device, checksummed there, downloaded once; HEAD and INDEX written by the host.  Import:
// META is untrusted input and is validated on the host (overflow-checked, every field held to the
// .cool header's limits, the layout derived and never read), DATA is uploaded once, checksummed,
// and every SEG descriptor table is verified on the device before a handle exists
// (dec_lat_seg_verify: the safety argument is at the kernel).
#include <limits.h>
#include <string.h>

#include <algorithm>

#include "dec_plan.h"

using namespace ccmi;

namespace {

constexpr size_t kHeadBytes = 64;
constexpr uint32_t kFileVersion = 1;
constexpr char kMagic[9] = "CCMILAT1";
constexpr uint64_t kMaxNetInts = 1u << 22; // upsampling + synthesis integers of one stream
constexpr int kScalars = 14;               // the record's FrameHost fields

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

bool add_ok(uint64_t a, uint64_t b, uint64_t &out)
{
    out = a + b;
    return out >= a;
}

// the contract's checksum over n bytes (zero-extended to whole words)
void file_sum(const uint8_t *p, size_t n, uint64_t sum[2])
{
    sum[0] = sum[1] = 0;
    size_t i = 0;
    for (; i + 4 <= n; i += 4) {
        uint32_t w;
        memcpy(&w, p + i, 4);
        sum[0] += w;
        sum[1] += (uint64_t)(i / 4 + 1) * w;
    }
    if (i < n) {
        uint32_t w = 0;
        memcpy(&w, p + i, n - i);
        sum[0] += w;
        sum[1] += (uint64_t)(i / 4 + 1) * w;
    }
}

struct Head {
    uint32_t n_streams = 0;
    uint64_t index_bytes = 0, data_off = 0, data_bytes = 0, index_sum[2] = {0, 0};
};

uint32_t rd32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
uint64_t rd64(const uint8_t *p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

int parse_head(const void *head, size_t head_bytes, const char *who, Head &H)
{
    if (!head) return ccmi_set_error(CCMI_ERR_ARG, "%s: null argument", who);
    if (head_bytes < kHeadBytes)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: %zu bytes, the head of a latent file takes %zu", who, head_bytes,
                              kHeadBytes);
    const uint8_t *p = static_cast<const uint8_t *>(head);
    if (memcmp(p, kMagic, 8) != 0) return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: not a latent file (magic)", who);
    const uint32_t version = rd32(p + 8);
    if (version != kFileVersion)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: file version %u, this library reads version %u", who, version,
                              kFileVersion);
    H.n_streams = rd32(p + 12);
    H.index_bytes = rd64(p + 16);
    H.data_off = rd64(p + 24);
    H.data_bytes = rd64(p + 32);
    H.index_sum[0] = rd64(p + 40);
    H.index_sum[1] = rd64(p + 48);
    if (H.n_streams < 1 || H.n_streams > (uint32_t)INT_MAX)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: n_streams %u", who, H.n_streams);
    if (rd64(p + 56) != 0) return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: the head's reserved field is not 0", who);
    // a record takes at least its fixed fields: bounds n_streams by the INDEX before anything is sized by it
    if (H.index_bytes % 8 || H.index_bytes > (1ull << 48) || H.index_bytes / 8 < H.n_streams)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: index_bytes %llu for %u streams", who,
                              (unsigned long long)H.index_bytes, H.n_streams);
    const uint64_t want = (kHeadBytes + H.index_bytes + 255) / 256 * 256;
    if (H.data_off != want)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: data_off %llu, the index ends at %llu: must be %llu", who,
                              (unsigned long long)H.data_off, (unsigned long long)(kHeadBytes + H.index_bytes),
                              (unsigned long long)want);
    uint64_t end;
    if (H.data_bytes % 256 || !add_ok(H.data_off, H.data_bytes, end) || end > (uint64_t)(SIZE_MAX / 2))
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: data_bytes %llu", who, (unsigned long long)H.data_bytes);
    return CCMI_OK;
}

// One stream's record, host form.  f carries the header facts only (ups / syn / arm empty).
struct Record {
    uint32_t type = 0, user_flags = 0;
    uint64_t part_bytes = 0, part_sum[2] = {0, 0};
    FrameHost f;
    uint32_t seg_words[CCMI_MAX_GRIDS] = {};
    size_t n_ups = 0, n_syn = 0; // integers
};

void record_of(const LatentStream &S, uint32_t user_flags, Record &R)
{
    R.type = (uint32_t)S.type;
    R.user_flags = user_flags;
    const FrameHost &f = S.f;
    R.f.h = f.h, R.f.w = f.w, R.f.bitdepth = f.bitdepth, R.f.frame_data_type = f.frame_data_type;
    R.f.intra_period = f.intra_period, R.f.dim_arm = f.dim_arm, R.f.n_hidden = f.n_hidden;
    R.f.n_ups = f.n_ups, R.f.ups_ks = f.ups_ks, R.f.n_pre = f.n_pre, R.f.pre_ks = f.pre_ks;
    R.f.n_branches = f.n_branches, R.f.sig_blk = f.sig_blk, R.f.n_layers = f.n_layers;
    R.f.layers = f.layers;
    R.f.blend = f.blend;
    for (int l = 0; l < CCMI_MAX_GRIDS; ++l) {
        R.f.lh[l] = f.lh[l], R.f.lw[l] = f.lw[l], R.f.lat_n[l] = f.lat_n[l];
        R.seg_words[l] = S.type == CCMI_LATENT_SEG && l < f.n_layers && f.lat_n[l] ? S.seg_words[l] : 0;
    }
    R.n_ups = f.ups.size();
    R.n_syn = f.syn.size();
}

size_t record_bytes(const Record &R)
{
    const size_t words = 8 + 1 + kScalars + 1 + 4 * R.f.layers.size() + 2 * (size_t)R.f.n_layers + 1 + R.f.blend.size();
    return align_up(4 * words, 8);
}

void put32(std::vector<uint8_t> &o, uint32_t v)
{
    uint8_t b[4];
    memcpy(b, &v, 4);
    o.insert(o.end(), b, b + 4);
}
void put64(std::vector<uint8_t> &o, uint64_t v)
{
    uint8_t b[8];
    memcpy(b, &v, 8);
    o.insert(o.end(), b, b + 8);
}

void write_record(const Record &R, std::vector<uint8_t> &o)
{
    const size_t start = o.size(), nb = record_bytes(R);
    const FrameHost &f = R.f;
    put32(o, (uint32_t)nb);
    put32(o, R.type);
    put64(o, R.part_bytes);
    put64(o, R.part_sum[0]);
    put64(o, R.part_sum[1]);
    put32(o, R.user_flags);
    const int sc[kScalars] = {f.h, f.w, f.bitdepth, f.frame_data_type, f.intra_period, f.dim_arm, f.n_hidden,
                              f.n_ups, f.ups_ks, f.n_pre, f.pre_ks, f.n_branches, f.sig_blk, f.n_layers};
    for (int v : sc) put32(o, (uint32_t)v);
    put32(o, (uint32_t)f.layers.size());
    for (const SynLayerDesc &L : f.layers) {
        put32(o, (uint32_t)L.n_out);
        put32(o, (uint32_t)L.ks);
        put32(o, (uint32_t)L.residual);
        put32(o, (uint32_t)L.relu);
    }
    for (int l = 0; l < f.n_layers; ++l) put32(o, f.lat_n[l]);
    for (int l = 0; l < f.n_layers; ++l) put32(o, R.seg_words[l]);
    put32(o, (uint32_t)f.blend.size());
    for (int32_t v : f.blend) put32(o, (uint32_t)v);
    o.resize(start + nb, 0);
}

// The layout of one stream's part (the arithmetic of latent_store_layout and seg_store_layout):
// offsets from `pos`, which is 256-byte aligned.  Everything entering it is bounded by the
// record's checks (h, w < 2^16; n_ups + n_syn <= kMaxNetInts; seg_words <= h_l w_l).
void part_layout(const Record &R, size_t pos, LatentStream &S)
{
    const FrameHost &f = R.f;
    S.type = (int)R.type;
    S.off = pos;
    S.ups_off = pos;
    pos += align_up(R.n_ups * 4, 16);
    S.syn_off = pos;
    pos += align_up(R.n_syn * 4, 16);
    const size_t eb = dec_lat_elem_bytes(S.type);
    for (int l = 0; l < CCMI_MAX_GRIDS; ++l) {
        S.grid_off[l] = l < f.n_layers ? pos : 0;
        S.seg_words[l] = 0;
        if (l >= f.n_layers || !f.lat_n[l]) continue;
        if (S.type == CCMI_LATENT_SEG) {
            S.seg_words[l] = R.seg_words[l];
            pos += dec_lat_seg_table_bytes(f.lh[l], f.lw[l]) + align_up((size_t)R.seg_words[l] * 4, 16);
        } else {
            pos += align_up((size_t)f.lh[l] * f.lw[l] * eb, 16);
        }
    }
    pos = align_up(pos, 256);
    S.bytes = pos - S.off;
}

struct Cursor {
    const uint8_t *p;
    size_t n, pos;
    bool ok = true;
    uint32_t u32()
    {
        if (pos > n || n - pos < 4) {
            ok = false;
            return 0;
        }
        const uint32_t v = rd32(p + pos);
        pos += 4;
        return v;
    }
    uint64_t u64()
    {
        const uint64_t lo = u32(), hi = u32();
        return lo | hi << 32;
    }
    int i32() { return (int)u32(); }
};

#define REC_FAIL(...) return ccmi_set_error(CCMI_ERR_BITSTREAM, __VA_ARGS__)

// Record i at the cursor: every field checked, the part's size derived and compared.
int parse_record(Cursor &c, const char *who, int i, Record &R)
{
    const size_t start = c.pos;
    const uint32_t nb = c.u32();
    R.type = c.u32();
    R.part_bytes = c.u64();
    R.part_sum[0] = c.u64();
    R.part_sum[1] = c.u64();
    R.user_flags = c.u32();
    FrameHost &f = R.f;
    int *sc[kScalars] = {&f.h, &f.w, &f.bitdepth, &f.frame_data_type, &f.intra_period, &f.dim_arm, &f.n_hidden,
                         &f.n_ups, &f.ups_ks, &f.n_pre, &f.pre_ks, &f.n_branches, &f.sig_blk, &f.n_layers};
    for (int *v : sc) *v = c.i32();
    const uint32_t n_syn = c.u32();
    if (!c.ok) REC_FAIL("%s: stream %d: the index ends inside its record", who, i);
    if (R.type > (uint32_t)CCMI_LATENT_SEG) REC_FAIL("%s: stream %d: latent_type %u", who, i, R.type);
    // the limits of the .cool header's fields (parse_frame_header): sizes 16 bits, the nibbles and bytes;
    // a nibble's kernel size is one the tail's upsampling takes (dec_tail.hip: ups_ks <= 16, pre_ks <= 15)
    if (f.h < 1 || f.h > 65535 || f.w < 1 || f.w > 65535) REC_FAIL("%s: stream %d: frame size h %d w %d", who, i, f.h, f.w);
    if (f.bitdepth < 8 || f.bitdepth > 23 || f.frame_data_type < 0 || f.frame_data_type > 15)
        REC_FAIL("%s: stream %d: bitdepth %d, frame_data_type %d", who, i, f.bitdepth, f.frame_data_type);
    if (f.intra_period != 0) REC_FAIL("%s: stream %d: intra_period %d", who, i, f.intra_period);
    if (f.dim_arm != 8 && f.dim_arm != 16 && f.dim_arm != 24 && f.dim_arm != 32)
        REC_FAIL("%s: stream %d: dim_arm %d", who, i, f.dim_arm);
    if (f.n_hidden < 0 || f.n_hidden > 4) REC_FAIL("%s: stream %d: %d ARM hidden layers", who, i, f.n_hidden);
    if (f.n_ups < 1 || f.n_ups > 15 || f.ups_ks < 2 || f.ups_ks > 15 || f.n_pre < 1 || f.n_pre > 15 || f.pre_ks < 1 ||
        f.pre_ks > 15)
        REC_FAIL("%s: stream %d: upsampling header %d x %d, %d x %d", who, i, f.n_ups, f.ups_ks, f.n_pre, f.pre_ks);
    if (f.n_branches < 1 || f.n_branches > 8) REC_FAIL("%s: stream %d: %d synthesis branches", who, i, f.n_branches);
    if (f.sig_blk < -128 || f.sig_blk > 127) REC_FAIL("%s: stream %d: sig_blk %d", who, i, f.sig_blk);
    if (f.n_layers < 2 || f.n_layers > CCMI_MAX_GRIDS) REC_FAIL("%s: stream %d: bad latent layer count %d", who, i, f.n_layers);
    if (n_syn < 1 || n_syn > CCMI_MAX_SYN_LAYERS) REC_FAIL("%s: stream %d: bad synthesis layer count %u", who, i, n_syn);
    f.layers.resize(n_syn);
    for (SynLayerDesc &L : f.layers) {
        L.n_out = c.i32();
        L.ks = c.i32();
        L.residual = c.i32();
        L.relu = c.i32();
    }
    for (int l = 0; l < f.n_layers; ++l) f.lat_n[l] = c.u32();
    for (int l = 0; l < f.n_layers; ++l) R.seg_words[l] = c.u32();
    const uint32_t n_blend = c.u32();
    if (!c.ok) REC_FAIL("%s: stream %d: the index ends inside its record", who, i);
    if (n_blend != (uint32_t)(f.n_branches > 1 ? f.n_branches : 0))
        REC_FAIL("%s: stream %d: %u blend integers for %d branches", who, i, n_blend, f.n_branches);
    f.blend.resize(n_blend);
    for (int32_t &v : f.blend) v = c.i32();
    if ((c.pos - start) % 8) c.u32();
    if (!c.ok) REC_FAIL("%s: stream %d: the index ends inside its record", who, i);
    if ((size_t)nb != c.pos - start)
        REC_FAIL("%s: stream %d: record_bytes %u, its counts give %zu", who, i, nb, c.pos - start);
    uint64_t per_branch = 0;
    int cin = f.n_layers;
    for (const SynLayerDesc &L : f.layers) {
        if (L.n_out < 1 || L.n_out > 255 || L.ks < 1 || L.ks > 255 || (L.ks & 1) == 0)
            REC_FAIL("%s: stream %d: synthesis layer of %d outputs, kernel size %d", who, i, L.n_out, L.ks);
        if ((L.residual | L.relu) & ~1) REC_FAIL("%s: stream %d: synthesis layer flags %d / %d", who, i, L.residual, L.relu);
        per_branch += (uint64_t)L.n_out * cin * L.ks * L.ks + L.n_out; // < 16 * 2^32
        cin = L.n_out;
    }
    if (f.layers.back().n_out < 3) REC_FAIL("%s: stream %d: synthesis must output >= 3 planes", who, i);
    R.n_ups = (size_t)f.n_ups * f.ups_ks + (size_t)f.n_pre * f.pre_ks;
    if (per_branch * f.n_branches + R.n_ups > kMaxNetInts)
        REC_FAIL("%s: stream %d: %llu network integers (at most %llu)", who, i,
                 (unsigned long long)(per_branch * f.n_branches + R.n_ups), (unsigned long long)kMaxNetInts);
    R.n_syn = (size_t)(per_branch * f.n_branches);
    for (int l = 0, hh = f.h, ww = f.w; l < f.n_layers; ++l, hh = (hh + 1) / 2, ww = (ww + 1) / 2) {
        f.lh[l] = hh;
        f.lw[l] = ww;
        if (f.lat_n[l] >= (1u << 24)) REC_FAIL("%s: stream %d, latent grid %d: lat_n %u", who, i, l, f.lat_n[l]);
        const uint64_t cap = std::min<uint64_t>((uint64_t)hh * ww, (uint64_t)kSegOffMax + kSegLen);
        if (R.type != (uint32_t)CCMI_LATENT_SEG || !f.lat_n[l]) {
            if (R.seg_words[l])
                REC_FAIL("%s: stream %d, latent grid %d: seg_words %u of a grid without a payload", who, i, l, R.seg_words[l]);
        } else if (R.seg_words[l] > cap) {
            REC_FAIL("%s: stream %d, latent grid %d: seg_words %u (at most %llu: h w values, 29-bit offsets)", who, i, l,
                     R.seg_words[l], (unsigned long long)cap);
        }
    }
    LatentStream S;
    part_layout(R, 0, S);
    if (R.part_bytes != (uint64_t)S.bytes)
        REC_FAIL("%s: stream %d: part_bytes %llu, its header gives %zu", who, i, (unsigned long long)R.part_bytes, S.bytes);
    return CCMI_OK;
}

// META as a whole: the head, every record, the sums of sizes, index_sum.
int parse_meta(const void *meta, size_t meta_bytes, const char *who, Head &H, std::vector<Record> &recs)
{
    if (int rc = parse_head(meta, meta_bytes, who, H)) return rc;
    if (meta_bytes - kHeadBytes < H.index_bytes)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: %zu bytes of META, the head states %llu", who, meta_bytes,
                              (unsigned long long)(kHeadBytes + H.index_bytes));
    const uint8_t *p = static_cast<const uint8_t *>(meta);
    uint64_t sum[2];
    file_sum(p + kHeadBytes, (size_t)H.index_bytes, sum);
    if (sum[0] != H.index_sum[0] || sum[1] != H.index_sum[1])
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: the index does not match its checksum (index_sum)", who);
    Cursor c{p, kHeadBytes + (size_t)H.index_bytes, kHeadBytes};
    recs.clear();
    uint64_t data = 0;
    for (uint32_t i = 0; i < H.n_streams; ++i) {
        recs.emplace_back();
        if (int rc = parse_record(c, who, (int)i, recs.back())) return rc;
        if (!add_ok(data, recs.back().part_bytes, data) || data > H.data_bytes)
            return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: stream %u: the parts pass data_bytes %llu", who, i,
                                  (unsigned long long)H.data_bytes);
    }
    if (c.pos != c.n)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: index_bytes %llu, the %u records take %zu", who,
                              (unsigned long long)H.index_bytes, H.n_streams, c.pos - kHeadBytes);
    if (data != H.data_bytes)
        return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: data_bytes %llu, the parts take %llu", who,
                              (unsigned long long)H.data_bytes, (unsigned long long)data);
    return CCMI_OK;
}

int pick_range(const Head &H, int first, int count, const char *who, int &n)
{
    const int total = (int)H.n_streams;
    if (first < 0 || first >= total)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: first %d outside the file's %d streams", who, first, total);
    n = count < 0 ? total - first : count;
    if (n < 1 || n > total - first)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: count %d from stream %d, the file has %d streams", who, count, first, total);
    return CCMI_OK;
}

// The import's workspace (bytes): the streams' sums and the grids' status words (cleared on the
// device), then the two job tables (uploaded in one copy).
struct ImportPlan {
    size_t n_verify = 0;
    size_t sums_off = 0, status_off = 0, tab_off = 0, verify_off = 0, total = 0;
    size_t clear_bytes() const { return tab_off; }
};

ImportPlan import_layout(const std::vector<Record> &recs, int first, int n)
{
    ImportPlan ip;
    for (int i = first; i < first + n; ++i)
        for (int l = 0; l < recs[i].f.n_layers; ++l)
            ip.n_verify += recs[i].type == (uint32_t)CCMI_LATENT_SEG && recs[i].f.lat_n[l] ? 1 : 0;
    ip.sums_off = 0;
    ip.status_off = align_up(16 * (size_t)n, 256);
    ip.tab_off = ip.status_off + align_up(4 * ip.n_verify, 256);
    ip.verify_off = ip.tab_off + align_up(sizeof(DecLatSumJob) * (size_t)n, 256);
    ip.total = ip.verify_off + align_up(sizeof(DecLatVerifyJob) * ip.n_verify, 256);
    return ip;
}

// The export's workspace: the DATA image and the streams' sums (cleared on the device), then the
// gather and the checksum job tables (one upload).
struct ExportPlan {
    std::vector<int> idx;
    std::vector<Record> recs;
    std::vector<size_t> part_off; // of the image
    size_t meta_bytes = 0, data_off = 0, data_bytes = 0;
    size_t n_gather = 0;
    size_t sums_off = 0, tab_off = 0, sumjob_off = 0, total = 0;
    size_t clear_bytes() const { return tab_off; }
};

int export_layout(const ccmi_latents *h, const int *index, int m, const char *who, ExportPlan &ep)
{
    if (!h) return ccmi_set_error(CCMI_ERR_ARG, "%s: the handle is NULL", who);
    const int n = (int)h->s.size();
    if (m < 1) return ccmi_set_error(CCMI_ERR_ARG, "%s: no streams (m < 1)", who);
    if (!index && m != n)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: %d streams without an index, the handle has %d", who, m, n);
    ep.idx.resize(m);
    ep.recs.resize(m);
    ep.part_off.resize(m);
    size_t index_bytes = 0, pos = 0;
    for (int j = 0; j < m; ++j) {
        const int i = index ? index[j] : j;
        if (i < 0 || i >= n)
            return ccmi_set_error(CCMI_ERR_ARG, "%s: stream %d: index %d outside the handle's %d streams", who, j, i, n);
        ep.idx[j] = i;
        const LatentStream &S = h->s[i];
        Record &R = ep.recs[j];
        record_of(S, 0, R);
        LatentStream T;
        part_layout(R, 0, T);
        R.part_bytes = T.bytes;
        if (T.bytes != S.bytes)
            return ccmi_set_error(CCMI_ERR_ARG, "%s: stream %d: its store part takes %zu bytes, the file form %zu", who, j,
                                  S.bytes, T.bytes);
        ep.part_off[j] = pos;
        pos += T.bytes;
        index_bytes += record_bytes(R);
        ep.n_gather += 2 + 2 * (size_t)S.f.n_layers;
    }
    ep.meta_bytes = kHeadBytes + index_bytes;
    ep.data_off = align_up(ep.meta_bytes, 256);
    ep.data_bytes = pos;
    ep.sums_off = align_up(pos, 256);
    ep.tab_off = ep.sums_off + align_up(16 * (size_t)m, 256);
    ep.sumjob_off = ep.tab_off + align_up(sizeof(DecLatGatherJob) * ep.n_gather, 256);
    ep.total = ep.sumjob_off + align_up(sizeof(DecLatSumJob) * (size_t)m, 256);
    return CCMI_OK;
}

// a device workspace: the caller's (checked), or one allocated for the call
struct Workspace {
    uint8_t *dev = nullptr;
    bool owned = false;
    ~Workspace() { if (owned && dev) (void)hipFree(dev); }
};

int check_workspace(const void *workspace, size_t workspace_bytes, size_t need, const char *who)
{
    if (!workspace) return CCMI_OK;
    if (workspace_bytes < need)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: workspace must be 256-byte aligned", who);
    return CCMI_OK;
}

int take_workspace(void *workspace, size_t need, Workspace &w)
{
    w.dev = static_cast<uint8_t *>(workspace);
    if (!w.dev) {
        CCMI_HIP_CHECK(hipMalloc(&w.dev, std::max<size_t>(need, 256)));
        w.owned = true;
    }
    return CCMI_OK;
}

struct Events {
    hipEvent_t e[3] = {};
    bool ok = true;
    Events()
    {
        for (auto &x : e)
            if (hipEventCreate(&x) != hipSuccess) ok = false;
    }
    ~Events()
    {
        for (auto &x : e)
            if (x) (void)hipEventDestroy(x);
    }
    void rec(int i, hipStream_t s)
    {
        if (ok) (void)hipEventRecord(e[i], s);
    }
};

// the handle's stream of a record: header facts, the part's layout from `pos`; networks empty
void stream_of(const Record &R, size_t pos, LatentStream &S)
{
    S.f = R.f;
    part_layout(R, pos, S);
}

} // namespace

extern "C" int ccmi_latents_file_head(const void *head, size_t head_bytes, int *n_streams, size_t *meta_bytes,
                                      size_t *file_bytes)
{
    Head H;
    if (int rc = parse_head(head, head_bytes, "latents_file_head", H)) return rc;
    if (n_streams) *n_streams = (int)H.n_streams;
    if (meta_bytes) *meta_bytes = kHeadBytes + (size_t)H.index_bytes;
    if (file_bytes) *file_bytes = (size_t)(H.data_off + H.data_bytes);
    return CCMI_OK;
}

extern "C" int ccmi_latents_export_plan(const ccmi_latents *h, const int *index, int m, size_t *meta_bytes,
                                        size_t *file_bytes, size_t *workspace_bytes)
{
    ExportPlan ep;
    if (int rc = export_layout(h, index, m, "latents_export_plan", ep)) return rc;
    if (meta_bytes) *meta_bytes = ep.meta_bytes;
    if (file_bytes) *file_bytes = ep.data_off + ep.data_bytes;
    if (workspace_bytes) *workspace_bytes = ep.total;
    return CCMI_OK;
}

extern "C" int ccmi_latents_export(const ccmi_latents *h, const int *index, int m, const uint32_t *user_flags, void *file,
                                   size_t file_bytes, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "latents_export";
    if (h && !h->resident)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: the handle is plan-only (built without a store): nothing to export", who);
    ExportPlan ep;
    if (int rc = export_layout(h, index, m, who, ep)) return rc;
    if (!file) return ccmi_set_error(CCMI_ERR_ARG, "%s: null argument", who);
    if (file_bytes < ep.data_off + ep.data_bytes)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: file buffer of %zu bytes, need %zu", who, file_bytes,
                              ep.data_off + ep.data_bytes);
    if (int rc = check_workspace(workspace, workspace_bytes, ep.total, who)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace w;
    if (int rc = take_workspace(workspace, ep.total, w)) return rc;
    // the job tables: every defined range of every stream to its place in the image
    std::vector<uint8_t> tab(ep.total - ep.tab_off, 0);
    DecLatGatherJob *gj = reinterpret_cast<DecLatGatherJob *>(tab.data());
    DecLatSumJob *sj = reinterpret_cast<DecLatSumJob *>(tab.data() + (ep.sumjob_off - ep.tab_off));
    size_t n_gather = 0;
    uint32_t gather_blocks = 0, sum_blocks = 0;
    for (int j = 0; j < m; ++j) {
        const LatentStream &S = h->s[ep.idx[j]];
        const FrameHost &f = S.f;
        LatentStream T;
        part_layout(ep.recs[j], ep.part_off[j], T);
        auto job = [&](size_t from, size_t to, size_t bytes) {
            if (!bytes) return;
            gj[n_gather++] = DecLatGatherJob{S.base + from, w.dev + to, bytes, gather_blocks, 0};
            gather_blocks += dec_lat_gather_blocks(bytes);
        };
        job(S.ups_off, T.ups_off, f.ups.size() * 4);
        job(S.syn_off, T.syn_off, f.syn.size() * 4);
        for (int l = 0; l < f.n_layers; ++l) {
            if (!f.lat_n[l]) continue;
            if (S.type == CCMI_LATENT_SEG) {
                const size_t table = dec_lat_seg_table_bytes(f.lh[l], f.lw[l]);
                job(S.grid_off[l], T.grid_off[l], (size_t)f.lh[l] * dec_lat_seg_per_row(f.lw[l]) * 4);
                job(S.grid_off[l] + table, T.grid_off[l] + table, (size_t)S.seg_words[l] * 4);
            } else {
                job(S.grid_off[l], T.grid_off[l], (size_t)f.lh[l] * f.lw[l] * dec_lat_elem_bytes(S.type));
            }
        }
        sj[j] = DecLatSumJob{reinterpret_cast<const uint32_t *>(w.dev + ep.part_off[j]),
                             reinterpret_cast<unsigned long long *>(w.dev + ep.sums_off) + 2 * (size_t)j, T.bytes / 4,
                             sum_blocks, 0};
        sum_blocks += dec_lat_sum_blocks(T.bytes / 4);
    }
    std::vector<uint64_t> sums(2 * (size_t)m, 0);
    uint8_t *out = static_cast<uint8_t *>(file);
    CCMI_HIP_CHECK(hipMemsetAsync(w.dev, 0, ep.clear_bytes(), s));
    CCMI_HIP_CHECK(hipMemcpyAsync(w.dev + ep.tab_off, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    if (int rc = launch_dec_lat_file_gather(reinterpret_cast<const DecLatGatherJob *>(w.dev + ep.tab_off), (int)n_gather,
                                            gather_blocks, s))
        return rc;
    if (int rc = launch_dec_lat_file_sum(reinterpret_cast<const DecLatSumJob *>(w.dev + ep.sumjob_off), m, sum_blocks, s))
        return rc;
    CCMI_HIP_CHECK(hipMemcpyAsync(out + ep.data_off, w.dev, ep.data_bytes, hipMemcpyDeviceToHost, s));
    CCMI_HIP_CHECK(hipMemcpyAsync(sums.data(), w.dev + ep.sums_off, 16 * (size_t)m, hipMemcpyDeviceToHost, s));
    CCMI_HIP_CHECK(hipStreamSynchronize(s)); // the tables and the host vectors are this call's
    // HEAD and INDEX
    std::vector<uint8_t> idx;
    idx.reserve(ep.meta_bytes - kHeadBytes);
    for (int j = 0; j < m; ++j) {
        Record &R = ep.recs[j];
        R.user_flags = user_flags ? user_flags[j] : 0;
        R.part_sum[0] = sums[2 * (size_t)j];
        R.part_sum[1] = sums[2 * (size_t)j + 1];
        write_record(R, idx);
    }
    uint64_t isum[2];
    file_sum(idx.data(), idx.size(), isum);
    std::vector<uint8_t> head;
    head.insert(head.end(), kMagic, kMagic + 8);
    put32(head, kFileVersion);
    put32(head, (uint32_t)m);
    put64(head, idx.size());
    put64(head, ep.data_off);
    put64(head, ep.data_bytes);
    put64(head, isum[0]);
    put64(head, isum[1]);
    put64(head, 0);
    memcpy(out, head.data(), kHeadBytes);
    memcpy(out + kHeadBytes, idx.data(), idx.size());
    memset(out + ep.meta_bytes, 0, ep.data_off - ep.meta_bytes);
    return CCMI_OK;
}

extern "C" int ccmi_latents_import_plan(const void *meta, size_t meta_bytes, int first, int count, size_t *data_off,
                                        size_t *data_bytes, size_t *store_bytes_each, size_t *workspace_bytes)
{
    const char *who = "latents_import_plan";
    Head H;
    std::vector<Record> recs;
    if (int rc = parse_meta(meta, meta_bytes, who, H, recs)) return rc;
    int n = 0;
    if (int rc = pick_range(H, first, count, who, n)) return rc;
    size_t off = (size_t)H.data_off, bytes = 0;
    for (int i = 0; i < first; ++i) off += (size_t)recs[i].part_bytes;
    for (int i = first; i < first + n; ++i) {
        if (store_bytes_each) store_bytes_each[i - first] = (size_t)recs[i].part_bytes;
        bytes += (size_t)recs[i].part_bytes;
    }
    if (data_off) *data_off = off;
    if (data_bytes) *data_bytes = bytes;
    if (workspace_bytes) *workspace_bytes = import_layout(recs, first, n).total;
    return CCMI_OK;
}

extern "C" int ccmi_latents_import(const void *meta, size_t meta_bytes, int first, int count, const void *data,
                                   size_t data_bytes, void *store, size_t store_bytes, void *workspace,
                                   size_t workspace_bytes, void *stream, uint32_t *user_flags, ccmi_latents **out)
{
    const char *who = "latents_import";
    if (out) *out = nullptr;
    if (!meta || !out) return ccmi_set_error(CCMI_ERR_ARG, "%s: null argument", who);
    Head H;
    std::vector<Record> recs;
    if (int rc = parse_meta(meta, meta_bytes, who, H, recs)) return rc;
    int n = 0;
    if (int rc = pick_range(H, first, count, who, n)) return rc;
    if ((store == nullptr) != (data == nullptr))
        return ccmi_set_error(CCMI_ERR_ARG, "%s: store and data go together (both NULL: a plan-only handle)", who);
    ccmi_latents *h = new ccmi_latents;
    struct Drop {
        ccmi_latents *p;
        ~Drop() { delete p; }
    } drop{h};
    h->s.resize(n);
    size_t pos = 0;
    for (int i = 0; i < n; ++i) {
        stream_of(recs[first + i], pos, h->s[i]);
        pos += h->s[i].bytes;
    }
    h->store_bytes = pos;
    const float none[4] = {0.f, 0.f, 0.f, 0.f};
    if (!store) {
        // plan-only: the networks' integers are in DATA, which this call has not seen; sized, zero
        for (int i = 0; i < n; ++i) {
            h->s[i].f.ups.assign(recs[first + i].n_ups, 0);
            h->s[i].f.syn.assign(recs[first + i].n_syn, 0);
            h->s[i].f24 = 0;
        }
        for (int i = 0; i < n && user_flags; ++i) user_flags[i] = recs[first + i].user_flags;
        dec_set_last_call(none);
        drop.p = nullptr;
        *out = h;
        return CCMI_OK;
    }
    if (data_bytes < pos) return ccmi_set_error(CCMI_ERR_ARG, "%s: data of %zu bytes, need %zu", who, data_bytes, pos);
    if (store_bytes < pos) return ccmi_set_error(CCMI_ERR_ARG, "%s: store of %zu bytes, need %zu", who, store_bytes, pos);
    if (reinterpret_cast<uintptr_t>(store) % 256)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: the store must be 256-byte aligned", who);
    const ImportPlan ip = import_layout(recs, first, n);
    if (int rc = check_workspace(workspace, workspace_bytes, ip.total, who)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace w;
    if (int rc = take_workspace(workspace, ip.total, w)) return rc;
    uint8_t *base = static_cast<uint8_t *>(store);
    std::vector<uint8_t> tab(ip.total - ip.tab_off, 0);
    DecLatSumJob *sj = reinterpret_cast<DecLatSumJob *>(tab.data());
    DecLatVerifyJob *vj = reinterpret_cast<DecLatVerifyJob *>(tab.data() + (ip.verify_off - ip.tab_off));
    struct At {
        int stream, l;
    };
    std::vector<At> grids;
    uint32_t sum_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const LatentStream &S = h->s[i];
        sj[i] = DecLatSumJob{reinterpret_cast<const uint32_t *>(base + S.off),
                             reinterpret_cast<unsigned long long *>(w.dev + ip.sums_off) + 2 * (size_t)i, S.bytes / 4,
                             sum_blocks, 0};
        sum_blocks += dec_lat_sum_blocks(S.bytes / 4);
        for (int l = 0; l < S.f.n_layers && S.type == CCMI_LATENT_SEG; ++l) {
            if (!S.f.lat_n[l]) continue;
            vj[grids.size()] = DecLatVerifyJob{reinterpret_cast<const uint32_t *>(base + S.grid_off[l]),
                                               reinterpret_cast<uint32_t *>(w.dev + ip.status_off) + grids.size(),
                                               S.f.lw[l], S.f.lh[l], (int)dec_lat_seg_per_row(S.f.lw[l]), S.seg_words[l]};
            grids.push_back(At{i, l});
        }
    }
    std::vector<uint64_t> sums(2 * (size_t)n, 0);
    std::vector<uint32_t> status(grids.size(), 0);
    Events ev;
    ev.rec(0, s);
    CCMI_HIP_CHECK(hipMemcpyAsync(base, data, pos, hipMemcpyHostToDevice, s));
    ev.rec(1, s);
    CCMI_HIP_CHECK(hipMemsetAsync(w.dev, 0, ip.clear_bytes(), s));
    CCMI_HIP_CHECK(hipMemcpyAsync(w.dev + ip.tab_off, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    if (int rc = launch_dec_lat_file_sum(reinterpret_cast<const DecLatSumJob *>(w.dev + ip.tab_off), n, sum_blocks, s))
        return rc;
    if (int rc = launch_dec_lat_seg_verify(reinterpret_cast<const DecLatVerifyJob *>(w.dev + ip.verify_off),
                                           (int)grids.size(), s))
        return rc;
    ev.rec(2, s);
    CCMI_HIP_CHECK(hipMemcpyAsync(sums.data(), w.dev + ip.sums_off, 16 * (size_t)n, hipMemcpyDeviceToHost, s));
    if (!grids.empty())
        CCMI_HIP_CHECK(hipMemcpyAsync(status.data(), w.dev + ip.status_off, 4 * grids.size(), hipMemcpyDeviceToHost, s));
    CCMI_HIP_CHECK(hipStreamSynchronize(s));
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    if (ev.ok) {
        (void)hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&ms[1], ev.e[1], ev.e[2]);
    }
    dec_set_last_call(ms);
    for (int i = 0; i < n; ++i) {
        const Record &R = recs[first + i];
        if (sums[2 * (size_t)i] != R.part_sum[0] || sums[2 * (size_t)i + 1] != R.part_sum[1])
            return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: stream %d: its data does not match its checksum (part_sum)", who,
                                  first + i);
    }
    for (size_t g = 0; g < grids.size(); ++g)
        if (status[g])
            return ccmi_set_error(CCMI_ERR_BITSTREAM, "%s: stream %d, latent grid %d: the descriptor table is not that of "
                                  "its payload (%s)", who, first + grids[g].stream, grids[g].l,
                                  status[g] & kSegBadCode     ? "a width code above 5"
                                  : status[g] & kSegBadOffset ? "an offset is not the sum of the words before it"
                                                              : "the words do not add up to seg_words");
    // the networks' integers, from the bytes the device holds
    const uint8_t *d = static_cast<const uint8_t *>(data);
    for (int i = 0; i < n; ++i) {
        LatentStream &S = h->s[i];
        const Record &R = recs[first + i];
        S.f.ups.resize(R.n_ups);
        S.f.syn.resize(R.n_syn);
        if (R.n_ups) memcpy(S.f.ups.data(), d + S.ups_off, R.n_ups * 4);
        if (R.n_syn) memcpy(S.f.syn.data(), d + S.syn_off, R.n_syn * 4);
        S.f24 = dec_syn_weights_fit24(S.f) ? 1 : 0;
        S.base = base;
        if (user_flags) user_flags[i] = R.user_flags;
    }
    h->resident = true;
    drop.p = nullptr;
    *out = h;
    return CCMI_OK;
}
