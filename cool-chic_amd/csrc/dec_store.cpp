// dec_store.cpp -- path B: latent stores made from latent stores.  Compaction of a built
// I8 / I16 / I32 store into the segmented form (CCMI_LATENT_SEG, the contract in ccmi.h; the
// kernels are dec_latents.hip's), one handle over the streams of several handles
// (ccmi_latents_concat), and the per-stream facts of a handle.
#include <limits.h>

#include <algorithm>

#include "dec_plan.h"

using namespace ccmi;

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What a compaction of `src` launches and where its tables sit in the workspace (bytes):
// the segment jobs (one per non-empty grid, streams then grids in order), the copy jobs of
// the networks' integers, the grids' payload words (totals) and the segments' words.
struct CompactPlan {
    struct Grid {
        int stream, l;
        uint32_t first_seg, n_segs;
    };
    std::vector<Grid> grids;
    uint32_t n_segs = 0;
    size_t n_copy = 0; // copy jobs: the non-empty upsampling / synthesis arrays
    size_t jobs_off = 0, copy_off = 0, totals_off = 0, desc_off = 0, total = 0;
    size_t table_bytes() const { return totals_off; } // what the host uploads: both job tables
};

int compact_layout(const ccmi_latents &src, const char *who, CompactPlan &cp)
{
    uint64_t segs = 0;
    for (size_t i = 0; i < src.s.size(); ++i) {
        const LatentStream &S = src.s[i];
        if (S.type == CCMI_LATENT_SEG)
            return ccmi_set_error(CCMI_ERR_ARG, "%s: stream %zu of the source is CCMI_LATENT_SEG already; a compaction takes "
                                  "I8 / I16 / I32 streams", who, i);
        for (int l = 0; l < S.f.n_layers; ++l) {
            if (!S.f.lat_n[l]) continue;
            const uint64_t n = (uint64_t)S.f.lh[l] * dec_lat_seg_per_row(S.f.lw[l]);
            if (segs + n > 0xFFFF0000ull)
                return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "%s: stream %zu, latent grid %d: more than 2^32 segments in one "
                                      "call; compact the streams in several calls", who, i, l);
            cp.grids.push_back(CompactPlan::Grid{(int)i, l, (uint32_t)segs, (uint32_t)n});
            segs += n;
        }
        cp.n_copy += (S.f.ups.empty() ? 0 : 1) + (S.f.syn.empty() ? 0 : 1);
    }
    cp.n_segs = (uint32_t)segs;
    cp.jobs_off = 0;
    cp.copy_off = align_up(sizeof(DecLatSegJob) * cp.grids.size(), 256);
    cp.totals_off = cp.copy_off + align_up(sizeof(DecLatPackJob) * cp.n_copy, 256);
    cp.desc_off = cp.totals_off + align_up(4 * cp.grids.size(), 256);
    cp.total = cp.desc_off + align_up(4 * (size_t)cp.n_segs, 256);
    return CCMI_OK;
}

// The segmented layout of src's streams, the payload of grid g of the plan taking words[g]
// 32-bit words (NULL: every segment at 32 bits, the upper bound).  Fills out.s (the FrameHosts
// and f24 copied from src) and out.store_bytes.
void seg_store_layout(const ccmi_latents &src, const CompactPlan &cp, const uint32_t *words, ccmi_latents &out)
{
    out.s.resize(src.s.size());
    size_t pos = 0, g = 0;
    for (size_t i = 0; i < src.s.size(); ++i) {
        const FrameHost &f = src.s[i].f;
        LatentStream &S = out.s[i];
        S.f = f;
        S.f24 = src.s[i].f24;
        S.type = CCMI_LATENT_SEG;
        S.off = pos;
        S.ups_off = pos;
        pos += align_up(f.ups.size() * 4, 16);
        S.syn_off = pos;
        pos += align_up(f.syn.size() * 4, 16);
        for (int l = 0; l < f.n_layers; ++l) {
            S.grid_off[l] = pos;
            if (!f.lat_n[l]) continue;
            const size_t payload = words ? (size_t)words[g] : (size_t)f.lh[l] * f.lw[l];
            S.seg_words[l] = (uint32_t)std::min<size_t>(payload, 0xFFFFFFFFu); // what an export writes
            pos += dec_lat_seg_table_bytes(f.lh[l], f.lw[l]) + align_up(payload * 4, 16);
            ++g;
        }
        pos = align_up(pos, 256);
        S.bytes = pos - S.off;
    }
    out.store_bytes = pos;
}

int check_source(const ccmi_latents *src, const char *who)
{
    if (!src) return ccmi_set_error(CCMI_ERR_ARG, "%s: the source handle is NULL", who);
    if (!src->resident)
        return ccmi_set_error(CCMI_ERR_ARG, "%s: the source handle is plan-only (built without a store): no latents to measure", who);
    return CCMI_OK;
}

// A compaction up to the scan: the workspace, the job tables (host image kept for the pack),
// width pass and scan, the grids' payload words read back.
struct CompactRun {
    CompactPlan cp;
    uint8_t *dev = nullptr;
    bool owned = false;
    std::vector<DecLatSegJob> jobs;
    std::vector<uint32_t> words;
    ~CompactRun() { if (owned && dev) (void)hipFree(dev); }
};

int compact_measure(const ccmi_latents &src, void *workspace, size_t workspace_bytes, hipStream_t s, const char *who,
                    CompactRun &r)
{
    if (int rc = compact_layout(src, who, r.cp)) return rc;
    const CompactPlan &cp = r.cp;
    r.dev = static_cast<uint8_t *>(workspace);
    if (r.dev) {
        if (workspace_bytes < cp.total)
            return ccmi_set_error(CCMI_ERR_ARG, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, cp.total);
        if (reinterpret_cast<uintptr_t>(r.dev) % 256)
            return ccmi_set_error(CCMI_ERR_ARG, "%s: workspace must be 256-byte aligned", who);
    } else {
        CCMI_HIP_CHECK(hipMalloc(&r.dev, std::max<size_t>(cp.total, 256)));
        r.owned = true;
    }
    uint32_t *desc = reinterpret_cast<uint32_t *>(r.dev + cp.desc_off);
    r.jobs.resize(cp.grids.size());
    for (size_t g = 0; g < cp.grids.size(); ++g) {
        const CompactPlan::Grid &G = cp.grids[g];
        const LatentStream &S = src.s[G.stream];
        const FrameHost &f = S.f;
        r.jobs[g] = DecLatSegJob{S.base + S.grid_off[G.l], desc + G.first_seg, nullptr, nullptr, f.lw[G.l], f.lh[G.l],
                                 (int)dec_lat_seg_per_row(f.lw[G.l]), (int)dec_lat_elem_bytes(S.type), G.first_seg, 0};
    }
    r.words.assign(cp.grids.size(), 0);
    if (r.jobs.empty()) return CCMI_OK;
    const DecLatSegJob *d_jobs = reinterpret_cast<const DecLatSegJob *>(r.dev + cp.jobs_off);
    uint32_t *d_totals = reinterpret_cast<uint32_t *>(r.dev + cp.totals_off);
    CCMI_HIP_CHECK(hipMemcpyAsync(r.dev + cp.jobs_off, r.jobs.data(), sizeof(DecLatSegJob) * r.jobs.size(),
                                  hipMemcpyHostToDevice, s));
    if (int rc = launch_dec_lat_seg_width(d_jobs, (int)r.jobs.size(), cp.n_segs, s)) return rc;
    if (int rc = launch_dec_lat_seg_scan(d_jobs, (int)r.jobs.size(), d_totals, s)) return rc;
    CCMI_HIP_CHECK(hipMemcpyAsync(r.words.data(), d_totals, 4 * r.words.size(), hipMemcpyDeviceToHost, s));
    CCMI_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t g = 0; g < cp.grids.size(); ++g)
        if (r.words[g] == kSegTotalBad)
            return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "%s: stream %d, latent grid %d: a segment's word offset does not "
                                  "fit a descriptor's 29 bits", who, cp.grids[g].stream, cp.grids[g].l);
    return CCMI_OK;
}

} // namespace

extern "C" int ccmi_latents_compact_plan(const ccmi_latents *src, size_t *store_bytes_max, size_t *workspace_bytes)
{
    if (!src) return ccmi_set_error(CCMI_ERR_ARG, "latents_compact_plan: the source handle is NULL");
    if (!store_bytes_max || !workspace_bytes) return ccmi_set_error(CCMI_ERR_ARG, "latents_compact_plan: null argument");
    CompactPlan cp;
    if (int rc = compact_layout(*src, "latents_compact_plan", cp)) return rc;
    ccmi_latents out;
    seg_store_layout(*src, cp, nullptr, out);
    *store_bytes_max = out.store_bytes;
    *workspace_bytes = cp.total;
    return CCMI_OK;
}

extern "C" int ccmi_latents_compact_measure(const ccmi_latents *src, void *workspace, size_t workspace_bytes, void *stream,
                                            size_t *store_bytes, size_t *store_bytes_each)
{
    if (int rc = check_source(src, "latents_compact_measure")) return rc;
    if (!store_bytes) return ccmi_set_error(CCMI_ERR_ARG, "latents_compact_measure: null argument");
    CompactRun r;
    if (int rc = compact_measure(*src, workspace, workspace_bytes, static_cast<hipStream_t>(stream),
                                 "latents_compact_measure", r))
        return rc;
    ccmi_latents out;
    seg_store_layout(*src, r.cp, r.words.data(), out);
    *store_bytes = out.store_bytes;
    for (size_t i = 0; i < out.s.size() && store_bytes_each; ++i) store_bytes_each[i] = out.s[i].bytes;
    return CCMI_OK;
}

extern "C" int ccmi_latents_compact(const ccmi_latents *src, void *store, size_t store_bytes, void *workspace,
                                    size_t workspace_bytes, void *stream, ccmi_latents **out)
{
    if (out) *out = nullptr;
    if (int rc = check_source(src, "latents_compact")) return rc;
    if (!store || !out) return ccmi_set_error(CCMI_ERR_ARG, "latents_compact: null argument");
    if (reinterpret_cast<uintptr_t>(store) % 256)
        return ccmi_set_error(CCMI_ERR_ARG, "latents_compact: the store must be 256-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    CompactRun r;
    if (int rc = compact_measure(*src, workspace, workspace_bytes, s, "latents_compact", r)) return rc;
    ccmi_latents *h = new ccmi_latents;
    struct Drop {
        ccmi_latents *p;
        ~Drop() { delete p; }
    } drop{h};
    seg_store_layout(*src, r.cp, r.words.data(), *h);
    if (store_bytes < h->store_bytes)
        return ccmi_set_error(CCMI_ERR_ARG, "latents_compact: store of %zu bytes, need %zu", store_bytes, h->store_bytes);
    const CompactPlan &cp = r.cp;
    uint8_t *base = static_cast<uint8_t *>(store);
    for (size_t g = 0; g < cp.grids.size(); ++g) {
        const CompactPlan::Grid &G = cp.grids[g];
        const LatentStream &S = h->s[G.stream];
        uint8_t *table = base + S.grid_off[G.l];
        r.jobs[g].desc_out = reinterpret_cast<uint32_t *>(table);
        r.jobs[g].payload = reinterpret_cast<uint32_t *>(table + dec_lat_seg_table_bytes(S.f.lh[G.l], S.f.lw[G.l]));
    }
    // the networks' integers: a plain int32 copy, store to store
    std::vector<DecLatPackJob> copy;
    uint32_t copy_blocks = 0;
    for (size_t i = 0; i < src->s.size(); ++i) {
        const LatentStream &A = src->s[i], &B = h->s[i];
        const size_t from[2] = {A.ups_off, A.syn_off}, to[2] = {B.ups_off, B.syn_off};
        const size_t cnt[2] = {A.f.ups.size(), A.f.syn.size()};
        for (int k = 0; k < 2; ++k) {
            if (!cnt[k]) continue;
            copy.push_back(DecLatPackJob{reinterpret_cast<const int32_t *>(A.base + from[k]), base + to[k], nullptr,
                                         (uint32_t)cnt[k], copy_blocks, 0, 0});
            copy_blocks += dec_lat_pack_blocks((uint32_t)cnt[k], CCMI_LATENT_I32);
        }
    }
    if (!r.jobs.empty())
        CCMI_HIP_CHECK(hipMemcpyAsync(r.dev + cp.jobs_off, r.jobs.data(), sizeof(DecLatSegJob) * r.jobs.size(),
                                      hipMemcpyHostToDevice, s));
    if (!copy.empty())
        CCMI_HIP_CHECK(hipMemcpyAsync(r.dev + cp.copy_off, copy.data(), sizeof(DecLatPackJob) * copy.size(),
                                      hipMemcpyHostToDevice, s));
    if (int rc = launch_dec_lat_seg_pack(reinterpret_cast<const DecLatSegJob *>(r.dev + cp.jobs_off), (int)r.jobs.size(),
                                         cp.n_segs, s))
        return rc;
    if (int rc = launch_dec_lat_pack(reinterpret_cast<const DecLatPackJob *>(r.dev + cp.copy_off), (int)copy.size(),
                                     copy_blocks, CCMI_LATENT_I32, s))
        return rc;
    CCMI_HIP_CHECK(hipStreamSynchronize(s)); // the job tables are this call's: nothing may read them later
    h->resident = true;
    for (LatentStream &S : h->s) S.base = base;
    drop.p = nullptr;
    *out = h;
    return CCMI_OK;
}

extern "C" int ccmi_latents_concat(const ccmi_latents *const *parts, int n_parts, ccmi_latents **out)
{
    if (out) *out = nullptr;
    if (!parts || !out) return ccmi_set_error(CCMI_ERR_ARG, "latents_concat: null argument");
    if (n_parts < 1) return ccmi_set_error(CCMI_ERR_ARG, "latents_concat: no parts (n_parts < 1)");
    size_t count = 0;
    for (int k = 0; k < n_parts; ++k) {
        if (!parts[k]) return ccmi_set_error(CCMI_ERR_ARG, "latents_concat: part %d is NULL", k);
        if (parts[k]->resident != parts[0]->resident)
            return ccmi_set_error(CCMI_ERR_ARG, "latents_concat: part %d is %s and part 0 is not; plan-only and resident "
                                  "handles do not mix", k, parts[k]->resident ? "resident" : "plan-only");
        count += parts[k]->s.size();
        if (count > (size_t)INT_MAX)
            return ccmi_set_error(CCMI_ERR_ARG, "latents_concat: more than %d streams (part %d)", INT_MAX, k);
    }
    ccmi_latents *h = new ccmi_latents;
    h->resident = parts[0]->resident;
    h->s.reserve(count);
    for (int k = 0; k < n_parts; ++k) {
        h->s.insert(h->s.end(), parts[k]->s.begin(), parts[k]->s.end());
        h->store_bytes += parts[k]->store_bytes;
    }
    *out = h;
    return CCMI_OK;
}

extern "C" int ccmi_latents_stream_info(const ccmi_latents *h, int i, int *latent_type, size_t *store_bytes)
{
    if (!h) return ccmi_set_error(CCMI_ERR_ARG, "latents_stream_info: the handle is NULL");
    if (i < 0 || i >= (int)h->s.size())
        return ccmi_set_error(CCMI_ERR_ARG, "latents_stream_info: stream %d outside the handle's %zu streams", i, h->s.size());
    if (latent_type) *latent_type = h->s[i].type;
    if (store_bytes) *store_bytes = h->s[i].bytes;
    return CCMI_OK;
}
