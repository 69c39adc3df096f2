// The operands every BMU kernel reads are DERIVED from the codebook W and rebuilt lazily:
//   |w|^2 (wsq; with a patch order also wsq_p) | the patch-order copy Wp / wsq_p (exact mode) | the float32 stage / tile image, in
//   the units' own order or in patch order | the 16-bit stage / tile image with its norms wn, the wmax2 pair and Wst_lo |
//   the exact plan's centroids, radii and |c|^2.
// This header owns WHICH OF THEM ARE CURRENT: one State per handle, moved only by the named transitions below -- what happened to
// the codebook, what a reader asked for, what a launch took on.  Pure host code (no HIP, no handle), in the manner of
// exact_policy.hpp: somhip.hip launches what decide() lists and tells the state so; som_operands_replay (include/somhip_test.h)
// exposes the same object to the CPU suite, which checks it against a model of the buffers' versions (tests/test_operands_cpu.py).
// A mistake here fails silently -- a kernel reads last epoch's image and returns plausible BMUs -- hence the one owner.
#pragma once

namespace somhip {
namespace operands {

// fixed at som_create
struct Config {
    bool half = false;        // the configured search reads a 16-bit image (precision bf16 / f16 / exact)
    bool exact = false;       // ... and re-scores in float32: the float32 image and |w|^2 belong to the search as well
    bool patch = false;       // exact mode: its images are in patch order (Wp, wsq_p exist)
    bool cosine = false;      // the 16-bit image is scaled by 1 / |w|: |w|^2 is due whenever it is rebuilt
    bool resident = false;    // exact mode up to 128 features: norms step + image kernel, fused merge, deferred image
    bool f32_stage = false;   // a float32 stage image exists (up to 128 features): the exact fused merge writes it
    bool valid() const { return (!exact || half) && (!patch || exact) && (!resident || exact); }
};

// who is about to read
enum class Request {
    Search,        // the configured BMU search (f32: float32 operands; bf16 / f16: the 16-bit image; exact: as ExactScreen)
    F32Units,      // a float32 kernel that names units by their place in its image: |w|^2, the float32 image in the units' own order
    ExactScreen,   // the exact mode's screen + re-score: 16-bit image, |w|^2, the float32 image in patch order where there is one
};

// what a request has to rebuild, in launch order
struct Rebuilds {
    bool flush = false, flush_cm = false;   // a 16-bit image an earlier request deferred and no launch took: due first (cm as below)
    bool wsq = false;                       // |w|^2 (and wsq_p)
    bool permute = false;                   // Wp, wsq_p from W, wsq
    bool f32 = false, f32_patch = false;    // the float32 image(s), from the patch-order copy
    bool half = false;                      // the 16-bit image with its norms ...
    bool skip_norms = false;                //   resident exact: the fused merge left wn and the wmax2 pair: straight to the image kernel
    bool deferred = false;                  //   resident exact: the image kernel is left to the launch (take_pending_image)
    bool cm = false;                        //   resident exact: the image kernel also sets the centroid levels' maxima
    bool any() const { return wsq || permute || f32 || half; }   // (besides the flush)
};

class State {
public:
    State() = default;
    explicit State(const Config& c) : cfg(c) {}
    const Config& config() const { return cfg; }

    // ---- what happened to the codebook ----
    // REPLACED (som_set_weights; a graph capture starts, so that the graph holds every rebuild, or fails): nothing is current
    void codebook_replaced() {
        w_dirty = wsq_dirty = wf_dirty = wp_dirty = true;
        wn_fresh = false; cen_fresh = false;
        prep_w_pending = false;              // (an image owed for the old codebook is owed no more: w_dirty covers the new one)
    }
    // PLAIN MERGE (merge_kernel): it writes Wp beside W where Wp was in step (patch_copy_in_step(), asked BEFORE the launch)
    void merged_plain() {
        const bool keep = patch_copy_in_step();
        codebook_replaced();
        wp_dirty = !keep;
    }
    // HALF-FUSED MERGE (merge_prep_half): the 16-bit image and its norms are the new codebook's
    void merged_half_fused() { codebook_replaced(); w_dirty = false; }
    // EXACT FUSED MERGE (exact_merge_prep_kernel): |w|^2, Wp, the float32 stage image in the handle's order, wn and the maximum
    // (the wmax2 pair zeroed in front) are the new codebook's, the centroids where it wrote them; the 16-bit image stays owed
    void merged_exact_fused(bool centroids) {
        codebook_replaced();
        wsq_dirty = false; wp_dirty = false;
        if (cfg.f32_stage) { wf_dirty = false; wf_patch = cfg.patch; }
        wn_fresh = true;
        cen_fresh = centroids;
    }

    // ---- a reader ----
    // may_defer: the caller is the launch that can write the resident exact image in one grid with its plan's (run_activation_bmu_launch)
    Rebuilds decide(Request rq, bool may_defer = false) const {
        Rebuilds r;
        const bool need_f32 = rq != Request::Search || !cfg.half || cfg.exact;
        const bool patch = cfg.patch && (rq == Request::ExactScreen || (rq == Request::Search && cfg.exact));
        r.flush = prep_w_pending && !may_defer;
        r.flush_cm = r.flush && prep_w_cm;
        r.f32 = need_f32 && (wf_dirty || wf_patch != patch);
        r.f32_patch = r.f32 && patch;
        r.half = cfg.half && w_dirty;
        r.wsq = wsq_dirty && (need_f32 || (r.half && cfg.cosine));
        r.permute = cfg.patch && wp_dirty && (r.f32_patch || r.half);
        if (r.half && cfg.resident) {
            r.skip_norms = wn_fresh;
            r.deferred = may_defer;
            r.cm = cen_fresh;
        }
        return r;
    }
    // ... and what it listed has been launched
    void commit(const Rebuilds& r) {
        if (r.flush) prep_w_pending = false;
        if (r.wsq) wsq_dirty = false;
        if (r.permute) wp_dirty = false;
        if (r.f32) { wf_dirty = false; wf_patch = r.f32_patch; }
        if (r.half) {
            w_dirty = false;
            wn_fresh = false;                // (the image kernel leaves its error maximum in the pair: no second straight run)
            if (r.deferred) { prep_w_pending = true; prep_w_cm = r.cm; }
        }
    }
    // the canary reads |w|^2 alone
    Rebuilds decide_wsq() const { Rebuilds r; r.wsq = wsq_dirty; return r; }
    // GRAPH REPLAYED: the captured epoch began with everything stale (codebook_replaced) and rebuilt what rq needs from there
    void graph_replayed(Request rq) {
        State all_stale(cfg);
        commit(all_stale.decide(rq));
    }
    // THE PENDING IMAGE: taken by the planned launch (one grid with the centroid images) or flushed on its own; *cm as Rebuilds::cm
    bool take_pending_image(bool* cm) {
        if (!prep_w_pending) return false;
        prep_w_pending = false;
        *cm = prep_w_cm;
        return true;
    }

    // ---- read-only questions ----
    bool f32_in_patch_order() const { return wf_patch; }
    bool image_pending() const { return prep_w_pending; }
    bool centroids_fresh() const { return cen_fresh; }   // the fused merge wrote centroids, radii, |c|^2 for this codebook
    bool patch_copy_in_step() const { return cfg.patch && !wp_dirty; }

private:
    Config cfg;
    bool w_dirty = true, wsq_dirty = true, wf_dirty = true, wp_dirty = true;   // 16-bit image | |w|^2 | float32 image | Wp
    bool wf_patch = false;        // the order the float32 image is in
    bool wn_fresh = false;        // resident exact: wn, wmax2[0] = max |w|^2 are this codebook's and wmax2[1] is zeroed
    bool cen_fresh = false;
    bool prep_w_pending = false, prep_w_cm = false;
};

}  // namespace operands
}  // namespace somhip
