// precision 'exact': the HOST side of the screen + re-score pipeline (bmu_exact.hpp), of block skipping (exact_skip.hpp,
// exact_skip_wide.hpp) and of the scout -- launch geometry, the per-pass kernel sequence, and the reserve of the scratch's four owners
// (PassScratch, PlanScratch, CentroidSet, SortedRows: somhip.hip), which allocate what exact_scratch.hpp's rule says and nothing else.
// Included by somhip.hip INSIDE its anonymous namespace, behind the handle (som_handle, ExactScratch) and the helpers it uses
// (DevBuf, kernel_per_cu, resident_slots, choose_parts, refresh_codebook_operands, launch_bmu_f32_any, Timed, HIPCHK ...): one
// translation unit, two files.  What a launch DECIDES -- plan at all, re-sort, scout, level 2, refine -- and the state those
// decisions move (pause ladder, re-sort schedule, level-2 probe, measured costs) is policy::PlanState in exact_policy.hpp: pure
// host arithmetic, unit-tested without a GPU (som_policy_eval, som_policy_replay: include/somhip_test.h).  launch_bmu_exact
// gathers the facts of a launch, acts on the LaunchPlan it gets back and reports what the launch measured.
// (no #pragma once / include guard on purpose: not a header of its own)

// ---- precision 'exact' (bmu_exact.hpp): screen -> candidate groups -> float32 re-score -> float32 fallback ----------
// E(n) = cA |x_n| wmax + cW wmax^2 + cB Bm in d' units; derivation in bmu_exact.hpp.  KAPPA ulps are charged per MFMA.
// the pass's counter block (PassScratch::ctr; layout and the tail's slots: PassCounters, bmu_exact.hpp) by name
struct PassCtr {
    int* base; int n_groups; bool whole_lines;
    int* gcount() const { return base; }
    int* gstart() const { return base + n_groups; }
    PassCounters* tail() const { return (PassCounters*)(gstart() + n_groups); }
    RowNeed* row_need() const { return (RowNeed*)base; }          // (before a launch's first pass: exact_scout_rowneed_kernel)
    // what a pass zeroes (whole_lines: up to the next multiple of 64 bytes -- the allocation has the room, EX_CTR_TAIL_INTS.  The fill of the exact
    //  size, 8 232 bytes at 1 024 groups, shows as two fill kernels in the kernel trace, the padded one as one:
    //  profiles/exact_chain_summary.md; SOM_EXACT_CHAIN=0: the exact size)
    size_t bytes() const {
        const size_t b = 2 * (size_t)n_groups * sizeof(int) + sizeof(PassCounters);
        return whole_lines ? (size_t)round_up((long)b, 64) : b;
    }
};
inline PassCtr pass_ctr(const som_handle* h) { return PassCtr{h->ex.pass.ctr, (int)cdiv(h->K, EX_GROUP), h->ex.sw.chain}; }

constexpr double EX_KAPPA = 6.0;     // measured through som_debug_mfma16: <= 2.4 (tests/test_gpu_exact.py holds it below 3)
ExactBound exact_bound(const som_handle* h) {
    const double u = std::ldexp(1.0, -24);
    // chain length of the float32 kernel (zero padded), MFMAs of the screen's one accumulator chain
    const double Dl = h->wide ? 32.0 * h->ft_kchunks : 8.0 * h->fr_kg;
    const double n_mfma = h->wide ? h->n_kchunks : h->ks32;
    const double gamma = Dl * u / (1.0 - Dl * u);
    const double slop = 1.01;                             // the kernel evaluates E in float32
    ExactBound eb{};
    // one pass on scaled half operands, measured operand errors (bmu_exact.hpp); +1: the initial accumulator's rounding
    eb.cB = (float)(slop * 2.0 * (EX_KAPPA * n_mfma + 1.0) * std::ldexp(1.0, -23));
    eb.cM = (float)(slop * 2.0);
    if (h->cfg.distance == SOM_DIST_COSINE) {
        // scores 1 - cos: the float32 kernel's chain (gamma_D), its two pairwise |.|^2 sums, product, sqrt, division and
        // subtraction (< 27 u together); the screen's two normalisations 1/sqrt(|.|^2) and their products (< 30 u)
        eb.cA = (float)(slop * 2.0 * (gamma + 57.0 * u));
        eb.cW = 0.0f;
        eb.unit = 1;
    } else {
        eb.cA = (float)(slop * (2.0 * gamma + 2.0 * u) * (1.0 + u));   // float32 kernel, relative to A (tau units)
        eb.cW = (float)(slop * u);
    }
    return eb;
}

// ---- the scratch (exact_scratch.hpp): what the handle sizes by, and the pass scratch's reserve ---------------------------------------
exscratch::Geometry exact_geometry(const som_handle* h) {
    // (item_slots: more workgroups than eight a CU never fit a chip: few features, small stages)
    return exscratch::Geometry{h->K, h->D, h->dp, h->stage_bytes, h->wide, (int)resident_slots(h, 8), h->ex.hook.pass_rows_override, h->ex.hook.pairs};
}

// (the screens write group minima and row masks for whole workgroup tiles: a pass's row stride must hold them)
static_assert(256 % K16_WG_SAMPLES == 0 && 256 % WD_WG_SAMPLES == 0 && K16_WG_SAMPLES % 64 == 0 && WD_WG_SAMPLES % 64 == 0,
              "exact: the pass stride (a multiple of 256 rows) must be a whole number of screen workgroup tiles");

int reserve(som_handle* h, PassScratch& p, const exscratch::PassSizes& z) {
    p.release();
    if (z.too_large) return fail(h, "exact: pass too large");
    int rc = p.gmin.alloc(h, z.gmin);
    if (!rc) rc = p.gflags.alloc(h, z.gflags);
    for (DevBuf<int>* b : {&p.rowcnt, &p.rowarg}) if (!rc) rc = b->alloc(h, z.rowcnt);
    if (!rc) rc = p.seed.alloc(h, z.seed);
    if (!rc) rc = p.plist.alloc(h, z.plist);
    if (!rc) rc = p.fb_list.alloc(h, z.fb_list);
    if (!rc) rc = p.tile_tab.alloc(h, z.tile_tab);
    if (!rc) rc = p.ctr.alloc(h, z.ctr);
    if (rc) p.release();
    else { p.stride = z.stride; p.pairs = z.pairs; p.max_tiles = z.max_tiles; }
    return rc;
}

// the pass scratch for `rows` rows, down the stride ladder of exact_scratch.hpp where the device refuses a pass
int exact_reserve(som_handle* h, long rows) {
    auto& ex = h->ex;
    const exscratch::Geometry g = exact_geometry(h);
    long stride = exscratch::first_stride(g, rows, ex.stride_cap);
    if (stride <= ex.pass.stride) return 0;
    if (!ex.pass_host) HIPCHK(h, hipHostMalloc((void**)&ex.pass_host, sizeof(PassCounters), hipHostMallocDefault));
    for (;;) {
        // TEST HOOK (tests/test_gpu_exact.py; SOM_TEST_HOOKS=1): behave as a device that refuses the scratch of passes above n rows
        const bool hooked = ex.hook.refuse_above > 0 && stride > ex.hook.refuse_above;
        if (!hooked) ex.plan.order_lost();               // (the resident order was built pass by pass: new passes, new order)
        const int rc = hooked ? fail(h, "exact: pass scratch refused (test hook)") : reserve(h, ex.pass, exscratch::pass(g, stride));
        if (rc == 0) return 0;
        stride = exscratch::next_stride(stride);
        if (stride == 0) return rc;                      // (the message of the last failed allocation stands)
        (void)hipGetLastError();
        ex.stride_cap = stride;                          // launch_bmu_exact walks passes of this many rows from now on
        if (h->debug) std::fprintf(stderr, "[somhip] exact: pass scratch refused, retrying with passes of %ld rows\n", stride);
    }
}

template <int KS32>
int exact_screen(som_handle* h, const __bf16* Xb, long n, unsigned long long* best64, const float* xsq, const float* xerr,
                 const float* xmax2, const ExactBound& eb, const float* seed, const int* glist, const int* gcnt,
                 const ScreenSelect& sel, bool* selected) {
    // sel: the select tail's arguments (plist null: none wanted); *selected: did this launch select -- only the work queue can
    *selected = false;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    // one pass on scaled half operands: a stage IS a group
    const bool tl = glist != nullptr;
    const void* kern = tl ? (const void*)bmu_bf16_k16_kernel<KS32, ExactEl, true, true> : (const void*)bmu_bf16_k16_kernel<KS32, ExactEl, true, false>;
    size_t lds = 2 * (size_t)k16_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, kern, 64 * K16_NW, lds, &per_cu)) return rc;
    const long blocks = cdiv(n, K16_WG_SAMPLES);
    const long slots = resident_slots(h, per_cu);
    int parts = choose_parts(h, blocks, slots, h->n_stages);
    if (tl && blocks >= slots) {
        // a tile's list is short where the plan works (tens of items of 1 024): every part of a tile loads the tile's 64 KB
        // of rows again, so the scan is split only where the lists are long enough to carry that (the last plan's share
        // is the forecast; 1 Mi rows, mid-schedule: three parts re-read 0.8 GB for 0.3 ms of screen)
        const double tiles16 = h->ex.share_forecast * (double)n_groups * K16_T;
        parts = tiles16 < 128.0 ? 1 : tiles16 < 320.0 ? std::min(parts, 2) : parts;
    }
    if (h->env_bf16_parts > 0) parts = std::min(h->env_bf16_parts, h->n_stages);
    if (h->debug)
        std::fprintf(stderr, "[somhip] exact screen: blocks=%ld per_cu=%d slots=%ld parts=%d groups=%d lists=%d\n", blocks, per_cu,
                     slots, parts, n_groups, tl ? 1 : 0);
    const dim3 grid((unsigned)blocks, (unsigned)parts), block(64 * K16_NW);
    if (tl && h->ex.sw.item_queue && glist == h->ex.pbuf.tlist) {
        // (the plan's lists as a work queue: a workgroup per slot of the chip, items of about equal length -- bmu_bf16_k16.hpp;
        //  the next plan cuts its lists for this many workgroups)
        // (sel, where the pass asks for it: the workgroup that ends a tile selects its rows' candidates too -- the select tail of
        //  bmu_bf16_k16.hpp; *selected tells the pass that exact_select_kernel has nothing left to do)
        h->ex.screen_slots = (int)std::min<long>(slots, h->ex.pbuf.item_slots);
        bmu_bf16_k16_kernel<KS32, ExactEl, true, true><<<dim3((unsigned)h->ex.screen_slots), block, lds, h->stream>>>(
            Xb, n, h->Wst, h->n_stages, h->K, best64, h->ex.pass.gmin, h->ex.pass.stride, h->ex.pass.gflags, xsq, xerr, xmax2, h->wmax2, h->wmax2 + 1, eb,
            seed, glist, gcnt, h->ex.pbuf.items + 8, (const int*)h->ex.pbuf.items.p, (int*)h->ex.pbuf.items.p + 1, nullptr, 0, sel);
        *selected = sel.plist != nullptr;
    } else if (tl)
        bmu_bf16_k16_kernel<KS32, ExactEl, true, true><<<grid, block, lds, h->stream>>>(
            Xb, n, h->Wst, h->n_stages, h->K, best64, h->ex.pass.gmin, h->ex.pass.stride, h->ex.pass.gflags, xsq, xerr, xmax2, h->wmax2, h->wmax2 + 1, eb,
            seed, glist, gcnt);
    else
        bmu_bf16_k16_kernel<KS32, ExactEl, true, false><<<grid, block, lds, h->stream>>>(
            Xb, n, h->Wst, h->n_stages, h->K, best64, h->ex.pass.gmin, h->ex.pass.stride, h->ex.pass.gflags, xsq, xerr, xmax2, h->wmax2, h->wmax2 + 1, eb,
            seed, nullptr, nullptr);
    return 0;
}

// beyond 128 features: the wide kernel's GM instance (groups = pairs of its 32-unit stages)
template <int KS32>
int exact_screen_wide(som_handle* h, const __bf16* Ximg, long n, unsigned long long* best64, const float* xsq, const float* xerr,
                      const float* xmax2, const ExactBound& eb, const int* glist = nullptr, const int* gcnt = nullptr) {
    if (glist != nullptr) {
        // under a plan (exact_skip_wide.hpp): every workgroup walks its tile's list of groups; parts where the lists are long
        auto kern = bmu_bf16_wide_kernel<KS32, ExactEl, true, true>;
        const size_t lds = (size_t)WD_SLOTS * wd_stage_bytes(KS32);
        int per_cu = 1;
        if (int rc = kernel_per_cu(h, (const void*)kern, 64 * WD_NW, lds, &per_cu)) return rc;
        const long blocks = cdiv(n, WD_WG_SAMPLES);
        const long slots = resident_slots(h, per_cu);
        const int n_groups = (int)cdiv(h->n_stages, 2);
        const double groups_forecast = h->ex.share_forecast * (double)n_groups;
        int parts = blocks >= slots ? (groups_forecast < 64.0 ? 1 : groups_forecast < 256.0 ? 2 : 4)
                                    : (int)std::min<long>(cdiv(slots, blocks), 16);
        if (h->env_bf16_parts > 0) parts = h->env_bf16_parts;
        parts = std::max(1, std::min(parts, n_groups));
        if (h->debug)
            std::fprintf(stderr, "[somhip] exact screen (wide, lists): blocks=%ld per_cu=%d slots=%ld parts=%d groups=%d\n", blocks, per_cu, slots, parts, n_groups);
        if (h->ex.sw.item_queue && glist == h->ex.pbuf.glist) {
            // (the plan's lists as a work queue: a workgroup per slot of the chip -- bmu_bf16_wide.hpp; the next plan cuts for this many)
            h->ex.screen_slots = (int)std::min<long>(slots, h->ex.pbuf.item_slots);
            bmu_bf16_wide_kernel<KS32, ExactEl, true, true><<<dim3((unsigned)h->ex.screen_slots), dim3(64 * WD_NW), lds, h->stream>>>(
                (const char*)Ximg, n, h->Wst, h->n_stages, best64, h->ex.pass.gmin, h->ex.pass.stride, (uint32_t*)h->ex.pass.gflags.p, xsq, xerr, xmax2,
                h->wmax2, h->wmax2 + 1, eb, glist, gcnt, n_groups, nullptr, nullptr, nullptr, 0, h->ex.pbuf.items + 8, (const int*)h->ex.pbuf.items.p,
                (int*)h->ex.pbuf.items.p + 1);
            return 0;
        }
        bmu_bf16_wide_kernel<KS32, ExactEl, true, true><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * WD_NW), lds, h->stream>>>(
            (const char*)Ximg, n, h->Wst, h->n_stages, best64, h->ex.pass.gmin, h->ex.pass.stride, (uint32_t*)h->ex.pass.gflags.p, xsq, xerr, xmax2,
            h->wmax2, h->wmax2 + 1, eb, glist, gcnt, n_groups);
        return 0;
    }
    auto kern = bmu_bf16_wide_kernel<KS32, ExactEl, true>;
    const size_t lds = (size_t)WD_SLOTS * wd_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 64 * WD_NW, lds, &per_cu)) return rc;
    const long blocks = cdiv(n, WD_WG_SAMPLES);
    const long slots = resident_slots(h, per_cu);
    const int n_groups = (int)cdiv(h->n_stages, 2);
    int parts = 1;
    if (blocks < slots) parts = (int)std::min<long>(cdiv(slots, blocks), 64);
    else {
        double best_eff = 0.0;
        for (int p = 1; p <= 8; ++p) {
            const long wgs = blocks * p;
            const double eff = (double)wgs / (double)(cdiv(wgs, slots) * slots);
            if (eff > best_eff + 0.01) { best_eff = eff; parts = p; }
        }
    }
    if (h->env_bf16_parts > 0) parts = h->env_bf16_parts;
    parts = std::max(1, std::min(parts, n_groups));
    if (h->debug)
        std::fprintf(stderr, "[somhip] exact screen (wide): blocks=%ld per_cu=%d slots=%ld parts=%d groups=%d\n", blocks, per_cu, slots,
                     parts, n_groups);
    bmu_bf16_wide_kernel<KS32, ExactEl, true><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * WD_NW), lds, h->stream>>>(
        (const char*)Ximg, n, h->Wst, h->n_stages, best64, h->ex.pass.gmin, h->ex.pass.stride, (uint32_t*)h->ex.pass.gflags.p, xsq, xerr, xmax2,
        h->wmax2, h->wmax2 + 1, eb);
    return 0;
}

int exact_screen_ks(som_handle* h, const __bf16* Xb, long n, unsigned long long* best64, const float* xsq, const float* xerr,
                    const float* xmax2, const ExactBound& eb, const float* seed, const int* glist, const int* gcnt,
                    const ScreenSelect& sel, bool* selected) {
    *selected = false;
    if (h->wide)
        return for_kchunks(h, "exact: no wide screen instance for this input_len", [&](auto k) {
            return exact_screen_wide<decltype(k)::value>(h, Xb, n, best64, xsq, xerr, xmax2, eb, glist, gcnt); });
    return for_ks32(h, "exact: the screen kernel supports input_len <= 128", [&](auto k) {
        return exact_screen<decltype(k)::value>(h, Xb, n, best64, xsq, xerr, xmax2, eb, seed, glist, gcnt, sel, selected); });
}

// ---- block skipping (exact_skip.hpp): buffers, the centroid images, the sorted pass, the scout, a pass's plan -----------------
int reserve(som_handle* h, CentroidSet& cs, const exscratch::Geometry& g) {
    if (cs.ready) return 0;
    cs.release();
    const auto zero = [&](char* p, size_t n) { const hipError_t e = hipMemsetAsync(p, 0, n, h->stream); return e == hipSuccess ? 0 : fail_hip(h, "hipMemsetAsync", e); };
    int rc = 0;
    for (int lv = 0; lv < exscratch::levels(g) && !rc; ++lv) {
        const exscratch::CentroidSizes z = exscratch::centroids(g, lv);
        auto& c = cs.lv[lv];
        c.n_slots = z.n_slots; c.n_cstages = z.n_cstages; c.n_img_stages = z.n_img_stages;
        rc = c.Cc.alloc(h, z.Cc);
        if (!rc) rc = c.rg.alloc(h, z.rg);
        if (!rc) rc = c.csq.alloc(h, z.csq);
        if (!rc) rc = c.cmax2.alloc(h, z.cmax2);
        if (!rc) rc = c.Cst.alloc(h, z.Cst);
        if (!rc) rc = zero(c.Cst, z.Cst);
        if (!rc && z.Cst_plain > 0) {
            rc = c.Cst_plain.alloc(h, z.Cst_plain);
            if (!rc) rc = zero(c.Cst_plain, z.Cst_plain);
        }
    }
    if (rc) cs.release(); else cs.ready = true;
    return rc;
}

// (*order_lost: the RESIDENT rows' buffers were replaced -- the caller tells the policy)
int reserve(som_handle* h, SortedRows& sr, const exscratch::SortedSizes& z, bool* order_lost) {
    if (z.cap <= sr.cap) return 0;
    // (kernels of an earlier launch may still read the old copies: a transient set's buffers are reused launch after launch)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sr.release();
    *order_lost = sr.resident;
    int rc = sr.order.alloc(h, z.order);
    if (!rc) rc = sr.Xb_s.alloc(h, z.Xb_s);
    // (sr.Xl_s, the rows' second half image: reserve_second_half, the first launch whose refinement pass engages)
    if (!rc) rc = sr.Xf_s.alloc(h, z.Xf_s);
    for (DevBuf<float>* b : {&sr.xsq_s, &sr.xerr_s, &sr.seed_s, &sr.sU_s}) if (!rc) rc = b->alloc(h, z.xsq_s);   // (a float a position each)
    if (!rc) rc = sr.lastpos_s.alloc(h, z.lastpos_s);
    if (rc) sr.release(); else sr.cap = z.cap;
    return rc;
}
int reserve_second_half(som_handle* h, SortedRows& sr) { return sr.Xl_s.alloc(h, exscratch::sorted(exact_geometry(h), sr.cap).Xl_s); }

int reserve(som_handle* h, PlanScratch& p, const exscratch::PlanSizes& z) {
    if (z.stride <= p.stride) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    p.release();
    int rc = 0;
    for (DevBuf<int>* b : {&p.sk_keys, &p.sk_keys2, &p.sk_vals, &p.scout_g}) if (!rc) rc = b->alloc(h, z.sk_keys);   // (an int a row each)
    if (!rc && z.tq > 0) rc = p.tq.alloc(h, z.tq);
    if (!rc) rc = p.need.alloc(h, z.need);
    if (!rc) rc = p.need2.alloc(h, z.need2);
    if (!rc) rc = p.glist.alloc(h, z.glist);
    if (!rc) rc = p.gcnt.alloc(h, z.gcnt);
    if (!rc) rc = p.tile_counts.alloc(h, z.tile_counts);
    if (!rc) rc = p.tlist.alloc(h, z.tlist);
    for (DevBuf<int>* b : {&p.tcnt, &p.tile_ticket}) if (!rc) rc = b->alloc(h, z.tcnt);
    if (!rc) rc = p.items.alloc(h, z.items);
    if (!rc) rc = p.sk_tmp.alloc(h, z.sk_tmp);
    if (rc) p.release();
    else { p.stride = z.stride; p.item_slots = z.item_slots; }
    return rc;
}

// sr: the sorted copies to (re)size for `rows` positions; stride: rows of one pass (the plan's own buffers)
int exact_skip_reserve(som_handle* h, SortedRows& sr, long rows, long stride) {
    auto& ex = h->ex;
    // TEST HOOK (tests/test_gpu_exact.py): behave as a device without memory for the sorted pass
    if (ex.hook.refuse_skip) return fail(h, "exact: block-skipping scratch refused (test hook)");
    const exscratch::Geometry g = exact_geometry(h);
    if (int rc = reserve(h, ex.cen, g)) return rc;
    bool order_lost = false;
    const int rc = reserve(h, sr, exscratch::sorted(g, rows), &order_lost);
    if (order_lost) ex.plan.order_lost();
    return rc ? rc : reserve(h, ex.pbuf, exscratch::plan(g, stride));
}

// centroids and radii of the groups and of their sub-blocks under the current codebook, the centroids' scaled half images
// and initial accumulators
// (q_blocks > 0: the launch's prep_wsqh_kernel is still due as well -- best64, n_rows: its merge keys -- and rides along where the
//  images go out in one grid; *q_done says whether it did)
int exact_skip_centroids(som_handle* h, const float* xmax2, unsigned q_blocks, unsigned long long* best64, long n_rows, bool* q_done) {
    auto& ex = h->ex;
    const float* Wsrc = h->ex_patch ? h->Wp : h->W;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    auto& c0 = ex.cen.lv[0];
    auto& c1 = ex.cen.lv[1];
    const CentroidLevel l1{c0.Cc, c0.rg, c0.csq, c0.cmax2, c0.n_slots}, l2{c1.Cc, c1.rg, c1.csq, c1.cmax2, c1.n_slots};
    // two launches for both levels: centroids + radii + |c|^2, then the stage images with their tails (the images take the
    // codebook's own power of two: a centroid is no longer than the longest unit)
    // (fresh centroids: the fused merge has written the first launch's outputs for this codebook -- exact_merge_prep_kernel)
    if (!h->ops.centroids_fresh())
        exact_centroids_kernel<<<dim3((unsigned)(cdiv(n_groups, 4) * 4)), dim3(512), 0, h->stream>>>(Wsrc, h->K, h->D, n_groups, l1, l2, h->wmax2);
    const int nst2 = ex.lp.level2 ? c1.n_cstages : 0;
    char* plain = ex.lp.scout ? c0.Cst_plain : nullptr;
    const dim3 tgrid((unsigned)cdiv((long)(c0.n_cstages + nst2) * K16_T, 4)), block(256);
    bool cm = false;
    if (h->ops.take_pending_image(&cm)) {
        // (the codebook's own 16-bit image is still due -- refresh_codebook_operands left it to this launch: both in one grid)
        const float* Wex = h->ex_patch ? h->Wp : h->W;
        // (cm: centroids the fused merge wrote -- their levels' maxima are due now that max |w|^2 is final; the error maxima it zeroed)
        float* cm1 = cm ? (float*)c0.cmax2 : nullptr;
        float* cm2 = cm ? (float*)c1.cmax2 : nullptr;
        const unsigned w_blocks = (unsigned)cdiv((long)h->n_stages * K16_T, 4);
        switch (h->ks32) {
#define SOM_PIMG_CASE(k) case k: exact_prep_images_kernel<k, ExactEl><<<dim3(w_blocks + tgrid.x + q_blocks), block, 0, h->stream>>>(w_blocks, tgrid.x, Wex, h->K, h->D, h->Wst, h->n_stages, \
            h->wmax2 + 1, h->Wst_lo, cm1, cm2, l1, c0.Cst, c0.n_cstages, l2, c1.Cst, nst2, xmax2, h->wmax2, plain, h->wn, h->stage_units, best64, n_rows); break;
        SOM_PIMG_CASE(1) SOM_PIMG_CASE(2) SOM_PIMG_CASE(3) SOM_PIMG_CASE(4)
#undef SOM_PIMG_CASE
        default: return fail(h, "exact: block skipping supports input_len <= 128");
        }
        HIPCHK(h, hipGetLastError());
        *q_done = q_blocks > 0;
        return 0;
    }
    switch (h->ks32) {
#define SOM_CIMG_CASE(k) case k: exact_centroid_image_kernel<k, ExactEl><<<tgrid, block, 0, h->stream>>>(l1, c0.Cst, c0.n_cstages, l2, c1.Cst, nst2, h->D, xmax2, h->wmax2, plain); break;
    SOM_CIMG_CASE(1) SOM_CIMG_CASE(2) SOM_CIMG_CASE(3) SOM_CIMG_CASE(4)
#undef SOM_CIMG_CASE
    default: return fail(h, "exact: block skipping supports input_len <= 128");
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// (re-)sort one pass: the rows [r0, r0 + n) of the row set in the order of their last BMU's group (prev: last epoch's ids) or
// of their nearest group centroid (scout_g: the scout's): the order (position -> row) into sr at s0, the sorted keys into sk_keys2
int exact_skip_sortkeys(som_handle* h, SortedRows& sr, long s0, long n, const int* prev, const int* scout_g) {
    auto& ex = h->ex;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    if (scout_g != nullptr)
        exact_groupkey_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(scout_g, n, n_groups, ex.pbuf.sk_keys, ex.pbuf.sk_vals);
    else
        exact_sortkey_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(prev, h->ex_inv, n, h->K, ex.pbuf.sk_keys, ex.pbuf.sk_vals);
    return radix_sort_rows(h, ex.pbuf.sk_keys, n, unitsort::key_bits(n_groups), ex.pbuf.sk_keys2, sr.order + s0, ex.pbuf.sk_tmp);
}
// ... and the operands gathered in that order (`order`: n positions -> rows of the pass) into sr at positions s0 ...
int exact_skip_gather(som_handle* h, SortedRows& sr, long s0, const int* order, const float* X, const __bf16* Xb, long n,
                      const float* xsq, const float* xerr, const float* xmax2) {
    const long np = round_up(n, SK_TILE);
    exact_gather_sorted_kernel<ExactEl><<<dim3((unsigned)cdiv(np, 16)), dim3(256), 0, h->stream>>>(
        order, n, np, h->dp, h->D, Xb, X, xsq, xerr, xmax2, sr.Xb_s + s0 * h->dp, sr.Xl_s != nullptr ? sr.Xl_s + s0 * h->dp : nullptr, sr.Xf_s + s0 * h->D,
        sr.xsq_s + s0, sr.xerr_s + s0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the scout, step 1: every row's nearest group centroid (the plain resident kernel on the plain level-1 centroid image)
template <int KS32>
int exact_scout_nearest_ks(som_handle* h, const __bf16* Xb, long n, unsigned long long* best64, int* g_out) {
    auto& ex = h->ex;
    const auto& c0 = ex.cen.lv[0];
    const void* kern = (const void*)bmu_bf16_k16_kernel<KS32, ExactEl, false, false>;
    const size_t lds = 2 * (size_t)k16_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, kern, 64 * K16_NW, lds, &per_cu)) return rc;
    const long blocks = cdiv(n, K16_WG_SAMPLES);
    const long slots = resident_slots(h, per_cu);
    const int parts = std::max(1, std::min(choose_parts(h, blocks, slots, c0.n_cstages), c0.n_cstages));
    bmu_bf16_k16_kernel<KS32, ExactEl, false, false><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * K16_NW), lds, h->stream>>>(
        Xb, n, c0.Cst_plain, c0.n_cstages, c0.n_slots, best64);
    bmu_finalize_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(best64, n, c0.n_slots, g_out);
    HIPCHK(h, hipMemsetAsync(best64, 0xFF, (size_t)n * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipGetLastError());
    return 0;
}
int exact_scout_nearest(som_handle* h, const __bf16* Xb, long n, unsigned long long* best64, int* g_out) {
    return for_ks32(h, "exact: the scout supports input_len <= 128",
                    [&](auto k) { return exact_scout_nearest_ks<decltype(k)::value>(h, Xb, n, best64, g_out); });
}

// the scout, step 3: per tile of the SORTED pass the groups of its rows' keys (`keys`: the pass's sorted keys), the plain
// kernel over those groups' units with indices kept: the best of them -> lastpos (the pseudo last BMU)
template <int KS32>
int exact_scout_pick_ks(som_handle* h, SortedRows& sr, long s0, long n, const int* keys, unsigned long long* best64) {
    auto& ex = h->ex;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    const long tiles = round_up(n, SK_TILE) / SK_TILE;
    const size_t lds_l = (size_t)cdiv(n_groups, 64) * sizeof(unsigned long long);
    exact_scout_lists_kernel<<<dim3((unsigned)tiles), dim3(64), lds_l, h->stream>>>(keys, nullptr, n, n_groups, ex.pbuf.tlist, ex.pbuf.tcnt);
    const void* kern = (const void*)bmu_bf16_k16_kernel<KS32, ExactEl, false, true>;
    const size_t lds = 2 * (size_t)k16_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, kern, 64 * K16_NW, lds, &per_cu)) return rc;
    bmu_bf16_k16_kernel<KS32, ExactEl, false, true><<<dim3((unsigned)tiles, 1), dim3(64 * K16_NW), lds, h->stream>>>(
        sr.Xb_s + s0 * h->dp, n, h->Wst, h->n_stages, h->K, best64, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ExactBound(),
        nullptr, ex.pbuf.tlist, ex.pbuf.tcnt);
    exact_scout_pos_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(best64, n, h->K, sr.lastpos_s + s0);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int exact_scout_pick(som_handle* h, SortedRows& sr, long s0, long n, const int* keys, unsigned long long* best64) {
    return for_ks32(h, "exact: the scout supports input_len <= 128",
                    [&](auto k) { return exact_scout_pick_ks<decltype(k)::value>(h, sr, s0, n, keys, best64); });
}

// the need bitmaps of a pass's plan -> the tiles' lists, their totals and the screen's work queue (the lists cut into items of
// about equal length): one launch whose last workgroup does the totals (SOM_EXACT_CHAIN=0: two launches)
void exact_plan_lists(som_handle* h, long tiles, int n_cstages, const unsigned long long* need2) {
    auto& ex = h->ex;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    PassCounters* const ctr = pass_ctr(h).tail();
    const int slots = ex.sw.item_queue ? (ex.screen_slots > 0 ? ex.screen_slots : ex.pbuf.item_slots) : 0;
    int2* const queue = ex.sw.item_queue ? ex.pbuf.items + 8 : nullptr;   // (items[0] = (n_items, counter): the queue's two words)
    int* const n_items = (int*)ex.pbuf.items.p;
    if (ex.sw.chain) {
        exact_lists_totals_kernel<<<dim3((unsigned)cdiv(tiles, LISTS_WG_TILES)), dim3(64 * LISTS_WG_TILES), 0, h->stream>>>(
            ex.pbuf.need, n_cstages, need2, n_groups, ex.pbuf.glist, ex.pbuf.gcnt, ex.pbuf.tile_counts, ex.pbuf.tlist, ex.pbuf.tcnt, tiles, &ctr->lists_done,
            &ctr->blocks_run, &ctr->groups_run, slots, queue, n_items, n_items + 1, ex.sw.item_len_pct, ex.pbuf.tile_ticket);
        return;
    }
    exact_lists_kernel<<<dim3((unsigned)tiles), dim3(64), 0, h->stream>>>(ex.pbuf.need, n_cstages, need2, n_groups, ex.pbuf.glist, ex.pbuf.gcnt,
                                                                         ex.pbuf.tile_counts, ex.pbuf.tlist, ex.pbuf.tcnt, ex.pbuf.tile_ticket);
    exact_list_totals_kernel<<<dim3(1), dim3(1024), 0, h->stream>>>(ex.pbuf.tile_counts, tiles, &ctr->blocks_run, &ctr->groups_run, slots, queue,
                                                                  n_items, n_items + 1, ex.sw.item_len_pct);
}

// (every ExactEl instance of the plan kernels is built both ways -- the threshold folded into the extra MFMA step, ex.sw.plan_fold, and
//  compared against P, SOM_EXACT_PLAN_FOLD=0 -- and every one of exact_plan_fused_kernel keeps three workgroups a CU without scratch)
// one pass's plan on the sorted rows sr[s0, s0 + n): level 1 (+ the seeds, from lastpos_s), level 2, the tiles' item lists
// -- in ONE launch (exact_plan_fused_kernel) where the pass is planned with level 2, from last BMUs alone (no scout), by one
// workgroup per tile, and the policy does not time level 2 in this launch (time_l2: the split pair keeps cost.ev[3] .. ev[4]
// around level 2, so that policy::Costs is fed as before); SOM_EXACT_FUSE_PLAN=0 / SOM_EXACT_CHAIN=0: always the split sequence
int exact_skip_plan(som_handle* h, SortedRows& sr, long s0, long n, const float* xmax2, const ExactBound& eb,
                    const int* lastpos2, bool time_l2 = false) {
    auto& ex = h->ex;
    PassCounters* const ctr = pass_ctr(h).tail();
    const long np = round_up(n, SK_TILE);
    const long tiles = np / SK_TILE;
    // (the select kernel walks the tiles' lists too: the masks of the blocks the screen does not run are never read)
    const dim3 block(64 * K16_NW);
    const auto& c0 = ex.cen.lv[0];
    const auto& c1 = ex.cen.lv[1];
    // (few tiles: their centroid stages split over up to four workgroups each, so that the plan fills the chip)
    const long want = (1024 + tiles - 1) / tiles;
    // (TEST HOOK SOM_EXACT_PLAN_PARTS=n: at most n workgroups per tile -- 1 brings a small pass to the one-workgroup-per-tile grid of a large one)
    const long parts_cap = ex.hook.plan_parts > 0 ? ex.hook.plan_parts : 4L;
    const dim3 pgrid((unsigned)tiles, (unsigned)std::max<long>(1, std::min<long>({want, parts_cap, (long)c0.n_cstages})));
    // (two stage slots + the words the workgroup produces; level 2: + its list of active stages)
    const size_t lds1 = 2 * (size_t)h->stage_bytes + (size_t)c0.n_cstages * 8;
    const size_t lds2 = 2 * (size_t)h->stage_bytes + (size_t)c0.n_cstages * 64 * sizeof(int) + (size_t)c1.n_cstages * 8;   // (+ its list of kept groups, its words)
    const bool l2 = ex.lp.level2;
    const int force = ex.sw.skip_mode == 3 ? 1 : 0;
    const __bf16* Xs = sr.Xb_s + s0 * h->dp;
    // (the stage slots, the list of kept groups, level 2's and level 1's words, level 2's thresholds of the tile's rows: within the
    //  CU's 160 KB wherever level 2's own list fits -- policy::LaunchFacts::l2_fits_lds leaves 10 KB --, checked all the same)
    const size_t lds = lds2 + (size_t)c0.n_cstages * 8 + (size_t)SK_TILE * 8;   // (8 bytes a row: level 2's threshold as MFMA operands, exact_plan_fused_kernel)
    if (ex.sw.fuse_plan && ex.sw.chain && l2 && lastpos2 == nullptr && pgrid.y == 1 && !time_l2 && lds <= 160 * 1024) {
        PlanListsOut lo;
        lo.n_groups = (int)cdiv(h->K, EX_GROUP);
        lo.glist = ex.pbuf.glist; lo.gcnt = ex.pbuf.gcnt; lo.tile_counts = ex.pbuf.tile_counts; lo.tlist = ex.pbuf.tlist; lo.tcnt = ex.pbuf.tcnt;
        lo.tile_ticket = ex.pbuf.tile_ticket;
        lo.done = &ctr->lists_done; lo.blocks_run = &ctr->blocks_run; lo.groups_run = &ctr->groups_run;
        lo.slots = ex.sw.item_queue ? (ex.screen_slots > 0 ? ex.screen_slots : ex.pbuf.item_slots) : 0;
        lo.items = ex.sw.item_queue ? ex.pbuf.items + 8 : nullptr;        // (as exact_plan_lists hands them to exact_lists_totals_kernel)
        lo.n_items = (int*)ex.pbuf.items.p; lo.item_ctr = lo.n_items + 1; lo.len_pct = ex.sw.item_len_pct;
#define SOM_PLAN_FUSED_RUN(k, F) { \
        { int pc; if (int rc = kernel_per_cu(h, (const void*)exact_plan_fused_kernel<k, ExactEl, F>, 64 * K16_NW, lds, &pc)) return rc; } \
        exact_plan_fused_kernel<k, ExactEl, F><<<dim3((unsigned)tiles), block, lds, h->stream>>>(Xs, n, c0.Cst, c0.n_cstages, c0.cmax2, c1.Cst, c1.n_slots, \
            c1.cmax2, sr.xsq_s + s0, sr.xerr_s + s0, xmax2, h->wmax2, h->wmax2 + 1, eb, sr.lastpos_s + s0, h->Wst, sr.seed_s + s0, force, lo); }
#define SOM_PLAN_FUSED_CASE(k) case k: if (ex.sw.plan_fold) SOM_PLAN_FUSED_RUN(k, true) else SOM_PLAN_FUSED_RUN(k, false) break;
        switch (h->ks32) {
        SOM_PLAN_FUSED_CASE(1) SOM_PLAN_FUSED_CASE(2) SOM_PLAN_FUSED_CASE(3) SOM_PLAN_FUSED_CASE(4)
        default: return fail(h, "exact: block skipping supports input_len <= 128");
        }
#undef SOM_PLAN_FUSED_CASE
#undef SOM_PLAN_FUSED_RUN
        ++ex.stats.plan_fused_launches;
        ++(ex.sw.plan_fold ? ex.stats.plan_folded : ex.stats.plan_compared);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    ++ex.stats.plan_split_launches;
    ++(ex.sw.plan_fold ? ex.stats.plan_folded : ex.stats.plan_compared);
    // (level 1 stores every word; level 2 only those of the stages it walks: its words start from zero -- cleared by the level-1
    //  workgroups, each the words of its own stages; SOM_EXACT_CHAIN=0: by a fill)
    unsigned long long* const need2_clear = l2 && ex.sw.chain ? ex.pbuf.need2.p : nullptr;
    if (l2 && !ex.sw.chain) HIPCHK(h, hipMemsetAsync(ex.pbuf.need2, 0, (size_t)tiles * c1.n_cstages * sizeof(unsigned long long), h->stream));
#define SOM_PLAN_RUN(k, F) { \
        { int pc; if (int rc = kernel_per_cu(h, (const void*)exact_plan_kernel<k, ExactEl, false, F>, 64 * K16_NW, lds1, &pc)) return rc; } \
        exact_plan_kernel<k, ExactEl, false, F><<<pgrid, block, lds1, h->stream>>>(Xs, n, c0.Cst, c0.n_cstages, c0.rg, c0.n_slots, \
            sr.xsq_s + s0, sr.xerr_s + s0, sr.sU_s + s0, xmax2, c0.cmax2, h->wmax2, h->wmax2 + 1, eb, ex.pbuf.need, sr.lastpos_s + s0, \
            h->Wst, sr.seed_s + s0, nullptr, 0, force, lastpos2, lastpos2 != nullptr ? &ctr->scout_wins : nullptr, need2_clear); \
        if (l2) { \
            if (time_l2) (void)hipEventRecord(ex.cost.ev[3], h->stream); \
            { int pc; if (int rc = kernel_per_cu(h, (const void*)exact_plan_kernel<k, ExactEl, true, F>, 64 * K16_NW, lds2, &pc)) return rc; } \
            exact_plan_kernel<k, ExactEl, true, F><<<dim3((unsigned)tiles, pgrid.y), block, lds2, h->stream>>>(Xs, n, c1.Cst, c1.n_cstages, c1.rg, c1.n_slots, \
                sr.xsq_s + s0, sr.xerr_s + s0, sr.sU_s + s0, xmax2, c1.cmax2, h->wmax2, h->wmax2 + 1, eb, ex.pbuf.need2, nullptr, \
                nullptr, nullptr, ex.pbuf.need, c0.n_cstages, force); \
            if (time_l2) (void)hipEventRecord(ex.cost.ev[4], h->stream); \
        } }
#define SOM_PLAN_CASE(k) case k: if (ex.sw.plan_fold) SOM_PLAN_RUN(k, true) else SOM_PLAN_RUN(k, false) break;
    switch (h->ks32) {
    SOM_PLAN_CASE(1) SOM_PLAN_CASE(2) SOM_PLAN_CASE(3) SOM_PLAN_CASE(4)
    default: return fail(h, "exact: block skipping supports input_len <= 128");
    }
#undef SOM_PLAN_CASE
#undef SOM_PLAN_RUN
    exact_plan_lists(h, tiles, c0.n_cstages, l2 ? ex.pbuf.need2.p : nullptr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- block skipping beyond 128 features (exact_skip_wide.hpp) ---------------------------------------------------------------
// centroids, radii, |c|^2 of the groups under the current codebook; their 32-to-a-stage image with its tails and its measured
// rounding error
int exact_wide_centroids(som_handle* h, const float* xmax2) {
    auto& ex = h->ex;
    auto& c0 = ex.cen.lv[0];
    const float* Wsrc = h->ex_patch ? h->Wp : h->W;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    wide_centroids_kernel<<<dim3((unsigned)n_groups), dim3(256), 0, h->stream>>>(Wsrc, h->K, h->D, n_groups, c0.Cc, c0.rg, c0.csq, c0.cmax2, h->wmax2);
    const long total = (long)c0.n_img_stages * WD_T * h->n_kchunks * 64;
    prep_w_bf16_wide_kernel<ExactEl><<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(c0.Cc, n_groups, h->D, h->n_kchunks, c0.Cst, c0.n_img_stages,
                                                                                             nullptr, h->wmax2);
    exact_werr_kernel<ExactEl><<<dim3((unsigned)cdiv(n_groups, 4 * EX_WERR_UNITS)), dim3(256), 0, h->stream>>>(c0.Cc, n_groups, h->D, h->wmax2, c0.cmax2 + 1, nullptr);
    char* plain = ex.lp.scout ? c0.Cst_plain : nullptr;
    if (plain) HIPCHK(h, hipMemcpyAsync(plain, c0.Cst, (size_t)c0.n_img_stages * h->stage_bytes, hipMemcpyDeviceToDevice, h->stream));
    wide_centroid_tail_kernel<<<dim3((unsigned)cdiv((long)c0.n_img_stages * WD_STAGE_UNITS, 256)), dim3(256), 0, h->stream>>>(
        c0.rg, c0.csq, n_groups, c0.Cst, c0.n_img_stages, h->stage_bytes, xmax2, h->wmax2, plain);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the sorted pass: float32 rows, norms, last BMUs gathered in the order, the tile image built from the sorted rows
int exact_wide_gather(som_handle* h, SortedRows& sr, long s0, const float* X, long n, const float* xsq, const float* xerr,
                      const int* prev, const float* xmax2) {
    const long np = round_up(n, SK_TILE);
    wide_gather_sorted_kernel<<<dim3((unsigned)cdiv(np, 4)), dim3(256), 0, h->stream>>>(sr.order + s0, n, np, h->D, X, xsq, xerr, prev,
                                                                                      sr.Xf_s + s0 * h->D, sr.xsq_s + s0, sr.xerr_s + s0, sr.lastpos_s + s0);
    const long n_blocks = np / h->tl_bm;
    const long total = n_blocks * h->n_kchunks * (h->tl_bm / 16) * TL_KS * 64;
    prep_tiles_bf16_kernel<ExactEl><<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
        sr.Xf_s + s0 * h->D, n, h->D, h->n_kchunks, n_blocks, h->tl_bm, h->tl_xtile, 1.0f, nullptr, (char*)(sr.Xb_s + s0 * h->dp), xmax2);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the scout beyond 128 features, step 1: every row's nearest group centroid (the plain wide kernel on the plain centroid image)
template <int KS32>
int exact_wide_scout_nearest_ks(som_handle* h, const __bf16* Ximg, long n, unsigned long long* best64, int* g_out) {
    auto& ex = h->ex;
    const auto& c0 = ex.cen.lv[0];
    const size_t lds = (size_t)WD_SLOTS * wd_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)bmu_bf16_wide_kernel<KS32, ExactEl>, 64 * WD_NW, lds, &per_cu)) return rc;
    const long blocks = cdiv(n, WD_WG_SAMPLES);
    const long slots = resident_slots(h, per_cu);
    const int parts = (int)std::max<long>(1, std::min<long>({cdiv(2 * slots, blocks), 8L, (long)c0.n_img_stages}));
    bmu_bf16_wide_kernel<KS32, ExactEl><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * WD_NW), lds, h->stream>>>(
        (const char*)Ximg, n, c0.Cst_plain, c0.n_img_stages, best64);
    bmu_finalize_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(best64, n, c0.n_slots, g_out);
    HIPCHK(h, hipMemsetAsync(best64, 0xFF, (size_t)n * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipGetLastError());
    return 0;
}
// ... step 3: per tile of the sorted pass the groups of its rows' keys, the plain wide kernel over those groups' units with
// indices kept: the best of them, as a UNIT id, -> lastpos_s (what the wide plan's float32 seed evaluates)
template <int KS32>
int exact_wide_scout_pick_ks(som_handle* h, SortedRows& sr, long s0, long n, const int* keys, unsigned long long* best64) {
    auto& ex = h->ex;
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    const long tiles = round_up(n, SK_TILE) / SK_TILE;
    const size_t lds_l = (size_t)cdiv(n_groups, 64) * sizeof(unsigned long long);
    exact_scout_lists_kernel<<<dim3((unsigned)tiles), dim3(64), lds_l, h->stream>>>(keys, nullptr, n, n_groups, ex.pbuf.glist, ex.pbuf.gcnt, 1);
    const size_t lds = (size_t)WD_SLOTS * wd_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)bmu_bf16_wide_kernel<KS32, ExactEl, false, true>, 64 * WD_NW, lds, &per_cu)) return rc;
    bmu_bf16_wide_kernel<KS32, ExactEl, false, true><<<dim3((unsigned)tiles, 1), dim3(64 * WD_NW), lds, h->stream>>>(
        (const char*)(sr.Xb_s + s0 * h->dp), n, h->Wst, h->n_stages, best64, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ExactBound(),
        ex.pbuf.glist, ex.pbuf.gcnt, n_groups);
    exact_scout_pos_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(best64, n, h->K, sr.lastpos_s + s0, h->ex_perm);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int exact_wide_scout_nearest(som_handle* h, const __bf16* Ximg, long n, unsigned long long* best64, int* g_out) {
    return for_kchunks(h, "exact: no wide scout instance for this input_len",
                       [&](auto k) { return exact_wide_scout_nearest_ks<decltype(k)::value>(h, Ximg, n, best64, g_out); });
}
int exact_wide_scout_pick(som_handle* h, SortedRows& sr, long s0, long n, const int* keys, unsigned long long* best64) {
    return for_kchunks(h, "exact: no wide scout instance for this input_len",
                       [&](auto k) { return exact_wide_scout_pick_ks<decltype(k)::value>(h, sr, s0, n, keys, best64); });
}

// one pass's plan on the sorted rows: the float32 score of every row's last BMU, the rows' thresholds, the wide kernel in its
// PLAN mode over the centroid image, the tiles' lists
template <int KS32>
int exact_wide_plan_ks(som_handle* h, SortedRows& sr, long s0, long n, const float* xmax2, const ExactBound& eb) {
    auto& ex = h->ex;
    const auto& c0 = ex.cen.lv[0];
    const long np = round_up(n, SK_TILE);
    const long tiles = np / SK_TILE;
    // (sr.lastpos_s holds the sorted rows' last BMUs as UNIT ids here; the seed itself is not used beyond 128 features)
    exact_seed_kernel<<<dim3((unsigned)cdiv(n * 16, 256)), dim3(256), 0, h->stream>>>(
        sr.Xf_s + s0 * h->D, n, h->D, h->W, h->wsq, h->K, sr.lastpos_s + s0, sr.xsq_s + s0, sr.xerr_s + s0, h->wmax2, xmax2, h->wmax2 + 1, eb, ex.pass.seed, ex.pbuf.tq);
    wide_plan_rows_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(n, sr.xsq_s + s0, sr.xerr_s + s0, ex.pbuf.tq, xmax2, c0.cmax2, h->wmax2,
                                                                                  h->wmax2 + 1, eb, ex.sw.skip_mode == 3 ? 1 : 0, sr.seed_s + s0, sr.sU_s + s0);
    HIPCHK(h, hipMemsetAsync(ex.pbuf.need, 0, (size_t)tiles * c0.n_cstages * sizeof(unsigned long long), h->stream));
    auto kern = bmu_bf16_wide_kernel<KS32, ExactEl, false, false, true>;
    const size_t lds = (size_t)WD_SLOTS * wd_stage_bytes(KS32) + (size_t)c0.n_cstages * sizeof(unsigned long long);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 64 * WD_NW, lds, &per_cu)) return rc;
    const long slots = resident_slots(h, per_cu);
    int parts = (int)std::max<long>(1, std::min<long>({cdiv(2 * slots, tiles), 8L, (long)c0.n_img_stages}));
    bmu_bf16_wide_kernel<KS32, ExactEl, false, false, true><<<dim3((unsigned)tiles, (unsigned)parts), dim3(64 * WD_NW), lds, h->stream>>>(
        (const char*)(sr.Xb_s + s0 * h->dp), n, c0.Cst, c0.n_img_stages, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ExactBound(),
        nullptr, nullptr, 0, sr.seed_s + s0, sr.sU_s + s0, ex.pbuf.need, c0.n_cstages);
    // (the tiles' lists and the listed screen's work queue: the lists -- counted in 16-unit blocks, four to a group -- cut into items)
    exact_plan_lists(h, tiles, c0.n_cstages, nullptr);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int exact_wide_plan(som_handle* h, SortedRows& sr, long s0, long n, const float* xmax2, const ExactBound& eb) {
    return for_kchunks(h, "exact: no wide plan instance for this input_len",
                       [&](auto k) { return exact_wide_plan_ks<decltype(k)::value>(h, sr, s0, n, xmax2, eb); });
}

template <int KG>
int exact_rescore_kg(som_handle* h, const float* X, unsigned long long* best64, int deint) {
    auto& ex = h->ex;
    auto kern = exact_rescore_mfma_kernel<KG>;
    const size_t lds = (size_t)fr_stage_bytes(KG);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 256, lds, &per_cu)) return rc;
    // (twice the resident slots: the runs of tiles are uneven -- partial tiles, idle waves -- and finer runs balance them)
    const long grid = std::min<long>(ex.pass.max_tiles, h->ex.sw.grid_mult * resident_slots(h, per_cu));
    kern<<<dim3((unsigned)grid), dim3(256), lds, h->stream>>>(X, h->D, h->Wfst, h->K, ex.pass.tile_tab, &pass_ctr(h).tail()->n_tiles, ex.pass.plist,
                                                             best64, h->ex_perm, nullptr, h->ex_sub44 ? 1 : 0, deint, nullptr);
    return 0;
}

// workgroups of exact_tiles_kernel: each repeats the scan of the groups' counts and writes its share of the tile table (one
// workgroup writing some tens of thousands of entries set that launch's time; SOM_EXACT_CHAIN=0: one)
inline unsigned exact_tiles_blocks(const som_handle* h) { return h->ex.sw.chain ? 16u : 1u; }

// the refinement pass over a sorted pass's candidate pairs (bmu_exact.hpp): tiles -> refined minima -> lists compacted in place
template <int KS32>
int exact_refine_ks(som_handle* h, SortedRows& sr, long r0, long n, const float* xmax2, const ExactBound& eb) {
    auto& ex = h->ex;
    const PassCtr pc = pass_ctr(h);
    const int n_groups = pc.n_groups;
    int* gcount = pc.gcount(); PassCounters* const ctr = pc.tail();
    int* n_tiles = &ctr->n_tiles;
    exact_tiles_kernel<<<dim3(exact_tiles_blocks(h)), dim3(1024), 0, h->stream>>>(gcount, n_groups, ex.pass.stride, ex.pass.stride * ex.pass.pairs, ex.pass.tile_tab, n_tiles,
                                                                                 &ctr->overflow, nullptr, nullptr, &ctr->pairs_in);
    uint32_t* rowmin2 = (uint32_t*)ex.pass.rowarg.p;            // (round 1's scratch: unused in the one-round scheme)
    // (all ones to start from: written by the select kernel, which has visited every row; SOM_EXACT_CHAIN=0: by a fill)
    if (!ex.sw.chain) HIPCHK(h, hipMemsetAsync(rowmin2, 0xFF, (size_t)n * sizeof(uint32_t), h->stream));
    const size_t lds = (size_t)k16_stage_bytes(KS32) + (size_t)K16_T * KS32 * 1024;
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)exact_refine_kernel<KS32, ExactEl>, 256, lds, &per_cu)) return rc;
    const long grid = std::min<long>(ex.pass.max_tiles, h->ex.sw.grid_mult * resident_slots(h, per_cu));
    exact_refine_kernel<KS32, ExactEl><<<dim3((unsigned)grid), dim3(256), lds, h->stream>>>(
        sr.Xb_s + r0 * h->dp, sr.Xl_s + r0 * h->dp, h->Wst, h->Wst_lo, ex.pass.tile_tab, n_tiles, ex.pass.plist, ex.pass.gmin, rowmin2);
    exact_thr2_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(rowmin2, n, sr.xsq_s + r0, sr.xerr_s + r0, h->wmax2, xmax2,
                                                                               h->wmax2 + 1, eb);
    exact_select2_kernel<<<dim3((unsigned)n_groups), dim3(256), 0, h->stream>>>(ex.pass.plist, ex.pass.gmin, ex.pass.stride, gcount, rowmin2, &ctr->pairs_out);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int exact_refine(som_handle* h, SortedRows& sr, long r0, long n, const float* xmax2, const ExactBound& eb) {
    return for_ks32(h, "exact: the refinement pass supports input_len <= 128",
                    [&](auto k) { return exact_refine_ks<decltype(k)::value>(h, sr, r0, n, xmax2, eb); });
}

// the lists' entries from gstart on -> tiles -> float32 scores merged into best64 (the pass's slice of the merge keys)
// (sorted_copy: X is a sorted pass's float32 copy -- up to 128 features and a multiple of 8 of them: de-interleaved rows,
//  exact_gather_sorted_kernel)
// (count_pairs: the tiles kernel leaves the pass's pair count in the counters; the planned launch's refinement pass has counted already)
int exact_rescore_round(som_handle* h, const float* X, const float* xsq, unsigned long long* best64, const int* gstart,
                        int* gstart_out, bool sorted_copy, bool count_pairs) {
    auto& ex = h->ex;
    const int deint = (sorted_copy && !h->wide && (h->D & 7) == 0) ? 1 : 0;
    const PassCtr pc = pass_ctr(h);
    const int n_groups = pc.n_groups;
    int* gcount = pc.gcount(); PassCounters* const ctr = pc.tail();
    int* n_tiles = &ctr->n_tiles;
    // (the pairs the select kernel found go back with the pass's counters -- unless the refinement pass has counted them already)
    exact_tiles_kernel<<<dim3(exact_tiles_blocks(h)), dim3(1024), 0, h->stream>>>(gcount, n_groups, ex.pass.stride, ex.pass.stride * ex.pass.pairs, ex.pass.tile_tab, n_tiles,
                                                                                 &ctr->overflow, gstart, gstart_out,
                                                                                 (gstart == nullptr && gstart_out == nullptr && count_pairs) ? &ctr->pairs_in : nullptr);
    if (h->wide) {
        // beyond 128 features: the float32 tile image, chunk by chunk
        if (!h->Wfimg) return fail(h, "exact: no float32 tile image");
        const bool cosine = h->cfg.distance == SOM_DIST_COSINE;
        const void* kern = cosine ? (const void*)exact_rescore_tiled_kernel<SCORE_COSINE>
                                  : (const void*)exact_rescore_tiled_kernel<SCORE_EUCLID_PART>;
        int per_cu = 1;
        if (int rc = kernel_per_cu(h, kern, 256, 0, &per_cu)) return rc;
        const long grid = std::min<long>(ex.pass.max_tiles, h->ex.sw.grid_mult * resident_slots(h, per_cu));
        if (cosine)
            exact_rescore_tiled_kernel<SCORE_COSINE><<<dim3((unsigned)grid), dim3(256), 0, h->stream>>>(
                X, h->D, xsq, h->Wfimg, h->ft_kchunks, h->K, ex.pass.tile_tab, n_tiles, ex.pass.plist, best64, h->ex_perm, nullptr, h->ex_sub44 ? 1 : 0);
        else
            exact_rescore_tiled_kernel<SCORE_EUCLID_PART><<<dim3((unsigned)grid), dim3(256), 0, h->stream>>>(
                X, h->D, xsq, h->Wfimg, h->ft_kchunks, h->K, ex.pass.tile_tab, n_tiles, ex.pass.plist, best64, h->ex_perm, nullptr, h->ex_sub44 ? 1 : 0);
        return 0;
    }
    switch (h->fr_kg) {
    case 1: return exact_rescore_kg<1>(h, X, best64, deint);
    case 2: return exact_rescore_kg<2>(h, X, best64, deint);
    case 4: return exact_rescore_kg<4>(h, X, best64, deint);
    case 8: return exact_rescore_kg<8>(h, X, best64, deint);
    case 16: return exact_rescore_kg<16>(h, X, best64, deint);
    }
    return fail(h, "exact: bad k-group count");
}

int build_tables(som_handle* h, double sigma, double eta, int neigh_f64, hipStream_t st);

// ---- one BMU launch: facts -> plan (policy::PlanState, exact_policy.hpp) -> passes -> outcome -------------------------------------

// can block skipping engage on this handle at all (whatever the feature count)?  By default on maps of >= 4096 units.
bool exact_skip_wanted(const som_handle* h) {
    const auto& ex = h->ex;
    return ex.sw.skip_mode > 0 && ex.sw.seed_on && (ex.sw.skip_mode > 1 ? cdiv(h->K, EX_GROUP) >= 2 : h->K >= 4096);
}

// a launch: the row set (float32 rows, |x|^2 and measured operand errors, operand image, the ids to write), the facts the
// policy decided on, and what the passes have measured and counted so far
struct ExactLaunch {
    const Rows rows;
    ExactBound eb;
    int n_groups;
    bool two_round;
    policy::LaunchFacts f;
    policy::LaunchOutcome o;
    bool lastpos_carried = false;    // sr.lastpos_s holds the rows' last BMUs' positions already (the last epoch's finalize): no exact_lastpos_kernel
    long pos_kept_rows = 0;          // rows whose positions this launch's finalize has stored
    long fallback_rows = 0;          // rows this launch handed to the float32 kernel
};

// Is there anything for the plan to skip?  The scout, the gather and the plan cost a fifth of a full scan: before the
// pass is committed to them, every stride-th TILE of its sorted order -- up to 128 of the very tiles the plan would see
// -- goes through gather, pick and plan as a small pass of its own and the executed share comes back (one host wait).
// The launch runs every block, unsorted, without a plan where the forecast says that is cheaper -- share x (screen
// time per block under a plan) + (what a scouted launch spends outside its screen) against the last launch without
// a plan, all MEASURED (before the first measurements: a scouted plan's overhead taken as a fifth of a full screen;
// with no full scan on record either: declined above 0.8 of the blocks) -- a random codebook, the smooth map of a
// schedule's second epoch, rows without structure.  The sample also says what level 2 is worth before it runs on
// the whole pass: it removes (1 - ratio) of a kept group's four blocks at its measured (else: a sixth of the
// group's screen) cost per kept group.  (policy::PlanState::tiles_sampled decides; it cancels the launch's plan where it declines.)
int exact_sample_tiles(som_handle* h, const ExactLaunch& L, SortedRows& sr, long r0, long s0, long tiles_all) {
    auto& ex = h->ex;
    auto& lp = ex.lp;
    const PassCtr pc = pass_ctr(h);
    unsigned long long* best = h->best64 + r0;
    auto& ss = ex.srt[1];
    const long st = tiles_all / 128, n_st = std::min<long>(128, tiles_all / st), ns = n_st * SK_TILE;
    int* s_order = ex.pbuf.sk_keys;                    // (the sort's input keys and row ids: free since the sort)
    int* s_keys = ex.pbuf.sk_vals;
    exact_sample_tiles_kernel<<<dim3((unsigned)n_st), dim3(SK_TILE), 0, h->stream>>>(sr.order + s0, ex.pbuf.sk_keys2, st, s_order, s_keys);
    const Rows& R = L.rows;
    if (int rc = exact_skip_gather(h, ss, 0L, s_order, R.X + r0 * h->D, R.Xb + r0 * h->dp, ns, R.xsq + r0, R.xerr + r0, R.xmax2)) return rc;
    if (int rc = exact_scout_pick(h, ss, 0L, ns, s_keys, best)) return rc;
    const int* lp2 = nullptr;
    if (L.f.have_last) {
        exact_lastpos_kernel<<<dim3((unsigned)cdiv(ns, 256)), dim3(256), 0, h->stream>>>(R.out + r0, s_order, h->ex_inv, ns, h->K, ex.pbuf.scout_g);
        lp2 = ex.pbuf.scout_g;                         // (the nearest groups have gone into the sort keys: free)
    }
    if (int rc = exact_skip_plan(h, ss, 0L, ns, R.xmax2, L.eb, lp2)) return rc;
    HIPCHK(h, hipMemcpyAsync(ex.pass_host, pc.tail(), sizeof(PassCounters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // (the sample's count of the scout's wins is not the pass's: cleared again)
    HIPCHK(h, hipMemsetAsync(&pc.tail()->scout_wins, 0, sizeof(int), h->stream));
    const double est = (double)ex.pass_host->blocks_run / (double)(n_st * L.n_groups * K16_T);
    const double est1 = (double)ex.pass_host->groups_run / (double)(n_st * L.n_groups);
    ex.fc.est = est; ex.fc.est1 = est1; ex.fc.n_st = (double)n_st; ex.fc.st = (double)st;
    ex.fc.blocks_run = (double)ex.pass_host->blocks_run; ex.fc.groups_run = (double)ex.pass_host->groups_run;
    ex.fc.level2 = lp.level2 ? 1.0 : 0.0;
    const bool decline = ex.plan.tiles_sampled(est, est1, L.f, lp);
    if (h->debug) {
        const policy::Costs& c = ex.plan.costs();
        std::fprintf(stderr, "[somhip] exact scout: %ld sample tiles of %ld would run %.4f of their blocks (level 1: %.4f) -> %s, level 2 %d "
                     "[per row: full %.3g us, block %.3g us, overhead %.3g us]\n", n_st, tiles_all, est, est1,
                     decline ? "no plan" : "plan", lp.level2 ? 1 : 0, 1e3 * c.full_total, 1e3 * policy::block_ms(c, L.f.blocks_per_row),
                     1e3 * policy::scouted_overhead(c));
    }
    return 0;
}

// rows the scheme could not settle (normally none): the float32 kernel itself
int exact_fallback_rows(som_handle* h, const ExactLaunch& L, long r0, int n_fb) {
    auto& ex = h->ex;
    int* out = L.rows.out;
    if (int rc = ex.pass.fbX.reserve(h, (size_t)n_fb * h->D, (size_t)1024 * h->D)) return rc;
    if (int rc = ex.pass.fb_ids.reserve(h, (size_t)n_fb, 1024)) return rc;
    // the float32 kernel names units by their place in its image: the units' own order for it
    if (h->ops.f32_in_patch_order()) if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    exact_gather_rows_kernel<<<dim3((unsigned)cdiv((long)n_fb * h->D, 256)), dim3(256), 0, h->stream>>>(
        L.rows.X + r0 * h->D, ex.pass.fb_list, n_fb, h->D, ex.pass.fbX);
    // (its part merge may reuse best64[0 .. n_fb): rows this pass has already settled)
    if (h->cfg.distance == SOM_DIST_COSINE) {
        // (|x|^2 of the gathered rows in NumPy's order, into the head of the pass's spent minima)
        float* fsq = (float*)ex.pass.gmin.p;
        row_sq_f32_kernel<<<dim3((unsigned)cdiv(n_fb, 256)), dim3(256), 0, h->stream>>>(ex.pass.fbX, n_fb, h->D, fsq);
        if (int rc = launch_bmu_f32_any<SCORE_COSINE>(h, ex.pass.fbX, n_fb, fsq, ex.pass.fb_ids)) return rc;
    } else if (int rc = launch_bmu_f32_any<SCORE_EUCLID_PART>(h, ex.pass.fbX, n_fb, nullptr, ex.pass.fb_ids)) return rc;
    exact_scatter_ids_kernel<<<dim3((unsigned)cdiv(n_fb, 256)), dim3(256), 0, h->stream>>>(ex.pass.fb_ids, ex.pass.fb_list, n_fb,
                                                                                        out + r0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ONE PASS over the rows [r0, r0 + n) under the launch's plan (h->ex.lp): scout, sort, gather, plan; screen; select, refine,
// re-score, finalize; the counters read back and added to the launch's outcome; the float32 fallback.
int exact_pass(som_handle* h, ExactLaunch& L, SortedRows& sr, long r0, long n) {
    auto& ex = h->ex;
    auto& cost = ex.cost;
    auto& lp = ex.lp;
    const PassCtr pc = pass_ctr(h);
    const int n_groups = L.n_groups;
    const Rows& R = L.rows;
    const float* X = R.X; const float* xsq = R.xsq; const float* xerr = R.xerr; const __bf16* Xb = R.Xb; const float* xmax2 = R.xmax2;
    int* out = R.out; const long N = R.N;
    const ExactBound& eb = L.eb;
    const bool have_last = L.f.have_last;
    const long s0 = L.f.resident ? r0 : 0;               // where the pass sits in the sorted copies
    if (r0 > 0) HIPCHK(h, hipEventRecord(cost.ev[0], h->stream));
    // (a pass behind one whose fallback rows went through the float32 kernel: its image back in patch order)
    if (h->ops.f32_in_patch_order() != h->ex_patch) if (int rc = refresh_codebook_operands(h, operands::Request::ExactScreen)) return rc;
    HIPCHK(h, hipMemsetAsync(pc.base, 0, pc.bytes(), h->stream));
    // (sorted pass: the screen, the select kernel and the merge keys work on positions of the sorted order)
    const float* p_xsq = xsq + r0; const float* p_xerr = xerr + r0; const float* p_seed = nullptr;
    const __bf16* p_Xb = Xb + r0 * h->dp;
    const float* p_X = X + r0 * h->D;                    // the rows the re-score reads, indexed like the lists' entries
    const int* p_order = nullptr;
    if (lp.skip) {
        unsigned long long* best = h->best64 + r0;
        if (lp.scout && h->wide) { if (int rc = exact_wide_scout_nearest(h, Xb + r0 * h->dp, n, best, ex.pbuf.scout_g)) return rc; }
        else if (lp.scout)
            if (int rc = exact_scout_nearest(h, Xb + r0 * h->dp, n, best, ex.pbuf.scout_g)) return rc;
        if (lp.resort) {
            if (lp.time_phases) { HIPCHK(h, hipEventRecord(cost.ev[5], h->stream)); }
            if (int rc = exact_skip_sortkeys(h, sr, s0, n, out + r0, lp.scout ? ex.pbuf.scout_g : nullptr)) return rc;
        }
        const long tiles_all = n / SK_TILE;
        if (lp.sample_tiles && r0 == 0 && tiles_all > 256)
            if (int rc = exact_sample_tiles(h, L, sr, r0, s0, tiles_all)) return rc;
    }
    // resident rows from their second epoch on: last epoch's BMU of every row caps the screen's keep threshold -- under a
    // plan the plan's prologue forms that seed from the operands it holds (exact_skip.hpp), else exact_seed_kernel
    ex.seed_live = ex.sw.seed_on && !h->wide && have_last;
    if (ex.seed_live && !lp.skip) {
        exact_seed_kernel<<<dim3((unsigned)cdiv(n * 16, 256)), dim3(256), 0, h->stream>>>(
            X + r0 * h->D, n, h->D, h->W, h->wsq, h->K, out + r0, xsq + r0, xerr + r0, h->wmax2, xmax2, h->wmax2 + 1, eb, ex.pass.seed);
        p_seed = ex.pass.seed;
    }
    if (lp.skip && h->wide) {
        // beyond 128 features: the sorted float32 rows + the tile image built from them, the plan as a mode of the wide kernel
        if (lp.resort) {
            // (no last BMUs: `out` holds nothing yet -- the gather's copy of it is overwritten by the scout's picks below)
            if (int rc = exact_wide_gather(h, sr, s0, X + r0 * h->D, n, xsq + r0, xerr + r0, have_last ? out + r0 : ex.pbuf.scout_g, xmax2)) return rc;
            if (lp.time_phases) { HIPCHK(h, hipEventRecord(cost.ev[6], h->stream)); L.o.sort_timed = true; }
            if (lp.scout)
                if (int rc = exact_wide_scout_pick(h, sr, s0, n, ex.pbuf.sk_keys2, h->best64 + r0)) return rc;
        } else {
            wide_prev_sorted_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(sr.order + s0, n, out + r0, sr.lastpos_s + s0);
        }
        if (int rc = exact_wide_plan(h, sr, s0, n, xmax2, eb)) return rc;
        p_xsq = sr.xsq_s + s0; p_xerr = sr.xerr_s + s0; p_seed = nullptr; p_Xb = sr.Xb_s + s0 * h->dp; p_order = sr.order + s0;
        p_X = sr.Xf_s + s0 * h->D;
    } else if (lp.skip) {
        unsigned long long* best = h->best64 + r0;
        if (lp.resort) {
            if (int rc = exact_skip_gather(h, sr, s0, sr.order + s0, X + r0 * h->D, Xb + r0 * h->dp, n, xsq + r0, xerr + r0, xmax2)) return rc;
            if (lp.time_phases) { HIPCHK(h, hipEventRecord(cost.ev[6], h->stream)); L.o.sort_timed = true; }
            if (sr.Xl_s != nullptr && r0 + n >= N) sr.xl_filled = true;
        }
        const int* lastpos2 = nullptr;
        if (lp.scout) {
            if (int rc = exact_scout_pick(h, sr, s0, n, ex.pbuf.sk_keys2, best)) return rc;
            if (have_last) {
                // (the rows' real last BMUs beside the scout's picks: the plan's prologue keeps the better unit; sk_vals: free since the sort)
                exact_lastpos_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(out + r0, sr.order + s0, h->ex_inv, n, h->K, ex.pbuf.sk_vals);
                lastpos2 = ex.pbuf.sk_vals;
            }
        } else if (!L.lastpos_carried) {
            // (carried: the last epoch's finalize has left exactly these positions in lastpos_s -- launch_bmu_exact)
            exact_lastpos_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(out + r0, sr.order + s0, h->ex_inv, n, h->K, sr.lastpos_s + s0);
        }
        if (int rc = exact_skip_plan(h, sr, s0, n, xmax2, eb, lastpos2, lp.time_phases && lp.level2)) return rc;
        if (lp.time_phases && lp.level2) L.o.l2_timed = true;
        p_xsq = sr.xsq_s + s0; p_xerr = sr.xerr_s + s0; p_seed = sr.seed_s + s0; p_Xb = sr.Xb_s + s0 * h->dp; p_order = sr.order + s0;
        p_X = sr.Xf_s + s0 * h->D;
    }
    // the listed screen on its work queue selects the candidates in its own launch (SOM_EXACT_FUSE_SELECT=0: exact_select_kernel
    // behind it, as on every other path): what the select kernel would get, handed to exact_screen
    bool sel_fused = false;
    ScreenSelect screen_sel{};
    if (ex.sw.fuse_select && lp.skip && !h->wide && !L.two_round && ex.sw.item_queue)
        screen_sel = ScreenSelect{ex.pbuf.glist, ex.pbuf.gcnt, ex.pass.plist, pc.gcount(), ex.pass.rowcnt, lp.refine && ex.sw.chain ? (uint32_t*)ex.pass.rowarg.p : nullptr,
                                     ex.pbuf.tile_ticket, &pc.tail()->ticket_tiles};
    {
        // (under a plan with the select tail the bracket -- and cost.ev[1] .. ev[2], the policy's screen time -- holds the selection too)
        Timed ts(h, SOM_K_SCREEN);
        if (lp.time_phases) { HIPCHK(h, hipEventRecord(cost.ev[1], h->stream)); }
        // (the lists the screen walks: dense 16-unit tiles up to 128 features, whole groups beyond)
        if (int rc = exact_screen_ks(h, p_Xb, n, h->best64 + r0, p_xsq, p_xerr, xmax2, eb, p_seed,
                              lp.skip ? (h->wide ? ex.pbuf.glist : ex.pbuf.tlist) : nullptr,
                              lp.skip ? (h->wide ? ex.pbuf.gcnt : ex.pbuf.tcnt) : nullptr, screen_sel, &sel_fused)) return rc;
        if (lp.time_phases) { HIPCHK(h, hipEventRecord(cost.ev[2], h->stream)); L.o.screen_timed = true; }
    }
    (sel_fused ? ex.stats.sel_fused_passes : ex.stats.sel_launched_passes) += 1;
    const dim3 sel_grid((unsigned)cdiv(n, 64)), sel_block(64 * EX_SCAN_SPLIT);
    unsigned long long* best = h->best64 + r0;
    // two rounds beyond 128 features, where a (row, group) pair costs 64 x D flop AND a gather of the row's D floats
    // (configs[4]: 92.8 -> 87.8 ms per epoch); one round up to 128 features, where the three launches more cost more than
    // the pairs they save (256 x 256 x 128, 1 Mi rows: 15.5 vs 15.8 ms; 65 536 rows: +3 % in every map state)
    if (L.two_round) {
        // round 1: every row against the group that holds its screen minimum; round 2: the groups within the ONE-unit
        // bound of that float32 score (exact_select_kernel<true>: 20-32 % fewer pairs than the one-round scheme on
        // smooth maps, up to one pair per row more on random ones)
        // (under a plan -- exact_skip_wide.hpp -- rows are sorted positions: p_X, p_xsq, p_xerr; the select kernel walks the lists)
        exact_first_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(
            best, n, n_groups, ex.pass.stride, p_xsq, h->wmax2, xmax2, eb, p_xerr, h->wmax2 + 1, ex.pass.plist, pc.gcount(), ex.pass.rowarg);
        if (int rc = exact_rescore_round(h, p_X, p_xsq, best, nullptr, pc.gstart(), lp.skip, !lp.refine)) return rc;
        exact_select_kernel<true><<<sel_grid, sel_block, 0, h->stream>>>(
            ex.pass.gmin, ex.pass.gflags, ex.pass.stride, n_groups, n, best, p_xsq, h->wmax2, xmax2, eb, p_xerr, h->wmax2 + 1, ex.pass.plist,
            pc.gcount(), ex.pass.rowcnt, ex.pass.rowarg, nullptr, lp.skip ? ex.pbuf.glist : nullptr, lp.skip ? ex.pbuf.gcnt : nullptr, SK_TILE);
        if (int rc = exact_rescore_round(h, p_X, p_xsq, best, pc.gstart(), nullptr, lp.skip, !lp.refine)) return rc;
    } else {
        if (!sel_fused)
            exact_select_kernel<false><<<sel_grid, sel_block, 0, h->stream>>>(
                ex.pass.gmin, ex.pass.gflags, ex.pass.stride, n_groups, n, best, p_xsq, h->wmax2, xmax2, eb, p_xerr, h->wmax2 + 1, ex.pass.plist,
                pc.gcount(), ex.pass.rowcnt, nullptr, p_seed, lp.skip ? ex.pbuf.glist : nullptr, lp.skip ? ex.pbuf.gcnt : nullptr, SK_TILE,
                nullptr, 0, 0, lp.refine && ex.sw.chain ? (uint32_t*)ex.pass.rowarg.p : nullptr);
        if (lp.refine)
            if (int rc = exact_refine(h, sr, s0, n, xmax2, eb)) return rc;
        if (int rc = exact_rescore_round(h, p_X, xsq + r0, best, nullptr, nullptr, lp.skip, !lp.refine)) return rc;
    }
    // (a sorted resident pass up to 128 features: the ids' positions in patch order stay behind for the next epoch's plan)
    const bool keep_pos = ex.sw.chain && lp.skip && !h->wide && L.f.resident && p_order != nullptr;
    exact_finalize_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(
        best, n, h->K, &pc.tail()->overflow, out + r0, ex.pass.fb_list, &pc.tail()->fallback, p_order,
        keep_pos ? sr.lastpos_s + s0 : nullptr, keep_pos && h->ex_patch ? h->ex_inv.p : nullptr);
    if (keep_pos) L.pos_kept_rows += n;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(ex.pass_host, pc.tail(), sizeof(PassCounters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(cost.ev[7], h->stream));
    if (h->early.armed && !h->early.done && R.resident && r0 + n >= N) {
        // the last pass of a resident epoch: the host waits for the counter only (an event behind the copy); what the
        // update needs besides the BMUs is queued behind it and runs while the host wakes up
        if (!ex.fb_ready) HIPCHK(h, hipEventCreateWithFlags(&ex.fb_ready, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(ex.fb_ready, h->stream));
        HIPCHK(h, hipMemsetAsync(h->SC, 0, (size_t)h->K * (h->D1p + 1) * sizeof(float), h->stream));
        if (int rc = build_tables(h, h->early.sigma, h->early.eta, h->early.neigh_f64, h->stream)) return rc;
        h->early.done = true;
        HIPCHK(h, hipEventSynchronize(ex.fb_ready));
    } else {
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, cost.ev[0], cost.ev[7]) == hipSuccess) L.o.t_total += ms;
        if (L.o.screen_timed && hipEventElapsedTime(&ms, cost.ev[1], cost.ev[2]) == hipSuccess) L.o.t_screen += ms;
        if (L.o.l2_timed && hipEventElapsedTime(&ms, cost.ev[3], cost.ev[4]) == hipSuccess) L.o.t_l2 += ms;
        if (L.o.sort_timed && hipEventElapsedTime(&ms, cost.ev[5], cost.ev[6]) == hipSuccess) L.o.t_sort += ms;
        (void)hipGetLastError();
    }
    const PassCounters& got = *ex.pass_host;
    const int n_fb = got.fallback;
    ex.stats.rows_total += n; ex.stats.rows_fallback += n_fb; ex.stats.chunks += 1;
    // (counted in 16-unit blocks: four per (256-row tile, group))
    ex.stats.blocks_total += cdiv(n, SK_TILE) * n_groups * K16_T;
    ex.last_plan_tiles = lp.skip && !h->wide ? cdiv(n, SK_TILE) : 0;   // (som_debug_exact_tile_blocks: the lists as this pass's screen walked them)
    ex.last_plan_l2 = lp.skip && lp.level2;
    ex.stats.blocks_run += lp.skip ? got.blocks_run : cdiv(n, SK_TILE) * n_groups * K16_T;
    L.o.groups_run += lp.skip ? got.groups_run : cdiv(n, SK_TILE) * n_groups;
    L.o.pairs_in += got.pairs_in;
    if (lp.refine) L.o.pairs_out += got.pairs_out;
    if (lp.skip && lp.scout && have_last) L.o.scout_wins += got.scout_wins;
    if (sel_fused) ex.stats.sel_ticket_tiles += got.ticket_tiles;
    L.fallback_rows += n_fb;
    if (n_fb < 0 || n_fb > n) return fail(h, "exact: fallback counter out of range");
    if (n_fb > 0) return exact_fallback_rows(h, L, r0, n_fb);
    return 0;
}

// R: the row set's float32 rows, their |x|^2 and measured errors, their operand image, the ids to write.
int launch_bmu_exact(som_handle* h, const Rows& R) {
    if (h->capturing) return fail(h, "precision 'exact' reads a counter back per pass: not capturable");
    if (!R.xsq || !R.xerr) return fail(h, "exact: no row norms");
    const float* X = R.X; const long N = R.N; const float* xmax2 = R.xmax2;
    auto& ex = h->ex;
    auto& cost = ex.cost;
    auto& lp = ex.lp;
    if (int rc = exact_reserve(h, N)) return rc;
    if (int rc = h->best64.reserve(h, (size_t)N, 1024)) return rc;
    if (!cost.have) {
        for (auto& e : cost.ev) HIPCHK(h, hipEventCreate(&e));
        cost.have = true;
    }
    HIPCHK(h, hipEventRecord(cost.ev[0], h->stream));
    // the stages' initial accumulators and the launch's merge keys: at once -- or, where the codebook's 16-bit image is still due
    // (flush_prep_w), behind the plan's decision: a planned launch up to 128 features sends them out in one grid with the images
    const long units = (long)h->n_stages * h->stage_units;
    const unsigned wsqh_blocks = (unsigned)cdiv(std::max(units, N), 256);
    auto launch_wsqh = [&]() {
        prep_wsqh_kernel<<<dim3(wsqh_blocks), dim3(256), 0, h->stream>>>(
            h->wn, h->K, h->wmax2, xmax2, h->Wst, h->n_stages, h->stage_bytes, h->stage_units, h->best64, N, 1);
    };
    bool wsqh_done = !h->ops.image_pending();
    if (wsqh_done) launch_wsqh();
    const int n_groups = (int)cdiv(h->K, EX_GROUP);
    const long chunk = std::min(exscratch::pass_rows(exact_geometry(h)), ex.pass.stride);
    ExactLaunch L{R, exact_bound(h), n_groups, ex.sw.two_round >= 0 ? ex.sw.two_round != 0 : h->wide, {}, {}};
    // THE FACTS.  Block skipping (exact_skip.hpp), one round, <= 128 features, maps of >= 4096 units: a plan needs, per row, SOME
    // unit whose distance bounds the distance to the BMU.  RESIDENT rows from their second epoch on have last epoch's BMU; every
    // other row set (query rows, streamed chunks, a row set's first epoch) -- and resident rows while last epoch's BMUs say
    // little, a schedule's first epochs -- gets a pseudo last BMU from the SCOUT.  The scout pays where a full scan costs more
    // than its own fixed part (some thirty small launches) several times over: 2 N K D flop at the screen's rate against a
    // quarter of a millisecond, i.e. from some 40 000 rows of a 256 x 256 x 128 map on.
    policy::LaunchFacts& f = L.f;
    f.resident = R.resident;
    f.have_last = R.ids_valid;
    f.rows = (const void*)X; f.n_rows = N;
    const bool scout_size_ok = ex.sw.scout_on && n_groups <= 262144 &&
                               (ex.sw.skip_mode > 1 || policy::rows_worth_a_scout((double)N, (double)h->K, (double)h->D));
    f.can_skip = exact_skip_wanted(h) && !h->wide && !L.two_round;
    f.scout_ok = f.can_skip && scout_size_ok;
    // beyond 128 features (exact_skip_wide.hpp): euclidean, resident rows with last epoch's BMUs, whole 64-unit groups
    f.wide = h->wide;
    f.wide_can = exact_skip_wanted(h) && h->wide && h->cfg.distance == SOM_DIST_EUCLIDEAN && h->K % EX_GROUP == 0 && (h->n_stages & 1) == 0;
    // (the scout there: rows without last BMUs -- queries, streamed chunks, a first epoch -- from the same break-even on)
    f.wide_scout_ok = f.wide_can && scout_size_ok;
    f.l2_fits_lds = 2 * (size_t)h->stage_bytes + (size_t)cdiv(n_groups, K16_STAGE_UNITS) * (64 * sizeof(int) + 4 * 8) <= 150 * 1024;   // (level 2's list of kept groups lives in LDS)
    f.have_lo_image = h->Wst_lo != nullptr;
    f.blocks_per_row = (double)n_groups * K16_T / (double)SK_TILE;
    f.skip_mode = ex.sw.skip_mode; f.refine_on = ex.sw.refine_on; f.sub_blocks = ex.sw.sub_blocks; f.res_every = ex.sw.res_every;

    lp = ex.plan.begin(f);
    ex.fc = som_handle::ExactScratch::Forecast{};
    ex.last_plan_tiles = 0; ex.last_plan_l2 = false;
    auto& sr = ex.srt[f.resident ? 0 : 1];
    // (the resident rows' carried positions: this launch's to use, and stale from here on unless its own finalize renews them;
    //  a launch over other rows works in srt[1] and writes other ids: it leaves them alone)
    const bool lastpos_was_valid = f.resident && sr.lastpos_valid;
    if (f.resident) sr.lastpos_valid = false;
    const int64_t run_before = ex.stats.blocks_run, total_before = ex.stats.blocks_total;
    if (lp.skip && exact_skip_reserve(h, sr, f.resident ? N : std::min(N, chunk), ex.pass.stride) != 0) {
        // no memory for the sorted pass's buffers: every block runs, from now on (the ids are the same either way)
        (void)hipGetLastError();
        if (h->debug) std::fprintf(stderr, "[somhip] exact: block skipping off (%s)\n", h->err.c_str());
        h->err.clear();
        lp.cancel(); ex.sw.skip_mode = 0;
    }
    if (lp.skip) {
        if (h->wide) { if (int rc = exact_wide_centroids(h, xmax2)) return rc; }
        else if (int rc = exact_skip_centroids(h, xmax2, wsqh_done ? 0u : wsqh_blocks, h->best64.p, N, &wsqh_done)) return rc;
    }
    if (int rc = flush_prep_w(h)) return rc;                 // (no plan, or the wide plan: the codebook's 16-bit image on its own)
    if (!wsqh_done) launch_wsqh();
    if (lp.estimate) {
        // the cheap question first (exact_scout_rowneed_kernel): 128 sampled rows against the group centroids (one small launch
        // and one host wait spent); policy::PlanState::rows_sampled cancels the plan where a row alone needs nearly every group
        const PassCtr pc = pass_ctr(h);
        const int n_samples = (int)std::min<long>(128, N);
        HIPCHK(h, hipMemsetAsync(pc.row_need(), 0, sizeof(RowNeed), h->stream));
        exact_scout_rowneed_kernel<<<dim3((unsigned)n_samples), dim3(256), (size_t)h->D * sizeof(float), h->stream>>>(
            X, N, h->D, n_samples, ex.cen.lv[0].Cc, ex.cen.lv[0].rg, n_groups, &pc.row_need()->need);
        const RowNeed* need_host = (const RowNeed*)ex.pass_host;   // (the pinned read-back is free before the first pass)
        HIPCHK(h, hipMemcpyAsync(ex.pass_host, pc.row_need(), sizeof(RowNeed), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const double need = (double)need_host->need / std::max(1.0, (double)need_host->rows * n_groups);
        if (h->debug) std::fprintf(stderr, "[somhip] exact scout: a sampled row needs %.4f of the groups\n", need);
        ex.fc.need = need; ex.fc.rows = (double)need_host->rows;
        ex.plan.rows_sampled(need, lp);
    }
    if (lp.sample_tiles && exact_skip_reserve(h, ex.srt[1], 128 * SK_TILE, ex.pass.stride) != 0) { (void)hipGetLastError(); h->err.clear(); lp.sample_tiles = false; }
    ex.share_forecast = ex.plan.share_last(f.resident);
    if (lp.refine && !sr.xl_filled) {
        // the rows' second half image (a quarter of the sorted copies' bytes) exists from the first launch that refines: the
        // order is rebuilt in that launch, so that the gather fills it
        if (sr.Xl_s == nullptr && reserve_second_half(h, sr) != 0) { (void)hipGetLastError(); h->err.clear(); lp.refine = false; }
        else lp.force_sort();
    }

    // (decided here: a refused reservation, the samples or a first refinement may have changed the plan since it began)
    L.lastpos_carried = ex.sw.chain && lastpos_was_valid && f.have_last && lp.skip && !lp.resort && !lp.scout && !h->wide && sr.lastpos_s != nullptr;
    if (L.lastpos_carried) ex.stats.lastpos_carried_epochs += 1;
    for (long r0 = 0; r0 < N; r0 += chunk)
        if (int rc = exact_pass(h, L, sr, r0, std::min(chunk, N - r0))) return rc;
    // (every pass of the epoch has stored its slice and no row went to the float32 kernel: the next epoch may skip exact_lastpos_kernel)
    if (f.resident) sr.lastpos_valid = L.pos_kept_rows == N && L.fallback_rows == 0;

    L.o.blocks_run = ex.stats.blocks_run - run_before; L.o.blocks_total = ex.stats.blocks_total - total_before;
    const policy::LaunchReport rep = ex.plan.end(f, lp, L.o);
    if (h->debug && rep.planned) {
        const policy::Costs& c = ex.plan.costs();
        const double pairs_out_row = (double)L.o.pairs_out / (double)std::max<long>(N, 1);
        if (!f.resident)
            std::fprintf(stderr, "[somhip] exact plan (transient, %ld rows): share %.4f level-1 %.4f level-2 %d refine %d pairs/row %.2f -> %.2f; %.3f ms (screen %.3f)\n",
                         N, rep.share, rep.l1_share, lp.level2 ? 1 : 0, lp.refine ? 1 : 0, rep.pairs_per_row, pairs_out_row, L.o.t_total, L.o.t_screen);
        else
            std::fprintf(stderr, "[somhip] exact plan %ld: share %.4f level-1 %.4f level-2 %d (paid %d) sorted %d scout %d (since %d, next forced at %d) refine %d pairs/row %.2f -> %.2f; "
                         "scout wins %.3f; %.3f ms (screen %.3f, level 2 %.3f, sort %.3f) [block %.3g us, level 2 per kept group %.3g us, ratio %.3f]\n",
                         (long)rep.planned_epochs, rep.share, rep.l1_share, lp.level2 ? 1 : 0, rep.level2_paid ? 1 : 0, lp.resort ? 1 : 0, lp.scout ? 1 : 0,
                         rep.epochs_since_sort, rep.next_forced_sort, lp.refine ? 1 : 0, rep.pairs_per_row, pairs_out_row, rep.win_share,
                         L.o.t_total, L.o.t_screen, L.o.t_l2, L.o.t_sort, 1e3 * c.blk_ms, 1e3 * c.l2_ms_group, c.l2_ratio);
    }
    return 0;
}
