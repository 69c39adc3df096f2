// precision 'exact', TOP-2: the host side of the second-smallest window (bmu_exact.hpp, "TOP-2") -- the screen's T2 instance over
// every block, one select on m2 + E, the float32 re-score twice over the same tiles (round 2 without round 1's winner), the
// sqrt'd distance's tie test on both units, the float32 top-2 kernel for the rows that are left.
// Included by somhip.hip INSIDE its anonymous namespace, behind exact_host.hpp and the query helpers (row_sq, launch_bmu_top2):
// one translation unit.  The launch takes no plan, no scout and no resident order, and it leaves the policy's state alone:
// ExactScratch::plan, ::lp, ::cost and the screen's block counters are not touched, and the pass scratch is only ever GROWN
// (which forgets a resident order) while there is no resident order to forget -- otherwise the rows go in passes of the
// scratch there is.
// (no #pragma once / include guard on purpose: not a header of its own)

// does the screen serve this handle's top-2 calls?  (the codebook images are the euclidean ones up to 128 features)
bool exact_top2_fast(const som_handle* h) {
    return h->exact && !h->wide && !h->tiled && h->cfg.distance == SOM_DIST_EUCLIDEAN && h->D <= 128 && h->K >= 2 && h->t2.on;
}

template <int KS32>
int exact_top2_screen(som_handle* h, const __bf16* Xb, long n, unsigned long long* best64, const float* xsq, const float* xerr,
                      const float* xmax2, const ExactBound& eb, int* parts_out, long* pitch_out) {
    const void* kern = (const void*)bmu_bf16_k16_kernel<KS32, ExactEl, true, false, true>;
    const size_t lds = 2 * (size_t)k16_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, kern, 64 * K16_NW, lds, &per_cu)) return rc;
    const long blocks = cdiv(n, K16_WG_SAMPLES);
    const long slots = resident_slots(h, per_cu);
    int parts = choose_parts(h, blocks, slots, h->n_stages);
    if (h->env_bf16_parts > 0) parts = std::min(h->env_bf16_parts, h->n_stages);
    const long pitch = round_up(n, 256);
    if (int rc = h->t2.m.reserve(h, (size_t)2 * parts * pitch, 1024)) return rc;
    if (h->debug)
        std::fprintf(stderr, "[somhip] exact top-2 screen: blocks=%ld per_cu=%d slots=%ld parts=%d groups=%d\n", blocks, per_cu, slots,
                     parts, (int)cdiv(h->K, EX_GROUP));
    bmu_bf16_k16_kernel<KS32, ExactEl, true, false, true><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * K16_NW), lds, h->stream>>>(
        Xb, n, h->Wst, h->n_stages, h->K, best64, h->ex.pass.gmin, h->ex.pass.stride, h->ex.pass.gflags, xsq, xerr, xmax2, h->wmax2, h->wmax2 + 1, eb,
        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h->t2.m, pitch);
    *parts_out = parts; *pitch_out = pitch;
    return 0;
}
int exact_top2_screen_ks(som_handle* h, const __bf16* Xb, long n, unsigned long long* best64, const float* xsq, const float* xerr,
                         const float* xmax2, const ExactBound& eb, int* parts_out, long* pitch_out) {
    return for_ks32(h, "exact top-2: the screen kernel supports input_len <= 128", [&](auto k) {
        return exact_top2_screen<decltype(k)::value>(h, Xb, n, best64, xsq, xerr, xmax2, eb, parts_out, pitch_out); });
}

// round 2: the tiles of round 1 once more, every row's argmin without the unit at excl[row]
template <int KG>
int exact_top2_rescore_kg(som_handle* h, const float* X, unsigned long long* best64, const int* excl) {
    auto& ex = h->ex;
    auto kern = exact_rescore_mfma_kernel<KG, true>;
    const size_t lds = (size_t)fr_stage_bytes(KG);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 256, lds, &per_cu)) return rc;
    const long grid = std::min<long>(ex.pass.max_tiles, ex.sw.grid_mult * resident_slots(h, per_cu));
    kern<<<dim3((unsigned)grid), dim3(256), lds, h->stream>>>(X, h->D, h->Wfst, h->K, ex.pass.tile_tab, &pass_ctr(h).tail()->n_tiles, ex.pass.plist,
                                                             best64, h->ex_perm, nullptr, h->ex_sub44 ? 1 : 0, 0, excl);
    return 0;
}
int exact_top2_rescore(som_handle* h, const float* X, unsigned long long* best64, const int* excl) {
    switch (h->fr_kg) {
    case 1: return exact_top2_rescore_kg<1>(h, X, best64, excl);
    case 2: return exact_top2_rescore_kg<2>(h, X, best64, excl);
    case 4: return exact_top2_rescore_kg<4>(h, X, best64, excl);
    case 8: return exact_top2_rescore_kg<8>(h, X, best64, excl);
    case 16: return exact_top2_rescore_kg<16>(h, X, best64, excl);
    }
    return fail(h, "exact top-2: bad k-group count");
}

// the float32 top-2 kernel on the n_list rows of `list` (indices into the pass), its pairs scattered back
int exact_top2_list_rows(som_handle* h, const float* X, const int* list, int n_list, int* out1, int* out2) {
    auto& t2 = h->t2;
    if (int rc = t2.X.reserve(h, (size_t)n_list * h->D, (size_t)1024 * h->D)) return rc;
    if (int rc = t2.xsq.reserve(h, (size_t)n_list, 1024)) return rc;
    if (int rc = t2.ids1.reserve(h, (size_t)n_list, 1024)) return rc;
    if (int rc = t2.ids2.reserve(h, (size_t)n_list, 1024)) return rc;
    // the float32 kernel names units by their place in its image: the units' own order for it
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    exact_gather_rows_kernel<<<dim3((unsigned)cdiv((long)n_list * h->D, 256)), dim3(256), 0, h->stream>>>(X, list, n_list, h->D, t2.X);
    row_sq_f32_kernel<<<dim3((unsigned)cdiv(n_list, 256)), dim3(256), 0, h->stream>>>(t2.X, n_list, h->D, t2.xsq);
    if (int rc = launch_bmu_top2(h, t2.X, n_list, t2.xsq, t2.ids1, t2.ids2)) return rc;
    exact_scatter_ids2_kernel<<<dim3((unsigned)cdiv(n_list, 256)), dim3(256), 0, h->stream>>>(t2.ids1, t2.ids2, list, n_list, out1, out2);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ONE PASS over the rows [r0, r0 + n): best1 / best2 are the pass's slices of the two rounds' merge keys.  *bad_w: the codebook
// holds a unit the scheme does not cover (the caller hands every row to the float32 kernel).
int exact_top2_pass(som_handle* h, const Rows& R, const ExactBound& eb, long r0, long n, unsigned long long* best1, unsigned long long* best2,
                    bool* bad_w) {
    const float* X = R.X; const float* xsq = R.xsq; const float* xerr = R.xerr; const __bf16* Xb = R.Xb; const float* xmax2 = R.xmax2;
    int* out1 = R.out; int* out2 = R.out2;
    auto& ex = h->ex;
    const PassCtr pc = pass_ctr(h);
    const int n_groups = pc.n_groups;
    // (a pass behind one whose listed rows went through the float32 kernel: its image back in patch order)
    if (h->ops.f32_in_patch_order() != h->ex_patch) if (int rc = refresh_codebook_operands(h, operands::Request::ExactScreen)) return rc;
    HIPCHK(h, hipMemsetAsync(pc.base, 0, pc.bytes(), h->stream));
    int parts = 1;
    long pitch = 0;
    {
        Timed ts(h, SOM_K_SCREEN);
        if (int rc = exact_top2_screen_ks(h, Xb + r0 * h->dp, n, best1, xsq + r0, xerr + r0, xmax2, eb, &parts, &pitch)) return rc;
    }
    exact_select_kernel<false, true><<<dim3((unsigned)cdiv(n, 64)), dim3(64 * EX_SCAN_SPLIT), 0, h->stream>>>(
        ex.pass.gmin, ex.pass.gflags, ex.pass.stride, n_groups, n, best1, xsq + r0, h->wmax2, xmax2, eb, xerr + r0, h->wmax2 + 1, ex.pass.plist, pc.gcount(),
        ex.pass.rowcnt, nullptr, nullptr, nullptr, nullptr, 0, h->t2.m, parts, pitch);
    // round 1: the tiles, the float32 first minimum k1; round 2: the same tiles without k1
    if (int rc = exact_rescore_round(h, X + r0 * h->D, xsq + r0, best1, nullptr, nullptr, false, true)) return rc;
    exact_top2_first_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(best1, n, h->K, h->ex_patch ? h->ex_inv.p : nullptr,
                                                                                     h->t2.excl);
    if (int rc = exact_top2_rescore(h, X + r0 * h->D, best2, h->t2.excl)) return rc;
    exact_top2_settle_kernel<<<dim3((unsigned)cdiv(std::max<long>(n, h->K), 256)), dim3(256), 0, h->stream>>>(
        best1, best2, n, h->K, xsq + r0, h->wsq, &pc.tail()->overflow, out1 + r0, out2 + r0, ex.pass.fb_list, &pc.tail()->fallback,
        &pc.tail()->bad_w);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(ex.pass_host, pc.tail(), sizeof(PassCounters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const PassCounters& got = *ex.pass_host;
    if (got.bad_w) { *bad_w = true; return 0; }
    const int n_list = got.fallback;
    if (n_list < 0 || n_list > n) return fail(h, "exact top-2: list counter out of range");
    h->t2.rows_f32 += n_list;
    if (h->debug)
        std::fprintf(stderr, "[somhip] exact top-2 pass: %ld rows, %d pairs (%.2f a row), %d rows to the float32 kernel%s\n", n, got.pairs_in,
                     (double)got.pairs_in / (double)n, n_list, got.overflow ? " (overflow)" : "");
    if (n_list > 0) return exact_top2_list_rows(h, X + r0 * h->D, ex.pass.fb_list, n_list, out1 + r0, out2 + r0);
    return 0;
}

// R: the query rows, their |x|^2 and measured operand errors, their half image; out / out2: the ids
int launch_top2_exact(som_handle* h, const Rows& R) {
    if (h->capturing) return fail(h, "precision 'exact' reads a counter back per pass: not capturable");
    if (!R.xsq || !R.xerr) return fail(h, "exact top-2: no row norms");
    const long N = R.N;
    auto& ex = h->ex;
    // the pass scratch: what there is, unless there is none -- or too little and no resident order that growing it would forget
    if (ex.pass.stride == 0 || (ex.pass.stride < exscratch::first_stride(exact_geometry(h), N, 0) && !ex.plan.order_valid()))
        if (int rc = exact_reserve(h, N)) return rc;
    const long chunk = std::min(exscratch::pass_rows(exact_geometry(h)), ex.pass.stride);
    const long off2 = round_up(N, 1024);                         // (round 2's merge keys behind round 1's)
    if (int rc = h->best64.reserve(h, (size_t)(off2 + N), 1024)) return rc;
    if (int rc = h->t2.excl.reserve(h, (size_t)std::min(N, chunk), 1024)) return rc;
    const long units = (long)h->n_stages * h->stage_units;
    prep_wsqh_kernel<<<dim3((unsigned)cdiv(std::max(units, N), 256)), dim3(256), 0, h->stream>>>(
        h->wn, h->K, h->wmax2, R.xmax2, h->Wst, h->n_stages, h->stage_bytes, h->stage_units, h->best64, N, 1);
    HIPCHK(h, hipMemsetAsync(h->best64 + off2, 0xFF, (size_t)N * sizeof(unsigned long long), h->stream));
    const ExactBound eb = exact_bound(h);
    h->t2.rows += N;
    const int64_t f32_before = h->t2.rows_f32;
    for (long r0 = 0; r0 < N; r0 += chunk) {
        bool bad_w = false;
        if (int rc = exact_top2_pass(h, R, eb, r0, std::min(chunk, N - r0), h->best64 + r0, h->best64 + off2 + r0, &bad_w)) return rc;
        if (bad_w) {
            // a unit with a NaN or infinite norm: the float32 kernel for every row of the call
            h->t2.rows_f32 = f32_before + N;
            if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
            return launch_bmu_top2(h, R.X, N, R.xsq, R.out, R.out2);
        }
    }
    return 0;
}
