// Host side of mips_index_remove (included by mips_hip.hip behind host_wide.hpp): stage the bitmap, read the windows' counts
// in the call's one synchronisation, plan (remove_plan.hpp) and enqueue one gather per window for every array of the index.
#pragma once

namespace {

constexpr int64_t kRemoveWindowBytes = 64ll << 20; // default window (profiles/remove/README.md)

inline int64_t remove_window_rows(const mips_index* ix) {
    if (ix->opt_remove_window > 0) return ix->opt_remove_window;
    const int64_t pitch = (int64_t)ix->ld * ix->esize; // (fp32-exact: the [hi | lo] planes and the fp32 rows share it)
    return std::max<int64_t>(mips::REM_TILE, kRemoveWindowBytes / pitch / mips::REM_TILE * mips::REM_TILE);
}

// One array ([rows][pitch bytes], pitch a multiple of 16), moved as the plan says; `bounce` holds the largest bounce move
int remove_gather_rows(const mips_remove::Plan& plan, const unsigned* keep, int64_t W, int64_t n, uint8_t* base, int64_t pitch, uint8_t* bounce,
                       hipStream_t st) {
    const int cpr = (int)(pitch / 16);
    const int seg = std::min(cpr, 256);
    for (const mips_remove::Move& m : plan.moves) {
        const int64_t row0 = m.window * W, nrows = mips_remove::window_rows(n, W, m.window);
        uint8_t* home = base + (size_t)m.base * pitch;
        const dim3 grid((unsigned)((nrows + mips::REM_TILE - 1) / mips::REM_TILE), (unsigned)((cpr + seg - 1) / seg));
        mips::remove_gather_kernel<<<grid, mips::REM_THREADS, 0, st>>>(keep, row0, n, (const mips::rem_u4*)base, (mips::rem_u4*)(m.direct ? home : bounce), cpr, seg);
        HIP_TRY(hipGetLastError());
        if (!m.direct) HIP_TRY(hipMemcpyAsync(home, bounce, (size_t)m.kept * pitch, hipMemcpyDeviceToDevice, st));
    }
    return MIPS_OK;
}

int remove_gather_labels(const mips_remove::Plan& plan, const unsigned* keep, int64_t W, int64_t n, int* labels, int* bounce, hipStream_t st) {
    for (const mips_remove::Move& m : plan.moves) {
        const int64_t row0 = m.window * W, nrows = mips_remove::window_rows(n, W, m.window);
        int* home = labels + m.base;
        mips::remove_gather_labels_kernel<<<(unsigned)((nrows + mips::REM_TILE - 1) / mips::REM_TILE), mips::REM_THREADS, 0, st>>>(
            keep, row0, n, labels, m.direct ? home : bounce);
        HIP_TRY(hipGetLastError());
        if (!m.direct) HIP_TRY(hipMemcpyAsync(home, bounce, (size_t)m.kept * sizeof(int), hipMemcpyDeviceToDevice, st));
    }
    return MIPS_OK;
}

int index_remove(mips_index* ix, const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, bool sel_dev, int64_t out_counts[2], hipStream_t st) {
    const int64_t n = ix->ntotal;
    out_counts[0] = 0;
    out_counts[1] = ix->nlabelled;
    if (n == 0) return MIPS_OK;
    // a split-tail search may still re-score on the rows from its tail stream
    int rc = wait_for_tail(ix, st, /*both_sets=*/true);
    if (rc) return rc;
    const int64_t W = remove_window_rows(ix), nwin = (n + W - 1) / W;
    const int wwords = (int)(W / 32);
    // scratch: [0, 16) the labelled survivors, then one count per window, then the keep words of whole windows
    const size_t counts_bytes = (size_t)round_up(nwin * (int64_t)sizeof(int), 16);
    rc = ix->sel_words.ensure(16 + counts_bytes + (size_t)nwin * wwords * sizeof(unsigned));
    if (rc) return rc;
    unsigned long long* lab_kept_dev = (unsigned long long*)ix->sel_words.p;
    int* kept_dev = (int*)((unsigned char*)ix->sel_words.p + 16);
    unsigned* keep = (unsigned*)((unsigned char*)ix->sel_words.p + 16 + counts_bytes);
    const uint8_t* src;
    int64_t bit0, nbytes;
    rc = bitmap_on_device(ix, sel_bits, sel_nbits, sel_bit0, sel_dev, st, src, bit0, nbytes);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(lab_kept_dev, 0, 16, st));
    mips::remove_stage_kernel<<<(unsigned)std::min<int64_t>(nwin, 1 << 16), mips::REM_THREADS, 0, st>>>(src, nbytes, bit0, n, ix->nlabelled, wwords, keep,
                                                                                                     kept_dev, nwin, lab_kept_dev);
    HIP_TRY(hipGetLastError());
    std::vector<int> kept((size_t)nwin);
    unsigned long long lab_kept = 0;
    HIP_TRY(hipMemcpyAsync(&lab_kept, lab_kept_dev, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(kept.data(), kept_dev, (size_t)nwin * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st)); // the one synchronisation of the call
    const mips_remove::Plan plan = mips_remove::make_plan(kept, W, n);
    if (plan.n_new == n) return MIPS_OK; // nothing removed: nothing touched, every cached scalar stays valid
    // the labelled prefix has its own plan: the same windows, cut at nlabelled
    mips_remove::Plan lab_plan;
    const int64_t nlab = ix->nlabelled;
    if (nlab > 0) {
        const int64_t nwl = (nlab + W - 1) / W;
        std::vector<int> kl(kept.begin(), kept.begin() + nwl);
        int64_t before = 0;
        for (int64_t w = 0; w + 1 < nwl; ++w) before += kept[w];
        kl[nwl - 1] = (int)((int64_t)lab_kept - before);
        lab_plan = mips_remove::make_plan(kl, W, nlab);
    }
    const int64_t pitch = (int64_t)ix->ld * ix->esize;
    int64_t bounce_rows = 0, bounce_labels = 0;
    for (const mips_remove::Move& m : plan.moves)
        if (!m.direct) bounce_rows = std::max(bounce_rows, m.kept);
    for (const mips_remove::Move& m : lab_plan.moves)
        if (!m.direct) bounce_labels = std::max(bounce_labels, m.kept);
    const size_t bounce_bytes = std::max((size_t)bounce_rows * pitch, (size_t)bounce_labels * sizeof(int));
    {
        // the bounce buffer lives on the stream: released behind the gathers however this block is left
        struct StreamAlloc {
            void* p = nullptr;
            hipStream_t st;
            hipError_t freed = hipSuccess;
            void release() {
                if (p) freed = hipFreeAsync(p, st);
                p = nullptr;
            }
            ~StreamAlloc() { release(); }
        } bounce{nullptr, st};
        if (bounce_bytes > 0) {
            hipError_t e = hipMallocAsync(&bounce.p, bounce_bytes, st);
            if (e != hipSuccess) return fail(MIPS_E_NOMEM, "mips_index_remove: hipMallocAsync(%zu) for the bounce buffer failed: %s", bounce_bytes, hipGetErrorString(e));
        }
        rc = remove_gather_rows(plan, keep, W, n, ix->rows, pitch, (uint8_t*)bounce.p, st);
        if (rc == MIPS_OK && ix->plane > 0)
            rc = remove_gather_rows(plan, keep, W, n, (uint8_t*)ix->rows_f32.p, (int64_t)ix->plane * sizeof(float), (uint8_t*)bounce.p, st);
        if (rc == MIPS_OK && nlab > 0) rc = remove_gather_labels(lab_plan, keep, W, nlab, ix->labels, (int*)bounce.p, st);
        bounce.release();
        if (rc == MIPS_OK && bounce.freed != hipSuccess) rc = fail(MIPS_E_HIP, "mips_index_remove: hipFreeAsync failed: %s", hipGetErrorString(bounce.freed));
    }
    if (rc) return rc; // (rows may have moved already: the index is to be reset)
    ix->ntotal = plan.n_new;
    ix->nlabelled = nlab > 0 ? lab_plan.n_new : 0;
    rows_changed(ix, plan.first_row); // (the rows before the first window that lost a row did not move)
    out_counts[0] = n - plan.n_new;
    out_counts[1] = ix->nlabelled;
    return MIPS_OK;
}

} // namespace
