// lin_diag.h -- what a tuning build (-DJH_TUNING, tools/build_variants.sh) prints about a check.
// Part of jh_lin.hip's translation unit (included there after LinRun). Every
// function checks its own knob and returns at once in the release library
// (tune_env is nullptr there); none of them launches a search.
#pragma once

namespace {

// JH_DEBUG>=2: phase 1's per-wave counters
void LinRun::diag_phase1_waves() {
    if (!dbg2) return;
    std::vector<unsigned long long> h((size_t)waves1 * 16);
    HIP_TRY(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long tot[16] = {0}, mx9 = 0;
    for (int w = 0; w < waves1; w++) { for (int k = 0; k < 16; k++) tot[k] += h[16 * w + k]; mx9 = std::max(mx9, h[16 * w + 9]); }
    fprintf(stderr, "[jh-dfs] waves=%d keys=%llu search=%.0f cyc/key | steps=%llu inserts=%llu evict=%llu lay-loads=%llu op-loads=%llu spills=%llu refills=%llu slow=%llu hbm-probes=%llu hbm-inserts=%llu | cyc/step=%.0f | wave-busy avg=%.0f max=%llu cyc\n",
            waves1, tot[3], (double)tot[2] / std::max(1ULL, tot[3]), tot[4], tot[5], tot[6], tot[7], tot[10],
            tot[11], tot[12], tot[13], tot[14], tot[8], (double)tot[2] / std::max(1ULL, tot[4]), (double)tot[9] / waves1, mx9);
    HIP_TRY(hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * (waves1 + 512) * 16, st));
}

// JH_DEBUG=4: what the late helpers took (end time in us after their start)
void LinRun::diag_helper_keys() {
    if (!(n_help > 0 && wh.key_prof)) return;
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<unsigned long long> kp(3 * (size_t)K);
    HIP_TRY(hipMemcpy(kp.data(), wh.key_prof, kp.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < K; k++)
        if (kp[3 * k])
            fprintf(stderr, "[jh-help] key %lld wg %llu verdict %llu won %llu inserts %llu cycles %llu end_us %llu\n",
                    (long long)k, (kp[3 * k + 2] >> 8) & 0xFFF, kp[3 * k + 2] & 0xFF, (kp[3 * k + 2] >> 20) & 1,
                    kp[3 * k + 1], kp[3 * k], kp[3 * k + 2] >> 32);
}

// JH_BFS_DUMP: workgroup 0's stored configurations (t:20 | s:12 | mask:32)
void LinRun::diag_bfs_dump() {
    const char *dp = tune_env("JH_BFS_DUMP");
    if (!dp) return;
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> nd(c.ncap);
    HIP_TRY(hipMemcpy(nd.data(), c.nodes, nd.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *fp = fopen(dp, "wb")) { fwrite(nd.data(), 8, nd.size(), fp); fclose(fp); }
}

// JH_DEBUG>=2: the race's per-workgroup (BFS) and per-wave (sequential) counters
void LinRun::diag_race_waves() {
    if (!dbg2) return;
    HIP_TRY(hipMemcpyAsync(qh, q, sizeof qh, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    n_unres = qh[Q_UNRES];
    std::vector<unsigned long long> h((size_t)wg2 * 16);
    HIP_TRY(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
    for (int w = 0; w < wg2; w++)
        if (h[16 * w + 4])
            fprintf(stderr, "[jh-bfs] wg %d keys=%llu cycles=%llu rounds=%llu configs=%llu cyc/round=%.0f | "
                    "count: hash=%llu live=%llu path=%llu closure=%llu cyc | global-set rounds=%llu cyc=%llu "
                    "configs=%llu, LDS-set rounds cyc=%llu configs=%llu | live: layers=%llu (LDS %llu) head-cyc=%llu LDS-layers-cyc=%llu\n",
                    w, h[16 * w + 4], h[16 * w], h[16 * w + 1], h[16 * w + 3],
                    (double)h[16 * w] / std::max(1ULL, h[16 * w + 1]), h[16 * w + 5], h[16 * w + 6],
                    h[16 * w + 7], h[16 * w + 8], h[16 * w + 10], h[16 * w + 9], h[16 * w + 11],
                    h[16 * w + 12], h[16 * w + 13], h[16 * w + 14] & 0xFFFFFFFF, h[16 * w + 14] >> 32, h[16 * w + 15], h[16 * w + 2]);
#ifdef JH_BFS_PROF
    {
        unsigned long long bp[8];
        HIP_TRY(hipMemcpyFromSymbol(bp, HIP_SYMBOL(g_bfs_prof), sizeof bp));
        const double nr = (double)std::max(1ULL, bp[4]), nl = (double)std::max(1ULL, bp[6]);
        unsigned long long bx[4];
        HIP_TRY(hipMemcpyFromSymbol(bx, HIP_SYMBOL(g_bfs_prof_x), sizeof bx));
        const double ni = (double)std::max(1ULL, bx[2]);
        fprintf(stderr, "[jh-bfs-prof] rounds=%llu cyc/round: claim+barrier %.0f items %.0f barrier %.0f tail %.0f | "
                "layers=%llu formation cyc/layer %.0f | tid0 items=%llu cyc/item: load+children %.0f insert8 %.0f record8 %.0f\n",
                bp[4], bp[0] / nr, bp[1] / nr, bp[2] / nr, bp[3] / nr, bp[6], bp[5] / nl, bx[2], bp[7] / ni, bx[0] / ni, bx[1] / ni);
        memset(bx, 0, sizeof bx);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bfs_prof_x), bx, sizeof bx));
        memset(bp, 0, sizeof bp);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bfs_prof), bp, sizeof bp));
    }
#endif
    std::vector<unsigned long long> g((size_t)waves2 * 16);
    HIP_TRY(hipMemcpy(g.data(), dbg + 16 * 256, g.size() * 8, hipMemcpyDeviceToHost));
    for (int w = 0; w < waves2; w++)
        if (g[16 * w + 4] > 0)
            fprintf(stderr, "[jh-seq] wave %d keys=%llu search=%llu cyc busy=%llu | steps=%llu inserts=%llu evict=%llu lay-loads=%llu op-loads=%llu spills=%llu refills=%llu slow=%llu hbm-probes=%llu | cyc/step=%.0f\n",
                    w, g[16 * w + 3], g[16 * w + 2], g[16 * w + 9], g[16 * w + 4], g[16 * w + 5], g[16 * w + 6],
                    g[16 * w + 7], g[16 * w + 10], g[16 * w + 11], g[16 * w + 12], g[16 * w + 13], g[16 * w + 14],
                    (double)g[16 * w + 2] / std::max(1ULL, g[16 * w + 4]));
}

// JH_DEFER_TIMES: the timeline -- when each deferred key was handed on (us
// after phase 1's first wave), when phase 1 ended, when the sequential search
// took the key (if helpers ran), and the key's final insert count
void LinRun::diag_defer_timeline() {
    if (!(defer_times && n_defer > 0)) return;
    HIP_TRY(hipStreamSynchronize(st));
    if (stream_p2) {
        int32_t nd = 0;
        HIP_TRY(hipMemcpy(&nd, q + Q_DEFER, sizeof nd, hipMemcpyDeviceToHost));
        n_defer = nd;
    }
    std::vector<unsigned long long> dt((size_t)K + 2);
    HIP_TRY(hipMemcpy(dt.data(), a.defer_time, dt.size() * 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> dk(n_defer);
    HIP_TRY(hipMemcpy(dk.data(), defer, sizeof(int32_t) * n_defer, hipMemcpyDeviceToHost));
    std::vector<jh_key_verdict> vv(K);
    HIP_TRY(hipMemcpy(vv.data(), out_dev, sizeof(jh_key_verdict) * K, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> ss;
    if (ctx->bufs.size() > WS_HELP_START && ctx->bufs[WS_HELP_START].p) {
        ss.resize(K);
        HIP_TRY(hipMemcpy(ss.data(), ctx->bufs[WS_HELP_START].p, 8 * K, hipMemcpyDeviceToHost));
    }
    fprintf(stderr, "[jh-defer] phase 1: %.1f us (first wave start to last wave end)\n", (dt[1] - dt[0]) / 100.0);
    std::vector<std::pair<double, int>> ev;
    for (int d = 0; d < n_defer; d++) ev.push_back({(dt[2 + dk[d]] - dt[0]) / 100.0, dk[d]});
    std::vector<std::pair<long long, int>> heavy;
    for (int d = 0; d < n_defer; d++) heavy.push_back({vv[dk[d]].explored, dk[d]});
    std::sort(heavy.rbegin(), heavy.rend());
    std::vector<unsigned long long> tl;
    if (ctx->bufs.size() > WS_TL && ctx->bufs[WS_TL].p) {
        tl.resize(TL_W * (size_t)K);
        HIP_TRY(hipMemcpy(tl.data(), ctx->bufs[WS_TL].p, 8 * tl.size(), hipMemcpyDeviceToHost));
    }
    auto us = [&](unsigned long long t) { return t ? (double)(t - dt[0]) / 100.0 : -1.0; };
    for (int i = 0; i < std::min(n_defer, 12); i++) {
        const int k = heavy[i].second;
        double st_us = -1;
        if (!ss.empty() && ss[k] && ss[k] != SEQ_HANDED) st_us = ((ss[k] & ~1ULL) - dt[0]) / 100.0;
        fprintf(stderr, "[jh-defer] key %d explored %lld valid %d deferred %.1f us seq-start %.1f us", k,
                heavy[i].first, vv[k].valid, (dt[2 + k] - dt[0]) / 100.0, st_us);
        if (!tl.empty())
            fprintf(stderr, " | bfs %.1f-%.1f us seq %.1f-%.1f us", us(tl[TL_W * k]), us(tl[TL_W * k + 1]),
                    us(tl[TL_W * k + 2]), us(tl[TL_W * k + 3]));
        fprintf(stderr, "\n");
    }
    if (!tl.empty()) {
        // the keys that ended last (the step's critical path)
        std::vector<std::pair<unsigned long long, int>> last;
        for (int d = 0; d < n_defer; d++) {
            const int k = dk[d];
            unsigned long long e = 0;
            for (int w = 1; w < TL_W; w += 2) e = std::max(e, tl[TL_W * k + w]);
            last.push_back({e, k});
        }
        std::sort(last.rbegin(), last.rend());
        for (int i = 0; i < std::min(n_defer, 8); i++) {
            const int k = last[i].second;
            fprintf(stderr, "[jh-last] key %d explored %lld valid %d deferred %.1f | bfs %.1f-%.1f seq %.1f-%.1f help %.1f-%.1f us\n",
                    k, (long long)vv[k].explored, vv[k].valid, (dt[2 + k] - dt[0]) / 100.0, us(tl[TL_W * k]),
                    us(tl[TL_W * k + 1]), us(tl[TL_W * k + 2]), us(tl[TL_W * k + 3]), us(tl[TL_W * k + 4]),
                    us(tl[TL_W * k + 5]));
        }
    }
    if (const char *csv = tune_env("JH_TL_CSV")) {
        // every deferred key: its quick search, its engines' times, its verdict
        std::vector<unsigned long long> di(2 * (size_t)K);
        HIP_TRY(hipMemcpy(di.data(), a.defer_info, 8 * di.size(), hipMemcpyDeviceToHost));
        if (FILE *fo = fopen(csv, "a")) {
            fprintf(fo, "key,explored,valid,deferred_us,p1_inserts,p1_tmax,n_ok,bfs0,bfs1,seq0,seq1,help0,help1\n");
            for (int d = 0; d < n_defer; d++) {
                const int k = dk[d];
                fprintf(fo, "%d,%lld,%d,%.1f,%llu,%llu,%llu", k, (long long)vv[k].explored, vv[k].valid,
                        (dt[2 + k] - dt[0]) / 100.0, di[2 * k], di[2 * k + 1] & 0xFFFFFFFFull, di[2 * k + 1] >> 32);
                for (int w = 0; w < TL_W; w++) fprintf(fo, ",%.1f", tl.empty() ? -1.0 : us(tl[TL_W * k + w]));
                fprintf(fo, "\n");
            }
            fclose(fo);
        }
    }
    int q5[5] = {0, 0, 0, 0, 0};
    for (auto &e2 : ev) q5[std::min(4, (int)(e2.first / (std::max(1.0, (dt[1] - dt[0]) / 100.0) / 5)))]++;
    fprintf(stderr, "[jh-defer] deferrals by fifth of phase 1: %d %d %d %d %d\n", q5[0], q5[1], q5[2], q5[3], q5[4]);
}

// JH_DEBUG>=3, after a workgroup-engine watchdog: each workgroup's enumeration trace
void LinRun::diag_acc_trace() {
    if (!((qh[Q_FLAGS] & QF_WG_WATCHDOGS) && acc_stats && ctx->bufs.size() > WS_DEBUG_WG && ctx->bufs[WS_DEBUG_WG].p && n_wg > 0 &&
          dbgenv && atoi(dbgenv) >= 3))
        return;
    std::vector<unsigned long long> tr((size_t)n_wg * 256);
    HIP_TRY(hipMemcpy(tr.data(), ctx->bufs[WS_DEBUG_WG].p, tr.size() * 8, hipMemcpyDeviceToHost));
    for (int g = 0; g < n_wg; g++) {
        for (int e = 0; e < 31; e++) {
            const unsigned long long *d8 = &tr[(size_t)g * 256 + 8 * e];
            if (!d8[3]) break;
            fprintf(stderr, "[jh-acc] wg %d key %llu d %llu depth %llu roots %llu cap %llu status %llu tail %llu ins %llu\n",
                    g, d8[0], d8[1], d8[2], d8[3], d8[4], d8[5], d8[6], d8[7]);
        }
        const unsigned long long *w8 = &tr[(size_t)g * 256 + 248];
        if (w8[6] == 0xDEAD)
            fprintf(stderr, "[jh-acc] wg %d WATCHDOG head %llu tail %llu active %llu cap_total %llu roots %llu wave %llu\n",
                    g, w8[0], w8[1], w8[2], w8[3], w8[4], w8[5]);
        const unsigned long long *l8 = &tr[(size_t)g * 256 + 240];
        if (l8[3] == 0xBEEF)
            fprintf(stderr, "[jh-acc] wg %d LOST ITEM pos %llu tail %llu cap_total %llu\n", g, l8[0], l8[1], l8[2]);
    }
}

// JH_WS_REPORT: the context's workspace, largest buffers first
void LinRun::diag_ws_report() {
    if (!tune_env("JH_WS_REPORT")) return;
    std::vector<std::pair<size_t, int>> b;
    size_t tot = 0;
    for (int i = 0; i < (int)ctx->bufs.size(); i++) { b.push_back({ctx->bufs[i].bytes, i}); tot += ctx->bufs[i].bytes; }
    std::sort(b.rbegin(), b.rend());
    fprintf(stderr, "[jh-ws] total %.2f GB:", tot / 1073741824.0);
    for (size_t i = 0; i < b.size() && i < 12; i++) fprintf(stderr, " slot %d %.2f GB;", b[i].second, b[i].first / 1073741824.0);
    fprintf(stderr, "\n");
}

// -DJH_XW_PROF: k_lin_xw's cycle counters
void LinRun::diag_xw_prof() {
#ifdef JH_XW_PROF
    if (n_x > 0) {
        unsigned long long x[12];
        HIP_TRY(hipMemcpyFromSymbol(x, HIP_SYMBOL(g_xw_prof), sizeof x));
        const double ni = (double)std::max(1ULL, x[5]);
        fprintf(stderr, "[jh-xw-prof] keys=%llu inserts=%llu cyc/insert: search %.0f | probe %.0f (%.2f slice probes) "
                "push %.0f lift %.0f | layer loads %.2f x %.0f cyc | pops %.2f x %.0f cyc (HBM frames %llu)\n",
                x[11], x[5], x[0] / ni, x[1] / ni, x[6] / ni, x[4] / ni, x[9] / ni, x[7] / ni,
                x[2] / (double)std::max(1ULL, x[7]), x[8] / ni, x[3] / (double)std::max(1ULL, x[8]), x[10]);
        memset(x, 0, sizeof x);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_xw_prof), x, sizeof x));
    }
#endif
}

// JH_DEBUG: the call's phases in one line, then the workgroup engine's and
// the enumeration's counters (after fill_summary: it prints sum's fields)
void LinRun::diag_summary() {
    if (!dbgenv) return;
    float a = 0, b = 0, c = 0;
    HIP_TRY(hipEventElapsedTime(&a, ctx->ev[EV_START], ctx->ev[EV_P1_START]));
    HIP_TRY(hipEventElapsedTime(&b, ctx->ev[EV_P1_START], ctx->ev[EV_P1_END]));
    float d = 0;
    HIP_TRY(hipEventElapsedTime(&d, ctx->ev[EV_P1_END], ctx->ev[EV_SEQ_END]));
    HIP_TRY(hipEventElapsedTime(&c, ctx->ev[EV_P1_END], ctx->ev[EV_BFS_END]));
    fprintf(stderr, "[jh] keys=%lld prep=%.3f ms phase1=%.3f ms (waves %d) deferred=%d (wide %d) bfs=%.3f ms (gave up %d) "
            "seq=%.3f ms (phase 2 %.3f ms, phase 3 %lld keys %.3f ms) wide %.3f ms (%d waves, phase 3 %lld keys) "
            "xw %d keys %.3f ms (%d waves)\n",
            (long long)K, a, b, waves1, n_defer, n_def_w, c, n_unres, d, sum->seq_ms, (long long)sum->n_phase3,
            sum->p3_ms, sum->wide_ms, waves_w, (long long)sum->n_phase3_wide, n_x, sum->xw_ms, waves_x);
    if (acc_stats && dbgenv && atoi(dbgenv) >= 3 && n_wg > 0) {
        std::vector<unsigned long long> tr((size_t)n_wg * 256);
        HIP_TRY(hipMemcpy(tr.data(), ctx->bufs[WS_DEBUG_WG].p, tr.size() * 8, hipMemcpyDeviceToHost));
        for (int g = 0; g < std::min(n_wg, 8); g++)
            for (int e = 0; e < 32; e++) {
                const unsigned long long *d8 = &tr[(size_t)g * 256 + 8 * e];
                if (!d8[3]) break;
                fprintf(stderr, "[jh-acc] wg %d key %llu d %llu depth %llu roots %llu cap %llu status %llu tail %llu ins %llu\n",
                        g, d8[0], d8[1], d8[2], d8[3], d8[4], d8[5], d8[6], d8[7]);
            }
    }
    if (acc_stats && dbgenv && atoi(dbgenv) >= 4) {
        std::vector<unsigned long long> kp(3 * (size_t)K);
        HIP_TRY(hipMemcpy(kp.data(), ctx->bufs[WS_STATS_KEYS].p, kp.size() * 8, hipMemcpyDeviceToHost));
        std::vector<int> ix;
        for (int64_t k = 0; k < K; k++) if (kp[3 * k]) ix.push_back((int)k);
        std::sort(ix.begin(), ix.end(), [&](int x, int y) { return kp[3 * x] > kp[3 * y]; });
        for (size_t i = 0; i < std::min<size_t>(12, ix.size()); i++)
            fprintf(stderr, "[jh-key] key %d memtime %.3g inserts %llu verdict %llu wg %llu\n", ix[i],
                    (double)kp[3 * ix[i]], kp[3 * ix[i] + 1], kp[3 * ix[i] + 2] & 255, kp[3 * ix[i] + 2] >> 8);
    }
#ifdef JH_ENUM_PROF
    {
        unsigned int a4[4]; unsigned long long b3[3];
        HIP_TRY(hipMemcpyFromSymbol(a4, HIP_SYMBOL(g_prof_hbm), 4));
        HIP_TRY(hipMemcpyFromSymbol(a4 + 1, HIP_SYMBOL(g_prof_gset), 4));
        HIP_TRY(hipMemcpyFromSymbol(a4 + 2, HIP_SYMBOL(g_prof_rounds), 4));
        HIP_TRY(hipMemcpyFromSymbol(a4 + 3, HIP_SYMBOL(g_prof_layers), 4));
        HIP_TRY(hipMemcpyFromSymbol(b3, HIP_SYMBOL(g_prof_form), 8));
        HIP_TRY(hipMemcpyFromSymbol(b3 + 1, HIP_SYMBOL(g_prof_close), 8));
        fprintf(stderr, "[jh-prof] hbm-probes %u gset-inserts %u rounds %u layers %u | memtime formation %.3g closure %.3g\n",
                a4[0], a4[1], a4[2], a4[3], (double)b3[0], (double)b3[1]);
        unsigned int z4[4] = {0, 0, 0, 0}; unsigned long long zb[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof_hbm), z4, 4));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof_gset), z4, 4));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof_rounds), z4, 4));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof_layers), z4, 4));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof_form), zb, 8));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof_close), zb, 8));
    }
#endif
    if (acc_stats) {
        unsigned long long st8[8];
        HIP_TRY(hipMemcpy(st8, acc_stats, sizeof st8, hipMemcpyDeviceToHost));
        fprintf(stderr, "[jh-wg] workgroups=%d enumerations=%llu new-nodes=%llu dead=%llu live=%llu inconclusive=%llu | "
                "memtime: keys %.3g, in enumerations %.3g (work loops %.3g)\n",
                n_wg, st8[0], st8[1], st8[2], st8[3], st8[4], (double)st8[7], (double)st8[5], (double)st8[6]);
    }
}

}  // namespace
