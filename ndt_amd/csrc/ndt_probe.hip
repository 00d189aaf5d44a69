// ndt_probe.hip -- what the diagnostics of a profiled pass print to stderr (NDT_HIP_STREAM_PROBE, NDT_HIP_SHADE_PROBE,
// NDT_HIP_EXIT_PROBE, NDT_PHASE_TIMING builds).  render_pass calls them after the frame has completed; profiles/stream_probe.py,
// levels_probe.py and exit_probe.py parse the lines.
#include "ndt_ctx.hpp"

// NDT_HIP_STREAM_PROBE: what every wavefront of the frame kernel did and when (100 MHz ticks)
void ndt_impl::print_stream_probe(const unsigned int *wave_log, float km)
{
    std::vector<unsigned int> log((size_t)24 * NDT_STREAM_LOG_WAVES);
    if (hipMemcpy(log.data(), wave_log, log.size() * sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned long long n[4] = { 0, 0, 0, 0 }, t[3] = { 0, 0, 0 }, parts[5] = { 0, 0, 0, 0, 0 };
    int waves = 0, busy_waves = 0;
    unsigned int t0 = 0, max_items = 0;
    bool any = false;
    for (int w = 0; w < NDT_STREAM_LOG_WAVES; ++w) {
        const unsigned int *q = &log[(size_t)24 * w];
        if (!q[9]) continue;
        if (!any || (int)(q[10] - t0) < 0) t0 = q[10];
        any = true;
    }
    double first_item = 1e30, last_item = 0, last_exit = 0, start_spread = 0;
    int hist[32] = { 0 };
    for (int w = 0; w < NDT_STREAM_LOG_WAVES; ++w) {
        const unsigned int *q = &log[(size_t)24 * w];
        if (!q[9]) continue;
        ++waves;
        const unsigned int items = q[0] + q[1] + q[2];
        if (items) ++busy_waves;
        if (items > max_items) max_items = items;
        for (int k = 0; k < 4; ++k) n[k] += q[k];
        for (int k = 0; k < 3; ++k) t[k] += q[4 + k];
        for (int k = 0; k < 5; ++k) parts[k] += q[12 + k];
        const double off = (q[10] - t0) / 100.0;
        if (off > start_spread) start_spread = off;
        if (q[7] && off + q[7] / 100.0 < first_item) first_item = off + q[7] / 100.0;
        if (off + q[8] / 100.0 > last_item) last_item = off + q[8] / 100.0;
        if (off + q[9] / 100.0 > last_exit) last_exit = off + q[9] / 100.0;
        int bin = (int)((off + q[8] / 100.0) / (km * 1000.0 / 32.0 + 1e-9));
        ++hist[bin < 0 ? 0 : bin > 31 ? 31 : bin];
    }
    std::string line;
    for (int b = 0; b < 32; ++b) {
        char buf[16];
        snprintf(buf, sizeof buf, " %d", hist[b]);
        line += buf;
    }
    fprintf(stderr, "ndt_hip: frame kernel %.3f ms: %d wavefronts (%d with work, at most %u items each) started within %.1f us; "
                    "node batches %llu (%.1f us each), shadow batches %llu (%.1f us each), lighting batches %llu (%.1f us each), "
                    "idle rounds %llu; first item at %.1f us, last item done at %.1f us, last exit at %.1f us; "
                    "wavefronts by the 32nd of the kernel in which they finished their last item:%s\n",
            km, waves, busy_waves, max_items, start_spread, n[0], n[0] ? t[0] / 100.0 / n[0] : 0.0, n[1],
            n[1] ? t[1] / 100.0 / n[1] : 0.0, n[2], n[2] ? t[2] / 100.0 / n[2] : 0.0, n[3], first_item, last_item, last_exit,
            line.c_str());
    fprintf(stderr, "ndt_hip:    per item: looking for work %.1f us (all kinds); node + shadow items: loading the rays %.1f us; trace_kd: node "
                    "batches %.1f us, shadow batches %.1f us; colours up the tree + counters %.1f us (node and lighting batches)\n",
            (n[0] + n[1] + n[2]) ? parts[0] / 100.0 / (n[0] + n[1] + n[2]) : 0.0,
            (n[0] + n[1]) ? parts[1] / 100.0 / (n[0] + n[1]) : 0.0, n[0] ? (parts[2] - parts[3]) / 100.0 / n[0] : 0.0,
            n[1] ? parts[3] / 100.0 / n[1] : 0.0, (n[0] + n[2]) ? parts[4] / 100.0 / (n[0] + n[2]) : 0.0);
}

// NDT_HIP_SHADE_PROBE=<k>: the lives of the wavefronts of the frame's k-th shade launch, of which the first `finish_waves`
// did the lighting part (shade_finish) and the rest the shading part behind it (shade_emit; pair launches)
void ndt_impl::print_shade_probe(const unsigned int *shade_log, int shade_probe, long long finish_waves)
{
    std::vector<unsigned int> log((size_t)2 * NDT_SHADE_LOG_WAVES);
    if (hipMemcpy(log.data(), shade_log, log.size() * sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned int t0 = 0;
    bool any = false;
    for (int w = 0; w < NDT_SHADE_LOG_WAVES; ++w)
        if (log[2 * w + 1] && (!any || (int)(log[2 * w] - t0) < 0)) {
            t0 = log[2 * w];
            any = true;
        }
    for (int part = 0; part < 2; ++part) {
        // part 0: lighting (shade_finish) wavefronts, part 1: shading (shade_emit) wavefronts
        int hist[48] = { 0 }, n_w = 0;
        double sum = 0, longest = 0, last_start = 0, last_end = 0;
        for (long long w = 0; w < NDT_SHADE_LOG_WAVES; ++w) {
            const bool lighting = w < finish_waves;
            if (!log[2 * w + 1] || lighting != (part == 0)) continue;
            const double st_us = (log[2 * w] - t0) / 100.0, dur = (log[2 * w + 1] - log[2 * w]) / 100.0;
            ++n_w;
            sum += dur;
            if (dur > longest) longest = dur;
            if (st_us > last_start) last_start = st_us;
            if (st_us + dur > last_end) last_end = st_us + dur;
            const int bin = (int)(dur / 4.0);
            ++hist[bin > 47 ? 47 : bin];
        }
        if (!n_w) continue;
        std::string line;
        for (int bin = 0; bin < 48; ++bin)
            if (hist[bin]) {
                char buf[48];
                snprintf(buf, sizeof buf, " %d-%d:%d", bin * 4, bin * 4 + 4, hist[bin]);
                line += buf;
            }
        fprintf(stderr, "ndt_hip: shade launch %d, %s: %d wavefronts, mean life %.1f us, longest %.1f us, last start at %.1f us, last end at %.1f us; lives per 4 us:%s\n",
                shade_probe, part == 0 ? "lighting" : "shading", n_w, sum / n_w, longest, last_start, last_end, line.c_str());
    }
}

// NDT_HIP_EXIT_PROBE: the life of every wavefront of one trace launch -- when the queue runs dry (first exit), how long the
// rest keeps going, and how much of that is the last wavefront's last batch.  q: the launch's NDT_EXIT_LOG_WORDS words.
static void print_exit_probe_launch(const unsigned int *q, int l)
{
    unsigned int t0 = 0;
    int n_w = 0;
    for (int w = 0; w < NDT_EXIT_LOG_WORDS / 8; ++w)
        if (q[8 * w + 2]) {
            if (!n_w || (int)(q[8 * w] - t0) < 0) t0 = q[8 * w];
            ++n_w;
        }
    int hist[64] = { 0 };
    double first = 1e30, last = 0, last_batch = 0, start_spread = 0;
    int simd_of_wave[16][4] = { { 0 } };        // workgroup wavefront w -> SIMD it ran on
    int wpw = 12;                               // wavefronts per workgroup of this launch (logged by the kernel)
    for (int w = 0; w < NDT_EXIT_LOG_WORDS / 8; ++w)
        if (q[8 * w + 2]) {
            // "out of work" = out of batches
            const double st_us = (q[8 * w] - t0) / 100.0, ex_us = (q[8 * w + 4] - t0) / 100.0;
            wpw = (int)(q[8 * w + 3] >> 24) > 0 && (q[8 * w + 3] >> 24) <= 16 ? (int)(q[8 * w + 3] >> 24) : wpw;
            ++simd_of_wave[w % wpw][(q[8 * w + 3] >> 4) & 3];
            if (st_us > start_spread) start_spread = st_us;
            if (ex_us < first) first = ex_us;
            if (ex_us > last) {
                last = ex_us;
                last_batch = (q[8 * w + 4] - q[8 * w + 1]) / 100.0;
            }
            const int bin = (int)(ex_us / 16.0);
            ++hist[bin > 63 ? 63 : bin];
        }
    std::string line;
    for (int bin = 0; bin < 64; ++bin)
        if (hist[bin]) {
            char buf[48];
            snprintf(buf, sizeof buf, " %d-%d:%d", bin * 16, bin * 16 + 16, hist[bin]);
            line += buf;
        }
    if (l == 0) {
        std::string m;
        for (int w = 0; w < wpw; ++w) {
            char buf[64];
            snprintf(buf, sizeof buf, " w%d:%d/%d/%d/%d", w, simd_of_wave[w][0], simd_of_wave[w][1], simd_of_wave[w][2], simd_of_wave[w][3]);
            m += buf;
        }
        fprintf(stderr, "ndt_hip: SIMD 0/1/2/3 of the workgroup's wavefronts (%d per workgroup):%s\n", wpw, m.c_str());
    }
    fprintf(stderr, "ndt_hip: trace launch %d: %d wavefronts start within %.1f us; first out of work at %.1f us, last at %.1f us (its last batch: %.1f us); exits per 16 us:%s\n",
            l, n_w, start_spread, first, last, last_batch, line.c_str());
}

void ndt_impl::print_exit_probe(const unsigned int *exit_log, int launches)
{
    std::vector<unsigned int> log((size_t)NDT_EXIT_LOG_LAUNCHES * NDT_EXIT_LOG_WORDS);
    if (hipMemcpy(log.data(), exit_log, log.size() * sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int l = 0; l < NDT_EXIT_LOG_LAUNCHES && l < launches; ++l) print_exit_probe_launch(log.data() + (size_t)l * NDT_EXIT_LOG_WORDS, l);
}

// NDT_PHASE_TIMING builds only (make -C ndt_amd/csrc timing): the accumulators of Workspace::dbg; other builds leave d[4] zero
void ndt_impl::print_phase_timing(const unsigned long long *dbg)
{
    unsigned long long d[160];
    if (hipMemcpy(d, dbg, sizeof(d), hipMemcpyDeviceToHost) != hipSuccess || !d[4]) return;
    fprintf(stderr, "ndt_hip: wave cycles T %llu G %llu I %llu list-end %llu prologue %llu outside %llu over %llu waves\n", d[0], d[1], d[2], d[3], d[5], d[6], d[4]);
    if (d[7] || d[32])
        fprintf(stderr, "ndt_hip:    coherent leaf scan: fetching windows %llu, boxes / gates of the windows %llu (its intersections are in I)\n", d[32], d[7]);
    fprintf(stderr, "ndt_hip: per-ray counts over %llu rays: node visits %llu, face gates %llu (pass %llu), item gates %llu (pass %llu), isect hits %llu\n",
            d[14], d[8], d[9], d[10], d[11], d[12], d[13]);
    if (d[60])
        fprintf(stderr, "ndt_hip: traversal stack over %llu rays: pops %llu, of them dropped at once %llu; T iterations with a pop in them %llu (of %llu)\n",
                d[14], d[60], d[61], d[62], d[16] + d[24]);
    fprintf(stderr, "ndt_hip: batch time inside trace_kd (100 MHz wall clock): closest max %.1f us mean %.1f us, shadow max %.1f us mean %.1f us\n",
            d[40] / 100.0, d[44] ? d[42] / 100.0 / d[44] : 0.0, d[41] / 100.0, d[45] ? d[43] / 100.0 / d[45] : 0.0);
    fprintf(stderr, "ndt_hip: per-ray maxima: %llu node visits, %llu gates, %llu intersections; per-batch maxima: %llu T, %llu G, %llu I iterations\n",
            d[46], d[47], d[48], d[49], d[50], d[51]);
    if (d[58])
        fprintf(stderr, "ndt_hip: shade_emit per wavefront (wall-clock ticks, mean over %llu): load+isect %.0f, light tests %.0f, segment reserve %.0f, shadow stores %.0f, spawn %.0f; slowest wavefront %llu\n",
                d[58], (double)d[52] / d[58], (double)d[53] / d[58], (double)d[54] / d[58], (double)d[55] / d[58], (double)d[56] / d[58], d[59]);
    for (int kind = 0; kind < 2; ++kind) {
        const unsigned long long *q = d + 16 + 8 * kind;
        fprintf(stderr, "ndt_hip: loop occupancy (%s rays): T %.1f%% of %llu iters, G %.1f%% of %llu, I %.1f%% of %llu\n",
                kind ? "shadow" : "closest", q[0] ? 100.0 * q[1] / (64.0 * q[0]) : 0.0, q[0],
                q[2] ? 100.0 * q[3] / (64.0 * q[2]) : 0.0, q[2], q[4] ? 100.0 * q[5] / (64.0 * q[4]) : 0.0, q[4]);
        if (q[4])
            fprintf(stderr, "ndt_hip:    I iterations execute %.2f primitive types on average; the commonest type holds %.1f of %.1f active lanes\n",
                    (double)q[6] / q[4], (double)q[7] / q[4], (double)q[5] / q[4]);
    }
}
