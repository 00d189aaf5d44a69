// ndt_frame.hip -- the device workspace and ONE pass of the ray pipeline over a set of primaries: primary rays, the
// bounce loop, bottom-up resolve, per-primary colour.  render_image (ndt.c:900) for the deterministic path is one
// such pass; recursive anti-aliasing and the sampled paths call it once per level / round.
#include "ndt_ctx.hpp"
#include "ndt_finish.hpp"
#include "ndt_shading.hpp"
#include <stddef.h>

static void free_stream_args(ndt_hip_ctx *ctx)
{
    for (void *p : ctx->sa_allocs) (void)hipFree(p);
    ctx->sa_allocs.clear();
    memset(&ctx->sa, 0, sizeof(ctx->sa));
    ctx->sa_cap = ctx->sa_sh_cap = 0;
    ctx->sa_nseg = 0;
}

hipError_t ndt_impl::sync_streams(ndt_hip_ctx *ctx)
{
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || !ctx->light_stream) return e;
    return hipStreamSynchronize(ctx->light_stream);
}

void ndt_impl::free_workspace(ndt_hip_ctx *ctx)
{
    for (void *p : ctx->ws_allocs) (void)hipFree(p);
    ctx->ws_allocs.clear();
    free_stream_args(ctx);
    memset(&ctx->ws, 0, sizeof(ctx->ws));
    ctx->ws_slab_words = 0;
    ctx->ws_dims = 0;
    ctx->ws_nseg = 0;
}

// ------------------------------------------------------------------ workspace

template <typename T> static int ws_alloc(ndt_hip_ctx *ctx, T **p, size_t count, bool stream_args = false)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, (count > 0 ? count : 1) * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(NDT_E_NOMEM, "hipMalloc of %zu bytes: %s", count * sizeof(T), hipGetErrorString(e));
    }
    (stream_args ? ctx->sa_allocs : ctx->ws_allocs).push_back(q);
    *p = (T *)q;
    return NDT_OK;
}

int ndt_impl::ensure_workspace(ndt_hip_ctx *ctx, long long cap, long long sh_cap)
{
    Workspace &ws = ctx->ws;
    const bool need_slab = ctx->tier == 1;
    const long long slab_lanes = 2048LL * NDT_TRACE_BLOCK;
    const long long slab_words = need_slab ? slab_lanes * ctx->sd.mask_words : 0;
    if (ws.cap >= cap && ws.sh_cap >= sh_cap && ctx->ws_dims == ctx->dims && ctx->ws_slab_words >= slab_words &&
        ctx->ws_nseg >= ctx->n_shadow_lights)
        return NDT_OK;
    if (cap < ws.cap) cap = ws.cap;
    if (sh_cap < ws.sh_cap) sh_cap = ws.sh_cap;
    cap = (cap + 63) & ~63LL;           // vectors are stored in tiles of 64 slots (load_soa / store_soa)
    sh_cap = (sh_cap + 63) & ~63LL;
    HIP_TRY(sync_streams(ctx));
    free_workspace(ctx);
    const int n = ctx->dims;
    int rc;
    // (an allocation that fails leaves no half-built workspace behind: the next call starts from nothing)
    auto give_up = [&](int code) {
        free_workspace(ctx);
        return code;
    };
    ws.cap = cap;
    ws.sh_cap = sh_cap;
    if ((rc = ws_alloc(ctx, &ws.ray_o, (size_t)n * cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.ray_v, (size_t)n * cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.frac, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.depth, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.rng_key, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.depth_left, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.hit_obj, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.hit_prim, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.hit_p, (size_t)n * cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.hit_n, (size_t)n * cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.clr, (size_t)3 * cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.child_refl, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.child_refr, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.sh_idx, (size_t)cap * (ctx->n_shadow_lights > 0 ? ctx->n_shadow_lights : 1)))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.sh_mask, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.count, (size_t)cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.so, (size_t)n * sh_cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.sv, (size_t)n * sh_cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.slim, (size_t)sh_cap))) return give_up(rc);
    // (three banks of the answers, taken in turn by the bounces: Workspace::sobj)
    if ((rc = ws_alloc(ctx, &ws.sobj, (size_t)3 * sh_cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.sprim, (size_t)3 * sh_cap))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.counters, NDT_CNT_ALLOC))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.ref_rays, 64 * 8))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.dbg, 160))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.exit_log, (size_t)NDT_EXIT_LOG_LAUNCHES * NDT_EXIT_LOG_WORDS))) return give_up(rc);
    if (ctx->shade_probe >= 0 && (rc = ws_alloc(ctx, &ws.shade_log, (size_t)2 * NDT_SHADE_LOG_WAVES))) return give_up(rc);
    if ((rc = ws_alloc(ctx, &ws.levels, NDT_MAX_LEVELS + 1))) return give_up(rc);
    ws.mask_slab_lanes = slab_lanes;
    if (need_slab) {
        if ((rc = ws_alloc(ctx, &ws.mask_slab, (size_t)slab_words))) return give_up(rc);
    }
    ctx->ws_slab_words = slab_words;
    ctx->ws_dims = ctx->dims;
    ctx->ws_nseg = ctx->n_shadow_lights > 0 ? ctx->n_shadow_lights : 1;
    return NDT_OK;
}

// The queues and counters of the streaming frame kernel for the current workspace: one fill counter, one lighting
// counter and one ring entry per node batch, the same per shadow batch of every light's segment, a parent and a
// wait count per node, an owner per shadow slot.  (They belong to a workspace and a light count: free_workspace releases
// them, and so does a change of either -- the previous set is freed, not kept until the workspace goes.)
static int ensure_stream_args(ndt_hip_ctx *ctx)
{
    const Workspace &ws = ctx->ws;
    const int n_seg = ctx->n_shadow_lights > 0 ? ctx->n_shadow_lights : 1;
    if (ctx->sa.ctl && ctx->sa_cap == ws.cap && ctx->sa_sh_cap == ws.sh_cap && ctx->sa_nseg == n_seg) return NDT_OK;
    if (!ctx->sa_allocs.empty()) {
        HIP_TRY(sync_streams(ctx));
        free_stream_args(ctx);
    }
    StreamArgs &sa = ctx->sa;
    // rings have room for a ticket per wavefront beyond the last entry (a wavefront's ticket may name a slot that is never written)
    const long long margin = NDT_STREAM_LOG_WAVES;
    const long long node_batches = ws.cap / 64 + margin;
    const long long seg_cap = (ws.sh_cap / n_seg) & ~63LL;
    const long long sh_batches = (long long)n_seg * (seg_cap / 64) + margin;
    int rc;
    if ((rc = ws_alloc(ctx, &sa.ctl, 1, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.node_fill, (size_t)node_batches, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.sh_pending, (size_t)node_batches, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.sh_fill, (size_t)sh_batches, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.sec_ring, (size_t)NDT_PRIM_SHARDS * node_batches, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.sh_ring, (size_t)sh_batches, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.fin_ring, (size_t)node_batches, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.parent, (size_t)ws.cap, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.pend, (size_t)ws.cap, true))) return rc;
    if ((rc = ws_alloc(ctx, &sa.sowner, (size_t)n_seg * seg_cap, true))) return rc;
    if (ctx->stream_probe && (rc = ws_alloc(ctx, &sa.wave_log, (size_t)24 * NDT_STREAM_LOG_WAVES, true))) return rc;
    sa.n_seg = n_seg;
    sa.seg_cap = (int)seg_cap;
    sa.node_batches = (int)node_batches;
    ctx->sa_cap = ws.cap;
    ctx->sa_sh_cap = ws.sh_cap;
    ctx->sa_nseg = n_seg;
    return NDT_OK;
}

// ------------------------------------------------------------------ dimension-independent kernels

// Everything a frame needs reset, in one launch (five small copies / fills of 10 us each before): node tail and
// overflow flags, the work-queue heads of the launches the frame can have, both parities of the shadow-segment
// counters, the reference-ray partial sums, the diagnostic words, and the primaries' range.
__global__ void k_frame_init(Workspace ws, int n_primary, LevelRange level0, int queue_ints)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int k = i; k < queue_ints; k += stride) ws.counters[NDT_CNT_QUEUE + k] = 0;
    for (int k = i; k < NDT_CNT_TOTAL - NDT_CNT_SEG; k += stride) ws.counters[NDT_CNT_SEG + k] = 0;
    for (int k = i; k < 64 * 8; k += stride) ws.ref_rays[k] = 0ull;
    for (int k = i; k < 160; k += stride) ws.dbg[k] = 0ull;
    if (i < 4) ws.counters[i] = (i == 0) ? n_primary : 0;
    if (i == 0) ws.levels[0] = level0;
}

// The frame's closing record, written to host-visible memory by the last kernel of the frame: the host polls its
// tag instead of queueing three small read-backs and synchronising the stream.  One wavefront.
//   [0] node tail  [1] overflow flags  [2] shadow slots wanted  [3] shadow rays of the frame  [4] bounces with nodes
//   [5] rays the reference would have traced  [7] tag
__global__ void k_frame_done(Workspace ws, int n_run, unsigned long long *done, unsigned long long tag)
{
    const int lane = threadIdx.x;
    unsigned long long ref = ws.ref_rays[8 * lane];         // 64 partial sums, one 64-byte line each
    for (int d = 32; d > 0; d >>= 1) ref += __shfl_xor(ref, d, 64);
    if (lane != 0) return;
    long long shadow = 0;
    int used = 0;
    for (int b = 0; b < n_run; ++b) {
        if (ws.levels[b].count <= 0) break;
        shadow += ws.levels[b].n_shadow;
        ++used;
    }
    done[0] = (unsigned long long)(long long)ws.counters[0];
    done[1] = (unsigned long long)(long long)ws.counters[2];
    done[2] = (unsigned long long)(long long)ws.counters[3];
    done[3] = (unsigned long long)shadow;
    done[4] = (unsigned long long)used;
    done[5] = ref;
    __threadfence_system();
    __hip_atomic_store(&done[7], tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The streaming pipeline's frame reset: control block, fill / lighting counters and rings of the batches the frame can
// have, the frame's own accumulators.  (Sized by the pool, not by the frame: a few MB of zeros.)
__global__ void __launch_bounds__(256) k_stream_init(Workspace ws, StreamArgs sa, long long node_batches, long long sh_batches)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    // the control block: zeros, except the node tail (the pool behind the primaries is free) and the primaries' share of
    // every shard's outstanding count -- written by the thread that owns the word, so that no zero can land on top of it
    int *ctl = reinterpret_cast<int *>(sa.ctl);
    const int nb0 = sa.root_begin >> 6, nb1 = nb0 + (sa.n_primary >> 6);       // the root batches
    for (long long k = i; k < (long long)(sizeof(StreamCtl) / sizeof(int)); k += stride) {
        int v = 0;
        if (k == (long long)(offsetof(StreamCtl, node_tail) / sizeof(int))) v = sa.root_begin + sa.n_primary;
        for (int sh = 0; sh < NDT_PRIM_SHARDS; ++sh)
            if (k == (long long)((offsetof(StreamCtl, outstanding) + sh * sizeof(StreamWord)) / sizeof(int))) {
                // root batches nb in [nb0, nb1) with nb % 8 == sh
                const int first = nb0 + ((sh - nb0 % NDT_PRIM_SHARDS) + NDT_PRIM_SHARDS) % NDT_PRIM_SHARDS;
                v = first < nb1 ? 128 * ((nb1 - 1 - first) / NDT_PRIM_SHARDS + 1) : 0;
            }
        ctl[k] = v;
    }
    for (long long k = i; k < node_batches; k += stride) {
        sa.node_fill[k] = 0;
        sa.sh_pending[k] = 0;
        for (int sh = 0; sh < NDT_PRIM_SHARDS; ++sh) sa.sec_ring[(long long)sh * node_batches + k] = 0;
        sa.fin_ring[k] = 0;
    }
    for (long long k = i; k < sh_batches; k += stride) {
        sa.sh_fill[k] = 0;
        sa.sh_ring[k] = 0;
    }
    for (long long k = i; k < 64 * 8; k += stride) ws.ref_rays[k] = 0ull;
    for (long long k = i; k < 4; k += stride) ws.counters[k] = 0;
}

// The streaming pipeline's closing record, in host-visible memory (the host polls the tag):
//   [0] node tail  [1] overflow flags  [2] abort  [3] shadow rays  [4] deepest bounce + 1  [5] reference-equivalent rays
//   [6] children  [7] tag
__global__ void k_stream_done(Workspace ws, StreamArgs sa, unsigned long long *done, unsigned long long tag)
{
    const int lane = threadIdx.x;
    unsigned long long ref = ws.ref_rays[8 * lane];
    for (int d = 32; d > 0; d >>= 1) ref += __shfl_xor(ref, d, 64);
    if (lane != 0) return;
    const StreamCtl *c = sa.ctl;
    done[0] = (unsigned long long)(long long)c->node_tail.v;
    done[1] = (unsigned long long)(long long)c->overflow.v;
    done[2] = (unsigned long long)(long long)(c->abort.v | (c->timeout_where.v << 8));
    done[3] = (unsigned long long)(long long)c->n_shadow.v;
    done[4] = (unsigned long long)(long long)(c->max_level.v + 1);
    done[5] = ref;
    done[6] = (unsigned long long)(long long)c->n_children.v;
    __threadfence_system();
    __hip_atomic_store(&done[7], tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Bottom-up combine of one bounce: get_ray_color's blend of its own colour with the colours
// its reflection / refraction children returned (blend_children, ndt_shading.hpp), with plain accesses.
__device__ __forceinline__ void resolve_node(const double *blob, const SceneDesc &sd, const Workspace &ws, int specular, long long g)
{
    if (ws.depth_left[g] <= 0) return;
    const int obj = ws.hit_obj[g];
    if (obj < 0) return;                        // background node: colour and count already final
    const Surface sf = surface_of(blob, sd, obj, specular);
    double c[3] = { ws.clr[0 * ws.cap + g], ws.clr[1 * ws.cap + g], ws.clr[2 * ws.cap + g] };
    int cnt = ws.count[g];
    const int child[2] = { ws.child_refl[g], ws.child_refr[g] };
    double ref[2][3] = { { 0.0, 0.0, 0.0 }, { 0.0, 0.0, 0.0 } };        // (a child that was cut off, -2: black)
    for (int j = 0; j < 2; ++j) {
        if (child[j] >= 0) {
            for (int k = 0; k < 3; ++k) ref[j][k] = ws.clr[k * ws.cap + child[j]];
            cnt += ws.count[child[j]];
        }
    }
    blend_children(c, sf.refl, specular, child[0] != -1, ref[0], child[1] != -1, ref[1]);
    ws.clr[0 * ws.cap + g] = c[0];
    ws.clr[1 * ws.cap + g] = c[1];
    ws.clr[2 * ws.cap + g] = c[2];
    ws.count[g] = cnt;
}

__global__ void __launch_bounds__(256) k_resolve(const double *blob, SceneDesc sd, Workspace ws, int specular, int level)
{
    const LevelRange lr = ws.levels[level];
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < lr.count; r += (long long)gridDim.x * blockDim.x)
        resolve_node(blob, sd, ws, specular, lr.begin + r);
}

// (the pixel itself: ndt_finish.hpp)
// resolve0: the bottom-up combine of the primaries' own bounce (the last k_resolve) happens here, in the thread that then
// finishes the pixel: one launch less at the end of a frame
#ifndef NDT_FINISH_BLOCK
#define NDT_FINISH_BLOCK 256
#endif
// What a finish launch adds to the frame's reference-equivalent ray count (every thread of the workgroup calls this): wavefront
// sum, then one atomic per wavefront spread over 64 cache lines (a single word saturates near 90 atomics/us, and there are 32k
// wavefronts at 1080p)
__device__ __forceinline__ void add_ref_rays(const Workspace &ws, unsigned long long weighted)
{
    for (int d = 32; d > 0; d >>= 1) weighted += __shfl_down(weighted, d, 64);
    if ((threadIdx.x & 63) == 0 && weighted) atomicAdd(ws.ref_rays + 8 * ((blockIdx.x * (NDT_FINISH_BLOCK / 64) + (threadIdx.x >> 6)) & 63), weighted);
}

__global__ void __launch_bounds__(NDT_FINISH_BLOCK) k_finish_pixels(const double *blob, SceneDesc sd, Workspace ws, RenderGeom rg, int N_,
                                                       double *rgba, double *depth_out, int resolve0)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long weighted = 0ull;
    if (resolve0 && g < rg.n_primary) resolve_node(blob, sd, ws, rg.specular, g);
    if (g < rg.n_primary && ws.depth_left[g] > 0) weighted = finish_pixel<false>(blob, sd, ws, rg, N_, g, rgba, depth_out);
    add_ref_rays(ws, weighted);
}

// early_pixels: the pixels of the parts in `take` (bit p: part p of pixel_part) and no others.  Launched early for part 1 or 2
// on the light stream, and as the frame's final launch for the parts no early launch took; a frame without early launches keeps
// k_finish_pixels above.  A pixel that is not taken is left alone -- resolve_node is not idempotent -- after the two to four
// words pixel_part reads.  The sums of ref_rays are integers: whichever launch adds a pixel's share, the total is the same.
__global__ void __launch_bounds__(NDT_FINISH_BLOCK) k_finish_part(const double *blob, SceneDesc sd, Workspace ws, RenderGeom rg, int N_,
                                                     double *rgba, double *depth_out, int resolve0, int take)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long weighted = 0ull;
    if (g < rg.n_primary && ((take >> pixel_part(ws, g)) & 1)) {
        if (resolve0) resolve_node(blob, sd, ws, rg.specular, g);
        if (ws.depth_left[g] > 0) weighted = finish_pixel<false>(blob, sd, ws, rg, N_, g, rgba, depth_out);
    }
    add_ref_rays(ws, weighted);
}

// max_optic_depth <= 0: get_ray_color returns black without tracing (ndt.c:340)
__global__ void k_fill_black(double *rgba, long long n_pixels)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    rgba[4 * i + 0] = 0.0; rgba[4 * i + 1] = 0.0; rgba[4 * i + 2] = 0.0; rgba[4 * i + 3] = 1.0;
}

// pixel_d2c, image.h:36-39
void ndt_impl::launch_fill_black(hipStream_t s, double *rgba, long long n_pixels)
{
    hipLaunchKernelGGL(k_fill_black, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, rgba, n_pixels);
}

void ndt_impl::add_stats(ndt_render_stats &acc, const ndt_render_stats &st)
{
    acc.rays_primary += st.rays_primary;
    acc.rays_secondary += st.rays_secondary;
    acc.rays_shadow += st.rays_shadow;
    acc.rays_ref_equiv += st.rays_ref_equiv;
    if (st.levels > acc.levels) acc.levels = st.levels;
    acc.trace_launches += st.trace_launches;
    acc.trace_ms += st.trace_ms;
    acc.frame_ms += st.frame_ms;
    if (st.node_capacity > acc.node_capacity) acc.node_capacity = st.node_capacity;
}

// ------------------------------------------------------------------ render

static hipEvent_t get_event(ndt_hip_ctx *ctx, size_t idx)
{
    while (ctx->ev_pool.size() <= idx) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        ctx->ev_pool.push_back(ev);
    }
    return ctx->ev_pool[idx];
}

static double wall_s()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// The host waits for a kernel of the running frame by polling a word of host-mapped memory for the frame's tag: no stream
// synchronisation, no read-back.  After 30 s without it the stream is synchronised and the word looked at once more; `what`
// (a format that may take `bounce`) is the error if it still is not there.
static int wait_for_tag(ndt_hip_ctx *ctx, const unsigned long long *word, unsigned long long tag, const char *what, int bounce = 0)
{
    const double t_wait = wall_s();
    while (__atomic_load_n(word, __ATOMIC_ACQUIRE) != tag) {
        if (wall_s() - t_wait > 30.0) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) != tag) return fail(NDT_E_STATE, what, bounce);
        }
    }
    return NDT_OK;
}

// The primaries a pass traces: one a sample, or one a pixel -- but none for the 46 blank lines between the eyes of a frame-packed
// image (primary_node makes no ray there, ndt.c:614-631)
static long long n_pixels(const RenderGeom &rg)
{
    if (rg.samples) return (long long)rg.n_samples;
    long long rows = rg.rows;
    if (rg.stereo == 4)
        for (int r = 0; r < rg.rows; ++r) {
            const int j = rg.row_pair ? rg.row_begin + (r >> 1) * rg.row_step + (r & 1) : rg.row_begin + r * rg.row_step;
            if (j >= 1080 && j <= 1080 + 45) rows -= 1;
        }
    return rows * rg.width;
}

// A profiled pass takes the frame's begin / end from the dispatch timestamps of its first and last kernel
template <typename Kernel, typename... Args>
static void launch_stamped(Kernel k, dim3 grid, dim3 block, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, Args... args)
{
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(k, grid, block, 0, s, ev_start, ev_stop, 0u, args...);
    else
        hipLaunchKernelGGL(k, grid, block, 0, s, args...);
}

static void launch_finish_pixels(ndt_hip_ctx *ctx, const SceneDesc &sd_pass, const Workspace &ws, const RenderGeom &rg, void *d_rgba, void *d_depth,
                                 int resolve0)
{
    hipLaunchKernelGGL(k_finish_pixels, dim3((unsigned)((rg.n_primary + NDT_FINISH_BLOCK - 1) / NDT_FINISH_BLOCK)), dim3(NDT_FINISH_BLOCK), 0, ctx->stream,
                       ctx->d_blob.as<double>(), sd_pass, ws, rg, ctx->dims, (double *)d_rgba, (double *)d_depth, resolve0);
}

// early_pixels: the parts in `take` only, on stream `on`
static void launch_finish_part(ndt_hip_ctx *ctx, hipStream_t on, const SceneDesc &sd_pass, const Workspace &ws, const RenderGeom &rg, void *d_rgba,
                               void *d_depth, int resolve0, int take)
{
    hipLaunchKernelGGL(k_finish_part, dim3((unsigned)((rg.n_primary + NDT_FINISH_BLOCK - 1) / NDT_FINISH_BLOCK)), dim3(NDT_FINISH_BLOCK), 0, on,
                       ctx->d_blob.as<double>(), sd_pass, ws, rg, ctx->dims, (double *)d_rgba, (double *)d_depth, resolve0, take);
}

// The frame kernel's arguments for a frame of `count` primaries: the roots of its forest, from slot 0, in batches of 64 (the last
// one padded)
static int stream_roots(ndt_hip_ctx *ctx, bool prof, long long count, StreamArgs &sa)
{
    sa = ctx->sa;
    sa.root_begin = 0;
    sa.n_primary = (int)((count + 63) & ~63LL);
    sa.valid_begin = 0;
    sa.valid_end = (int)count;
    sa.roots_are_primaries = 1;
    sa.fused = 0;
    if (!prof) sa.wave_log = nullptr;
    else if (sa.wave_log) HIP_TRY(hipMemsetAsync(sa.wave_log, 0, (size_t)24 * NDT_STREAM_LOG_WAVES * sizeof(unsigned int), ctx->stream));
    return NDT_OK;
}

static void launch_stream_init(ndt_hip_ctx *ctx, const Workspace &ws, const StreamArgs &sa, hipEvent_t ev_start)
{
    const long long sh_batches = (long long)sa.n_seg * (sa.seg_cap / 64) + NDT_STREAM_LOG_WAVES;
    launch_stamped(k_stream_init, dim3(512), dim3(256), ctx->stream, ev_start, nullptr, ws, sa, (long long)sa.node_batches, sh_batches);
}

// render_pass_levels and one attempt of it: the pools overflowed and have been grown, render the pass again (not an NDT_E_* code)
static const int PASS_AGAIN = 1;

// ---- the streaming pipeline: one persistent launch for the whole ray tree (ndt_stream.hpp).  no_room: the pools the frame
// kernel wants cannot be had (auto then renders the pass per bounce).
static int render_pass_stream(ndt_hip_ctx *ctx, const RenderGeom &rg, const SceneDesc &sd_pass, bool prof, void *d_rgba, void *d_depth, long long cap,
                              long long sh_cap, ndt_render_stats &st, bool &no_room)
{
    hipStream_t s = ctx->stream;
    const NdtKernelTable *kt = ctx->kt;
    const int n_seg = ctx->n_shadow_lights > 0 ? ctx->n_shadow_lights : 1;
    for (int attempt = 0; attempt < 8; ++attempt) {
        // every light's shadow segment can hold one ray per node
        if (sh_cap < cap * n_seg) sh_cap = cap * n_seg;
        int rc = NDT_OK;
        if (cap > 0x7fffff00LL || sh_cap > 0x7fffff00LL) rc = fail(NDT_E_NOMEM, "ray tree exceeds 2^31 nodes");
        if (!rc) rc = ensure_workspace(ctx, cap, sh_cap);
        if (!rc) rc = ensure_stream_args(ctx);
        no_room = rc == NDT_E_NOMEM;
        if (rc) return rc;
        const Workspace ws = ctx->ws;
        StreamArgs sa;
        if ((rc = stream_roots(ctx, prof, rg.n_primary, sa))) return rc;
        // the kernel makes its own primaries and writes its own pixels (option stream_fused, on by default)
        sa.fused = ctx->stream_fused ? 1 : 0;
        sa.rgba = (double *)d_rgba;
        sa.depth_out = (double *)d_depth;
        hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
        if (prof) {
            ev_begin = get_event(ctx, 0);
            ev_end = get_event(ctx, 1);
            ev_k0 = get_event(ctx, 2);
            ev_k1 = get_event(ctx, 3);
        }
        const unsigned long long tag = ++ctx->frame_tag;
        launch_stream_init(ctx, ws, sa, ev_begin);
        if (!sa.fused) kt->primary(s, ctx->d_blob.as<double>(), sd_pass, ws, rg);
        kt->frame_stream(s, ctx->d_blob.as<double>(), sd_pass, ws, rg, sa, ctx->tier, ctx->sd.mask_words, ev_k0, ev_k1);
        if (!sa.fused) launch_finish_pixels(ctx, sd_pass, ws, rg, d_rgba, d_depth, 0);
        launch_stamped(k_stream_done, dim3(1), dim3(64), s, nullptr, ev_end, ws, sa, ctx->d_done, tag);
        HIP_TRY(hipGetLastError());
        if ((rc = wait_for_tag(ctx, &ctx->h_done[7], tag, "the frame never completed"))) return rc;
        if (prof) HIP_TRY(hipEventSynchronize(ev_end));
        const int overflow = (int)(long long)ctx->h_done[1], aborted = (int)(long long)ctx->h_done[2];
        if (overflow != 0) {
            if (overflow & 1) cap *= 2;
            if (overflow & 2) sh_cap *= 2;
            continue;
        }
        if (aborted != 0)
            return fail(NDT_E_STATE, "the frame kernel gave up (abort %d, where %d): a work item never arrived", aborted & 0xff, aborted >> 8);
        st = ndt_render_stats{};
        st.rays_primary = n_pixels(rg);
        st.rays_secondary = (long long)ctx->h_done[6];
        st.rays_shadow = (long long)ctx->h_done[3];
        st.rays_ref_equiv = (long long)ctx->h_done[5];
        st.levels = (int)ctx->h_done[4];
        st.trace_launches = 1;
        st.node_capacity = ws.cap;
        if (prof) {
            float km = 0, fm = 0;
            HIP_TRY(hipEventElapsedTime(&km, ev_k0, ev_k1));
            HIP_TRY(hipEventElapsedTime(&fm, ev_begin, ev_end));
            st.trace_ms = km;
            st.frame_ms = fm;
            if (sa.wave_log) print_stream_probe(sa.wave_log, km);
        }
        return NDT_OK;
    }
    return fail(NDT_E_NOMEM, "ray-tree workspace kept overflowing");
}

// ---- the per-bounce pipeline.  One attempt at the pass -- a frame in flight: what the pass is, and what the launches of the
// attempt share.  The stream is never synchronised inside a frame: the range of every bounce is published on the device (by
// the prologue of the trace launch behind its shading, TraceJob::publish_level) and read there; the host only learns, from
// the mailbox, whether there is a next bounce to enqueue.  Bounce 0 = the primaries.
struct FrameInFlight {
    ndt_hip_ctx *ctx;
    const RenderGeom &rg;
    const SceneDesc &sd_pass;
    const bool prof;
    void *d_rgba, *d_depth;
    hipStream_t s;
    const NdtKernelTable *kt;
    Workspace ws;
    const int n_levels;             // a node spawns children only while depth_left > 1
    // light windows: window k's scene description, and how many window emits the frame has had (they take the two banks of
    // window counters in turn)
    const int n_win;
    const bool windowed;
    // Option light_overlap (one light window): the lighting of every bounce but the deepest runs on the light stream,
    // beside the trace launch of the NEXT bounce, which does not need it.  Nothing is put on the main stream
    // for it: shade_finish(b) is launched when the mailbox says that the stream has passed the trace launch of bounce b
    // (light_beside).  ev_lit[b % 3], on the light stream behind shade_finish(b), marks the last reader of bank b % 3 of the
    // shadow answers.
    const bool overlap;
    hipStream_t ls;
    hipEvent_t ev_lit[3] = { nullptr, nullptr, nullptr };
    int light_next = 0;                         // the first bounce whose lighting has not gone to the light stream
    hipEvent_t light_tail = nullptr;            // the light stream's last event, while the main stream has not waited for it
    // Option early_pixels (where `overlap` holds): the pixels of primaries that are final long before the end of the frame are
    // finished on the light stream -- part 1 (missed) beside trace launch 1, part 2 (hit, no child) behind shade_finish(0) --
    // and the frame's final launch takes the parts that were not launched in this attempt (early_pixels_beside)
    const int early;                            // 0 none, 1 part 1, 2 parts 1 and 2
    int early_done = 0;                         // bit p: part p was launched early in this attempt
    hipEvent_t ev_early = nullptr;              // on the light stream behind the launch of part 1
    std::vector<SceneDesc> sd_win;
    int win_emits = 0;
    unsigned long long tag = 0;
    int slots = 0, queue_slot = 0;  // work queues zeroed by frame init / handed out so far
    int launches = 0;               // trace launches
    size_t ev_n = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> trace_ev;
    std::vector<std::string> trace_dbg;
    // NDT_HIP_SHADE_PROBE=<k>: the k-th shade launch of the frame logs the life of each of its wavefronts
    int shade_launch = 0;
    long long shade_probe_finish_waves = 0;     // wavefronts of the lighting part of the probed launch
    int n_run;                                  // bounces enqueued (the per-bounce resolve walks them)
    std::vector<long long> level_nodes;         // node count of every bounce (an upper bound: sizes grids)
    int pending_finish = -1;                    // bounce whose lighting has not been launched yet
    long long pending_upper = 0;
    bool resolve_with_finish = false;           // the deepest bounce was blended by its lighting launch

    FrameInFlight(ndt_hip_ctx *c, const RenderGeom &g, const SceneDesc &sd, bool p, void *rgba, void *depth)
        : ctx(c), rg(g), sd_pass(sd), prof(p), d_rgba(rgba), d_depth(depth), s(c->stream), kt(c->kt), ws(c->ws),
          n_levels(g.max_depth > 1 ? g.max_depth : 1), n_win((int)c->windows.size()), windowed(n_win > 1),
          overlap(c->light_overlap && !windowed), ls(c->light_stream), early(overlap ? c->early_pixels : 0), n_run(n_levels)
    {
        ws.mail = ctx->d_mail;
        ws.mail_tag = ctx->d_mail_tag;
        for (int k = 0; windowed && k < n_win; ++k) sd_win.push_back(window_desc(ctx, sd_pass, k));
    }

    int render(long long &cap, long long &sh_cap, ndt_render_stats &st);
    int render_frame(long long &cap, long long &sh_cap, ndt_render_stats &st);
    int frame_init(long long &sh_cap);
    int traced(TraceJob &tj, const std::string &what, const SceneDesc *sd_job = nullptr);
    int answer_bank(int b) const { return overlap ? b % 3 : 0; }   // of sobj / sprim, for the shadow rays of bounce b
    Workspace shade_ws(long long finish_nodes, int b, hipStream_t on);
    int trace_primaries();
    void light_and_shade(int b, long long upper);
    int light_beside(int b);
    int early_pixels_beside(int part);
    int mark_light_tail(hipEvent_t ev);
    hipError_t join_light();
    int trace_bounce(int b, long long upper);
    int trace_windows(int b, long long upper);
    void light_last();
    void resolve();
    int close();
    int report(long long &cap, long long &sh_cap, ndt_render_stats &st);
    hipError_t print_debug(int levels_used);
};

// Every way out of a frame -- its image, PASS_AGAIN, an error -- leaves the main stream behind whatever the frame put on the light
// stream: the attempt that follows, or whoever synchronises the main stream before freeing the pools, is behind it too
int FrameInFlight::render(long long &cap, long long &sh_cap, ndt_render_stats &st)
{
    const int rc = render_frame(cap, sh_cap, st);
    const hipError_t e = join_light();          // (a frame that closed has joined already: light_tail is null)
    if (rc == NDT_OK && e != hipSuccess) return fail(NDT_E_DEVICE, "joining the light stream: %s", hipGetErrorString(e));
    return rc;
}

// the main stream waits (on the device) for the light stream's last launch
hipError_t FrameInFlight::join_light()
{
    if (!light_tail) return hipSuccess;
    const hipError_t e = hipStreamWaitEvent(s, light_tail, 0);
    light_tail = nullptr;
    return e;
}

// light_overlap: the lighting of bounce b on the light stream.  The caller has seen the mailbox tag of bounce b + 2: the prologue
// of trace launch b + 1 posted it, so the main stream has passed trace launch b -- the shadow answers of bounce b are complete, as
// is everything else shade_finish_node reads -- and the kernel needs no event to wait for: it starts at once,
// beside trace launch b + 1, and the main stream carries no marker for it.
int FrameInFlight::light_beside(int b)
{
    kt->shade_finish(ls, ctx->d_blob.as<double>(), sd_pass, shade_ws(level_nodes[b], b, ls), rg, b, level_nodes[b], 0);
    // (early_pixels 2: the primaries without a child are final now; their pixels go directly behind, ahead of the event)
    int rc;
    if (b == 0 && early >= 2 && (rc = early_pixels_beside(NDT_PART_CHILDLESS))) return rc;
    if ((rc = mark_light_tail(ev_lit[b % 3]))) return rc;
    light_next = b + 1;
    return NDT_OK;
}

// early_pixels: the pixels of one part of the primaries on the light stream, with nothing to wait for and no marker on the main
// stream.  Part 1: the caller has seen the mailbox tag of bounce 1, which the prologue of trace launch 1 posted -- the main stream
// has passed shade_emit(0), which wrote everything pixel_part and a missed primary's pixel read; the launch runs as trace launch 1
// drains, and its own event becomes the light stream's tail.  Part 2: the caller has just put shade_finish(0) on this stream and
// records the event behind both.  Either way the joins that order the main stream behind the lighting order it behind this.
int FrameInFlight::early_pixels_beside(int part)
{
    launch_finish_part(ctx, ls, sd_pass, ws, rg, d_rgba, d_depth, 0, 1 << part);
    early_done |= 1 << part;
    return part == NDT_PART_MISSED ? mark_light_tail(ev_early) : NDT_OK;
}

// `ev` behind whatever has just been put on the light stream: from now on the joins wait for it.  If the event cannot be
// recorded no join could cover those launches, so the host waits for the light stream here, before the error goes out
int FrameInFlight::mark_light_tail(hipEvent_t ev)
{
    const hipError_t e = hipEventRecord(ev, ls);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ls);
        return fail(NDT_E_DEVICE, "hipEventRecord on the light stream: %s", hipGetErrorString(e));
    }
    light_tail = ev;
    return NDT_OK;
}

int FrameInFlight::render_frame(long long &cap, long long &sh_cap, ndt_render_stats &st)
{
    int rc;
    if ((rc = frame_init(sh_cap))) return rc;
    if ((rc = trace_primaries())) return rc;
    long long upper = rg.n_primary;         // node count of the bounce
    for (int b = 0; b < n_levels; ++b) {
        // (the same bounce limit whatever the light windows: a windowed pass uses its work queues again, but light_window must
        // not change what renders)
        if ((windowed ? b + 2 : queue_slot + 1) > NDT_QUEUE_SLOTS || b + 1 > NDT_MAX_LEVELS)
            return fail(NDT_E_UNSUPPORTED, "more than %d bounces", NDT_QUEUE_SLOTS - 1);
        if (b > 0) {
            // published by the trace launch of bounce b - 1, which ran right after shade_emit(b - 1) -- and behind trace launch
            // b - 2: the lighting of bounce b - 2 can go (light_overlap)
            if ((rc = wait_for_tag(ctx, &ctx->h_mail_tag[b], tag, "bounce %d was never published", b))) return rc;
            upper = ctx->h_mail[b].count;
            if (early >= 1 && b == 1 && (rc = early_pixels_beside(NDT_PART_MISSED))) return rc;
            if (overlap && b >= 2 && (rc = light_beside(b - 2))) return rc;
            if (upper <= 0) {
                n_run = b;
                break;
            }
        }
        level_nodes.push_back(upper);
        light_and_shade(b, upper);
        if ((rc = trace_bounce(b, upper))) return rc;
        if (windowed && (rc = trace_windows(b, upper))) return rc;
        pending_finish = b;
        pending_upper = upper;
    }
    light_last();
    if (overlap && n_run >= 2 && light_next == n_run - 2) {
        // the bounce limit ended the loop: the last trace launch posts a bounce of its own, and with it where the stream is
        if ((rc = wait_for_tag(ctx, &ctx->h_mail_tag[n_run], tag, "bounce %d was never published", n_run))) return rc;
        if ((rc = light_beside(n_run - 2))) return rc;
    }
    HIP_TRY(join_light());                  // the resolve reads the colours every bounce's lighting left
    resolve();
    // (early_pixels: the parts that went to the light stream in this attempt are finished; the final launch takes the others)
    if (early_done) launch_finish_part(ctx, s, sd_pass, ws, rg, d_rgba, d_depth, n_run >= 1 ? 1 : 0, 7 & ~early_done);
    else launch_finish_pixels(ctx, sd_pass, ws, rg, d_rgba, d_depth, n_run >= 1 ? 1 : 0);
    if ((rc = close())) return rc;
    return report(cap, sh_cap, st);
}

// Everything the frame needs reset, and the primaries' range (k_frame_init).  PASS_AGAIN: the shadow queue cannot hold the
// primaries' segments.
int FrameInFlight::frame_init(long long &sh_cap)
{
    if (prof) {
        // frame time = start of the frame's first kernel .. end of its last (their own dispatch timestamps)
        ev_begin = get_event(ctx, ev_n++);
        ev_end = get_event(ctx, ev_n++);
    }
    for (int p = 0; overlap && p < 3; ++p)
        if (!(ev_lit[p] = get_event(ctx, ev_n++))) return fail(NDT_E_DEVICE, "hipEventCreate failed");
    if (early && !(ev_early = get_event(ctx, ev_n++))) return fail(NDT_E_DEVICE, "hipEventCreate failed");
    if (prof && ctx->exit_probe)
        HIP_TRY(hipMemsetAsync(ws.exit_log, 0, (size_t)NDT_EXIT_LOG_LAUNCHES * NDT_EXIT_LOG_WORDS * sizeof(unsigned int), s));
    tag = ++ctx->frame_tag;
    LevelRange level0;
    level0.begin = 0;
    level0.count = rg.n_primary;
    level0.seg_stride = (rg.n_primary + 63) & ~63LL;
    level0.n_shadow = 0;
    if ((long long)ctx->n_shadow_lights * level0.seg_stride > ws.sh_cap) {
        sh_cap = (long long)ctx->n_shadow_lights * level0.seg_stride;
        return PASS_AGAIN;
    }
    // one trace launch per bounce and light window + the primaries' own (more than NDT_QUEUE_SLOTS: see traced)
    const long long want_slots = (long long)n_levels * (windowed ? n_win : 1) + 2;
    slots = want_slots > NDT_QUEUE_SLOTS ? NDT_QUEUE_SLOTS : (int)want_slots;
    launch_stamped(k_frame_init, dim3(8), dim3(256), s, ev_begin, nullptr, ws, rg.n_primary, level0, slots * NDT_QUEUE_INTS);
    if (windowed) HIP_TRY(hipMemsetAsync(ws.counters + NDT_CNT_WIN, 0, (NDT_CNT_ALLOC - NDT_CNT_WIN) * sizeof(int), s));
    return NDT_OK;
}

// One trace launch of the frame, on the next work queue
int FrameInFlight::traced(TraceJob &tj, const std::string &what, const SceneDesc *sd_job)
{
    // (more trace launches than work queues -- light windows: a queue is used again once the stream has passed the launch
    // that used it before, zeroed on the stream first)
    tj.queue = ws.counters + NDT_CNT_QUEUE + (queue_slot % NDT_QUEUE_SLOTS) * NDT_QUEUE_INTS;
    if (queue_slot++ >= slots) HIP_TRY(hipMemsetAsync(tj.queue, 0, NDT_QUEUE_INTS * sizeof(int), s));
    const SceneDesc &sdj = sd_job ? *sd_job : sd_pass;
    tj.exit_log = (ctx->exit_probe && prof && launches < NDT_EXIT_LOG_LAUNCHES) ? ws.exit_log + (size_t)launches * NDT_EXIT_LOG_WORDS : nullptr;
    hipEvent_t a = nullptr, b2 = nullptr;
    if (prof) {
        a = get_event(ctx, ev_n++);
        b2 = get_event(ctx, ev_n++);
        trace_ev.push_back({ a, b2 });
        trace_dbg.push_back(what);
    }
    kt->trace(s, ctx->d_blob.as<double>(), sdj, ws, tj, ctx->tier, ctx->sd.mask_words, a, b2);
    ++launches;
    return NDT_OK;
}

// the workspace a shade launch on stream `on` gets: the bank of the shadow answers of bounce b (the bounce it lights, if it lights
// one), and the shade probe's log if it is the probed launch (`finish_nodes` of it are lit; the log is cleared on the launch's stream)
Workspace FrameInFlight::shade_ws(long long finish_nodes, int b, hipStream_t on)
{
    Workspace w = ws;
    w.sobj += answer_bank(b) * ws.sh_cap;
    w.sprim += answer_bank(b) * ws.sh_cap;
    if (shade_launch++ != ctx->shade_probe || !prof) {
        w.shade_log = nullptr;
    } else {
        shade_probe_finish_waves = (finish_nodes + 255) / 256 * 4;
        (void)hipMemsetAsync(w.shade_log, 0, (size_t)2 * NDT_SHADE_LOG_WAVES * sizeof(unsigned int), on);
    }
    return w;
}

// the dense half of a trace launch: closest-hit queries of nodes in the pool
static void job_closest(TraceJob &tj, const Workspace &ws)
{
    tj.dense.o = ws.ray_o; tj.dense.v = ws.ray_v; tj.dense.stride = ws.cap; tj.dense.lim = nullptr;
    tj.dense.valid = ws.depth_left; tj.dense.out_obj = ws.hit_obj; tj.dense.out_prim = ws.hit_prim;
    tj.begin = 0;
}

// the segmented half: shadow rays of bounce b (at most `upper` nodes) in n_seg segments of the shadow queue, counted in seg_count;
// the answers go to bank `bank` of sobj / sprim
static void job_shadow(TraceJob &tj, const Workspace &ws, const SceneDesc &sd_pass, int b, long long upper, int n_seg, const int *seg_count,
                       int bank = 0)
{
    tj.n_seg = n_seg;
    tj.seg.o = ws.so; tj.seg.v = ws.sv; tj.seg.stride = ws.sh_cap; tj.seg.lim = ws.slim; tj.seg.valid = nullptr;
    tj.seg_light_origins = sd_pass.light_origins;      // (what shade_emit_node left out: ndt_kernels.hip)
    tj.seg.out_obj = ws.sobj + bank * ws.sh_cap; tj.seg.out_prim = ws.sprim + bank * ws.sh_cap;
    tj.seg_count = seg_count;
    tj.seg_stride = (upper + 63) & ~63LL;           // sizes the grid only
    tj.levels = ws.levels;
    tj.seg_level = b;
}

// closest-hit queries of the primaries: the only launch that is not shared
int FrameInFlight::trace_primaries()
{
    // (the variant is built for the planar camera: VR and panorama frames take k_primary)
    const bool fuse_primaries = (ctx->fuse_primaries < 0 ? ctx->dims >= 4 : ctx->fuse_primaries != 0) && ctx->cam_type == 0;
    // (no k_primary: the first trace launch makes the primaries it traces, TraceJob::make_primaries)
    if (!fuse_primaries) kt->primary(s, ctx->d_blob.as<double>(), sd_pass, ws, rg);
    TraceJob tj{};
    job_closest(tj, ws);
    tj.count = rg.n_primary;
    tj.publish_level = -1;
    if (fuse_primaries) {
        tj.make_primaries = 1;
        tj.rg = rg;
    }
    return traced(tj, "primaries + closest 0");
}

// Hit points, shadow rays of bounce b, and the rays of the next bounce -- behind the lighting of the previous bounce, which is
// waiting for the shadow answers the last trace launch produced; or (light_overlap) alone: the next trace launch needs what
// shade_emit(b) makes, nothing before the resolve needs what shade_finish(b - 1) does, and that goes to the light stream once
// the stream has passed the trace launch it depends on (render_frame, light_beside)
void FrameInFlight::light_and_shade(int b, long long upper)
{
    if (windowed) {
        // (the lighting of the last window of bounce b-1 and the shading of bounce b see different lights: two launches)
        if (pending_finish >= 0)
            kt->shade_last(s, ctx->d_blob.as<double>(), sd_win[n_win - 1], shade_ws(pending_upper, pending_finish, s), rg, pending_finish, pending_upper, 0,
                           ctx->windows[n_win - 1].first);
        kt->shade_emit(s, ctx->d_blob.as<double>(), sd_win[0], shade_ws(0, b, s), rg, b, upper);
    } else {
        if (!overlap && pending_finish >= 0)
            kt->shade_finish(s, ctx->d_blob.as<double>(), sd_pass, shade_ws(pending_upper, pending_finish, s), rg, pending_finish, pending_upper, 0);
        kt->shade_emit(s, ctx->d_blob.as<double>(), sd_pass, shade_ws(0, b, s), rg, b, upper);
    }
    pending_finish = -1;
}

// ONE launch: shadow rays of bounce b (of its first light window) + closest-hit rays of bounce b + 1, which its prologue publishes
int FrameInFlight::trace_bounce(int b, long long upper)
{
    long long next_upper = 2 * upper;           // each node spawns at most two
    if (next_upper > ws.cap) next_upper = ws.cap;
    TraceJob tj{};
    job_shadow(tj, ws, sd_pass, b, upper, windowed ? ctx->windows[0].n_seg : ctx->n_shadow_lights, NDT_SEG_COUNTERS(ws, b), answer_bank(b));
    job_closest(tj, ws);
    tj.count = next_upper;                      // sizes the grid only
    tj.dense_level = b + 1;
    tj.publish_level = b;
    tj.publish_tag = tag;
    // (light_overlap) the launch writes the bank of answers that shade_finish(b - 3) read: behind it.  That lighting went to the
    // light stream a whole bounce ago (with the tag of bounce b - 1), so in a healthy frame the event is long past, and a wait
    // for a past event puts nothing on the stream
    if (overlap && b >= 3) HIP_TRY(hipStreamWaitEvent(s, ev_lit[b % 3], 0));
    return traced(tj, "shadow " + std::to_string(b) + " + closest " + std::to_string(b + 1), windowed ? &sd_win[0] : nullptr);
}

// Light windows 1 .. of bounce b.  Window k: fold the answers of window k-1 into the nodes' colours and emit their shadow rays of
// window k, then trace them
int FrameInFlight::trace_windows(int b, long long upper)
{
    for (int k = 1; k < n_win; ++k) {
        const ndt_hip_ctx::LightWindow &w = ctx->windows[k];
        int *bank = ws.counters + NDT_CNT_WIN + 64 * (win_emits & 1);
        int *next_bank = ws.counters + NDT_CNT_WIN + 64 * ((win_emits + 1) & 1);
        ++win_emits;
        kt->shade_window(s, ctx->d_blob.as<double>(), sd_win[k - 1], sd_win[k], shade_ws(upper, b, s), rg, b, upper, ctx->windows[k - 1].first, w.first, bank, next_bank,
                         w.n_seg, k > 1 ? 1 : 0);
        if (w.n_seg == 0) continue;
        TraceJob tj{};
        job_shadow(tj, ws, sd_pass, b, upper, w.n_seg, bank);
        tj.count = 0;                               // shadow rays only
        tj.dense_level = -1;
        tj.publish_level = -1;
        int rc = traced(tj, "shadow " + std::to_string(b) + " window " + std::to_string(k), &sd_win[k]);
        if (rc) return rc;
    }
    return NDT_OK;
}

// The lighting of the deepest bounce that has nodes: blended on the spot (its nodes have no child nodes)
// (light_overlap: on the main stream, like the resolve that follows it)
void FrameInFlight::light_last()
{
    if (pending_finish < 0) return;
    resolve_with_finish = pending_finish >= 1 && pending_finish == n_run - 1;
    if (windowed)
        kt->shade_last(s, ctx->d_blob.as<double>(), sd_win[n_win - 1], shade_ws(pending_upper, pending_finish, s), rg, pending_finish, pending_upper,
                       resolve_with_finish ? 1 : 0, ctx->windows[n_win - 1].first);
    else
        kt->shade_finish(s, ctx->d_blob.as<double>(), sd_pass, shade_ws(pending_upper, pending_finish, s), rg, pending_finish, pending_upper,
                         resolve_with_finish ? 1 : 0);
}

// bottom-up colour resolve, deepest bounce first (bounce 0, the primaries: inside k_finish_pixels)
void FrameInFlight::resolve()
{
    for (int b = n_run; b-- > 1;) {
        if (resolve_with_finish && b == n_run - 1) continue;
        long long blocks = (level_nodes[b] + 255) / 256;
        if (blocks > NDT_SHADE_MAX_BLOCKS) blocks = NDT_SHADE_MAX_BLOCKS;
        hipLaunchKernelGGL(k_resolve, dim3((unsigned)blocks), dim3(256), 0, s, ctx->d_blob.as<double>(), sd_pass, ws, rg.specular, b);
    }
}

// k_frame_done is the last kernel of the frame: once its tag is here, the image and the record are complete
int FrameInFlight::close()
{
    launch_stamped(k_frame_done, dim3(1), dim3(64), s, nullptr, ev_end, ws, n_run, ctx->d_done, tag);
    HIP_TRY(hipGetLastError());
    int rc = wait_for_tag(ctx, &ctx->h_done[7], tag, "the frame never completed");
    if (rc) return rc;
    if (prof) HIP_TRY(hipEventSynchronize(ev_end));     // the closing kernel has run: its completion is at most microseconds away
    return NDT_OK;
}

// The closing record (k_frame_done): a pool overflowed somewhere in the frame -- grow it, PASS_AGAIN -- or the pass's statistics
int FrameInFlight::report(long long &cap, long long &sh_cap, ndt_render_stats &st)
{
    const unsigned long long *done = ctx->h_done;
    const int overflow = (int)(long long)done[1], sh_wanted = (int)(long long)done[2];
    if (overflow != 0) {
        if (ctx->debug_levels)
            fprintf(stderr, "ndt_hip: overflow: per-bounce kernels %d (needs %d); pool %lld nodes, %lld shadow slots\n", overflow, sh_wanted, cap,
                    sh_cap);
        if (overflow & 1) cap *= 2;
        if (overflow & 2) {
            sh_cap *= 2;
            if (sh_cap < sh_wanted) sh_cap = sh_wanted;
        }
        return PASS_AGAIN;
    }
    st = ndt_render_stats{};
    st.rays_primary = n_pixels(rg);
    st.rays_secondary = (long long)(int)(long long)done[0] - rg.n_primary;
    st.rays_shadow = (long long)done[3];
    st.rays_ref_equiv = (long long)done[5];
    st.levels = (int)done[4];
    st.trace_launches = launches;
    st.node_capacity = ws.cap;
    if (prof) {
        float ms = 0, fm = 0;
        for (auto &pr : trace_ev) {
            float m = 0;
            HIP_TRY(hipEventElapsedTime(&m, pr.first, pr.second));
            ms += m;
        }
        st.trace_ms = ms;
        if (ctx->debug_levels) HIP_TRY(print_debug(st.levels));
        HIP_TRY(hipEventElapsedTime(&fm, ev_begin, ev_end));
        st.frame_ms = fm;
    }
    return NDT_OK;
}

// NDT_HIP_DEBUG_LEVELS of a profiled pass: the bounce table, the probes, every trace launch's time
hipError_t FrameInFlight::print_debug(int levels_used)
{
    LevelRange *hl = ctx->h_levels;
    const hipError_t e = hipMemcpy(hl, ws.levels, (size_t)(n_run + 1) * sizeof(LevelRange), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int b = 0; b < levels_used; ++b) fprintf(stderr, "ndt_hip: bounce %d: %lld nodes, %lld shadow rays\n", b, hl[b].count, hl[b].n_shadow);
    if (ctx->shade_probe >= 0 && ws.shade_log) print_shade_probe(ws.shade_log, ctx->shade_probe, shade_probe_finish_waves);
    if (ctx->exit_probe) print_exit_probe(ws.exit_log, launches);
    print_phase_timing(ws.dbg);
    for (size_t i = 0; i < trace_ev.size(); ++i) {
        float m = 0;
        (void)hipEventElapsedTime(&m, trace_ev[i].first, trace_ev[i].second);
        fprintf(stderr, "ndt_hip: trace launch %zu: %.3f ms (%s)\n", i, m, trace_dbg[i].c_str());
    }
    return hipSuccess;
}

// Grows the pools and renders again on overflow, at most 8 times
static int render_pass_levels(ndt_hip_ctx *ctx, const RenderGeom &rg, const SceneDesc &sd_pass, bool prof, void *d_rgba, void *d_depth, long long cap,
                              long long sh_cap, ndt_render_stats &st)
{
    for (int attempt = 0; attempt < 8; ++attempt) {
        if (cap > 0x7fffff00LL || sh_cap > 0x7fffff00LL) return fail(NDT_E_NOMEM, "ray tree exceeds 2^31 nodes");
        int rc = ensure_workspace(ctx, cap, sh_cap);
        if (rc) return rc;
        FrameInFlight frame(ctx, rg, sd_pass, prof, d_rgba, d_depth);
        if ((rc = frame.render(cap, sh_cap, st)) != PASS_AGAIN) return rc;
    }
    return fail(NDT_E_NOMEM, "ray-tree workspace kept overflowing");
}

// One pass of the ray pipeline over the primaries `rg` describes: primary rays, the bounce loop,
// bottom-up resolve, per-primary colour (k_finish_pixels) into d_rgba.  Grid mode writes a
// rows x width image, list mode one RGBA per sample.  max_depth > 0 (the callers handle -l 0).
int ndt_impl::render_pass(ndt_hip_ctx *ctx, RenderGeom rg, bool prof, void *d_rgba, ndt_render_stats &st, void *d_depth)
{
    rg.want_depth = d_depth ? 1 : 0;
    const long long n_primary = rg.n_primary;
    long long cap = ctx->ws.cap, sh_cap = ctx->ws.sh_cap;
    if (cap < 2 * n_primary + 4096) cap = 2 * n_primary + 4096;
    const long long want_sh = n_primary * (ctx->n_shadow_lights > 0 ? ctx->n_shadow_lights : 1) + 4096;
    if (sh_cap < want_sh) sh_cap = want_sh;
    if (ctx->test_small_pool && ctx->ws.cap == 0) {
        // tests only: a fresh context starts with a node pool that a reflective scene overflows, so that the
        // overflow -> grow -> render-again path of the two pipelines is exercised (tests/test_gpu_parity.py)
        cap = ((n_primary + 63) & ~63LL) + 64;
    }
    // (the gate prepass of trace_kd: the scene description a pass's kernels get carries the gated items only when it is on)
    SceneDesc sd_pass = ctx->sd;
    if (ctx->gate_prepass == 0 || (ctx->gate_prepass == 2 && n_primary > ctx->gate_prepass_below)) sd_pass.gate_bits = 0ull;
    // (a pass over a LIST of image positions -- recursive anti-aliasing's samples, all of them on the edges the first pass found:
    // 15 rays a sample where a frame has 2.4 a pixel -- crosses over much earlier: profiles/r03_modes_1080p.txt)
    const long long stream_upto = rg.samples ? ctx->stream_below_list : ctx->stream_below;
    // (a scene of more than one light window: the per-bounce kernels, whatever the pipeline -- the frame kernel keeps one 64-bit
    // mask of fired lights per node)
    const bool windowed = ctx->windows.size() > 1;
    const bool use_stream = !windowed && (ctx->pipeline == 2 || (ctx->pipeline == 0 && n_primary <= stream_upto));
    if (use_stream) {
        bool no_room = false;
        const int rc = render_pass_stream(ctx, rg, sd_pass, prof, d_rgba, d_depth, cap, sh_cap, st, no_room);
        // (auto only) the frame kernel keeps one shadow slot per node AND light for the whole frame: with many lights that can
        // exceed what the per-bounce pipeline, which sizes its segments bounce by bounce, needs by far.  When it does not fit --
        // 2^31 slots, or the allocation fails -- auto renders the pass per bounce instead of failing.
        if (!(no_room && ctx->pipeline == 0)) return rc;
        if (cap < ctx->ws.cap) cap = ctx->ws.cap;
        if (sh_cap < ctx->ws.sh_cap) sh_cap = ctx->ws.sh_cap;
    }
    return render_pass_levels(ctx, rg, sd_pass, prof, d_rgba, d_depth, cap, sh_cap, st);
}
