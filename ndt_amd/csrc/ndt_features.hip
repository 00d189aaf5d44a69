// ndt_features.hip -- what a pixel shows: ndt_hip_render_features / ndt_hip_render_features_device / ndt_hip_features_launches.
// The closest hit of every pixel's primary ray -- object, hit point and normal in all N coordinates -- as planes in pixel order.
//
// The pass is built from the per-dimension kernels as they are, the chain ndt_hip_trace_rays runs behind the primaries of a frame:
//   NdtKernelTable::primary    the rays of the shard's pixels into the workspace (the RenderGeom of a deterministic frame)
//   NdtKernelTable::trace      one dense closest-hit job over them, no limit array
//   NdtKernelTable::hitpoints  the winning primitive intersected again: hit point and normal
//   k_features_gather          the workspace's 8 x 8 tiles, component-major slots, to planes [c][rows * width]; a hit within EPSILON
//                              of the ray's origin becomes a miss here (ndt.c:376), as shade_emit_node makes it one
// on the context's stream, behind or in front of a frame: every kernel of a frame writes what it reads of the workspace first.
// No kernel waits for another workgroup, trip counts come from sizes, and there are no atomics.
#include "ndt_ctx.hpp"

namespace {

struct FeatureDst {
    int *id;
    double *position, *normal, *ray_o, *ray_v;
};

// One thread a pixel.  Slot g of the pool <-> lane (g % 64) of 8 x 8 pixel tile (g / 64) (primary_node); a vector's component c
// stands at (g / 64) * n * 64 + c * 64 + g % 64 (store_soa).  Every store is one element of a plane at the pixel's index: the
// lanes of a wavefront write consecutive elements.
__global__ void __launch_bounds__(256) k_features_gather(const int *__restrict__ hit_obj, const double *__restrict__ ray_o,
                                                         const double *__restrict__ ray_v, const double *__restrict__ hit_p,
                                                         const double *__restrict__ hit_n, int n, int width, int tiles_x,
                                                         long long n_pixels, FeatureDst dst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    const int py = (int)(i / width), px = (int)(i - (long long)py * width);
    const long long g = ((long long)(py >> 3) * tiles_x + (px >> 3)) * 64 + ((py & 7) * 8 + (px & 7));
    const long long at = (g >> 6) * (long long)(n * 64) + (g & 63);
    int obj = hit_obj[g];
    if (obj >= 0) {
        // v_dist(hit, origin) in vectNd_dot's order (vectNd.h:215-227): the even components' sum, the odd ones', then the root
        double d0 = hit_p[at] - ray_o[at], d1 = hit_p[at + 64] - ray_o[at + 64];
        double s0 = d0 * d0, s1 = d1 * d1;
        for (int c = 2; c < n; c += 2) {
            d0 = hit_p[at + c * 64] - ray_o[at + c * 64];
            s0 = s0 + d0 * d0;
            if (c + 1 < n) {
                d1 = hit_p[at + (c + 1) * 64] - ray_o[at + (c + 1) * 64];
                s1 = s1 + d1 * d1;
            }
        }
        if (!(sqrt(s0 + s1) > NDT_EPS)) obj = -1;       // ndt.c:376
    }
    if (dst.id) dst.id[i] = obj + 1;
    for (int c = 0; c < n; ++c) {
        const long long to = (long long)c * n_pixels + i, from = at + c * 64;
        if (dst.position) dst.position[to] = obj >= 0 ? hit_p[from] : 0.0;
        if (dst.normal) dst.normal[to] = obj >= 0 ? hit_n[from] : 0.0;
        if (dst.ray_o) dst.ray_o[to] = ray_o[from];
        if (dst.ray_v) dst.ray_v[to] = ray_v[from];
    }
}

} // namespace

void ndt_impl::free_features(ndt_hip_ctx *ctx)
{
    FeatureState &f = ctx->features;
    f.d_id.release();
    f.d_position.release();
    f.d_normal.release();
    f.d_ray_o.release();
    f.d_ray_v.release();
    f = FeatureState();
}

int ndt_impl::features_check(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, int *rows)
{
    if (!ctx || !p) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (!ctx->have_scene) return fail(NDT_E_STATE, "%s: no scene uploaded", who);
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0)
        return fail(NDT_E_INVALID, "%s: bad geometry: %d x %d, rows %d by %d", who, p->width, p->height, p->row_begin, p->row_step);
    for (int k = 0; k < 4; ++k)
        if (p->reserved[k] != 0) return fail(NDT_E_INVALID, "%s: reserved render parameter set", who);
    if (p->samples < 1) return fail(NDT_E_INVALID, "%s: samples=%d", who, p->samples);
    if (p->recursive_aa)
        return fail(NDT_E_UNSUPPORTED, "%s: no features of a recursive_aa frame: its pixels are averages of corner samples, not one primary ray", who);
    if (p->samples > 1) return fail(NDT_E_UNSUPPORTED, "%s: no features with samples = %d: a pixel has no single primary ray", who, p->samples);
    if (p->stereo == NDT_STEREO_ANAGLYPH) return fail(NDT_E_UNSUPPORTED, "%s: no features of an anaglyph frame: two primary rays a pixel", who);
    if (p->stereo == NDT_STEREO_HIDEF) return fail(NDT_E_UNSUPPORTED, "%s: no features of a frame-packed (HIDEF) frame", who);
    if (p->stereo < NDT_STEREO_MONO || p->stereo > NDT_STEREO_HIDEF) return fail(NDT_E_UNSUPPORTED, "%s: stereo mode %d", who, p->stereo);
    if (p->stereo != NDT_STEREO_MONO && !ctx->have_eyes)
        return fail(NDT_E_INVALID, "%s: stereo needs leftEye / rightEye (camera.h:60-61) in the flat scene", who);
    *rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    if (*rows < 1) return refuse_empty_shard(who, *rows);
    const long long n_primary = (long long)((p->width + 7) / 8) * ((*rows + 7) / 8) * 64;
    if (n_primary > 0x3fffffffLL) return fail(NDT_E_UNSUPPORTED, "%s: image too large for one call", who);
    return NDT_OK;
}

int ndt_impl::features_pass(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, const ndt_feature_planes &dst)
{
    if (!ctx->have_scene || !ctx->kt) return fail(NDT_E_STATE, "%s: no scene uploaded", who);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n = ctx->dims, rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    const long long n_pixels = (long long)rows * p->width;
    ctx->features.launches = 0;
    if (p->max_optic_depth <= 0) {
        // get_ray_color returns without tracing (ndt.c:340): no pixel shows anything, and the depth map holds zeros
        if (dst.id) HIP_TRY(hipMemsetAsync(dst.id, 0, (size_t)n_pixels * sizeof(int), s));
        for (double *plane : { dst.position, dst.normal, dst.ray_o, dst.ray_v })
            if (plane) HIP_TRY(hipMemsetAsync(plane, 0, (size_t)n * n_pixels * sizeof(double), s));
        return NDT_OK;
    }
    // the RenderGeom ndt_hip_render_depth_device makes for a deterministic frame
    RenderGeom rg{};
    rg.width = p->width;
    rg.height = p->height;
    rg.row_begin = p->row_begin;
    rg.row_step = p->row_step;
    rg.rows = rows;
    rg.tiles_x = (rg.width + 7) / 8;
    rg.tiles_y = (rg.rows + 7) / 8;
    rg.n_primary = rg.tiles_x * rg.tiles_y * 64;
    rg.max_depth = p->max_optic_depth;
    rg.specular = p->specular ? 1 : 0;
    rg.img_w = p->width;
    rg.img_h = p->height;
    rg.aspect_w = p->width;
    rg.aspect_h = p->height;
    rg.eye = 1;
    rg.stereo = p->stereo;
    const long long cnt = rg.n_primary;
    int rc = ensure_workspace(ctx, cnt > ctx->ws.cap ? cnt : ctx->ws.cap, ctx->ws.sh_cap > 0 ? ctx->ws.sh_cap : 4096);
    if (rc) return rc;
    const Workspace ws = ctx->ws;
    // (the trace launch leaves the primitive of a padding slot alone, and k_hitpoints reads every slot's)
    HIP_TRY(hipMemsetAsync(ws.hit_prim, 0xff, (size_t)cnt * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(ws.counters + NDT_CNT_QUEUE, 0, NDT_QUEUE_INTS * sizeof(int), s));
    ctx->kt->primary(s, ctx->d_blob.as<double>(), ctx->sd, ws, rg);
    TraceJob tj{};
    tj.n_seg = 0;
    tj.dense.o = ws.ray_o; tj.dense.v = ws.ray_v; tj.dense.stride = ws.cap; tj.dense.lim = nullptr; tj.dense.valid = ws.depth_left;
    tj.dense.out_obj = ws.hit_obj; tj.dense.out_prim = ws.hit_prim; tj.begin = 0; tj.count = cnt; tj.levels = nullptr;
    tj.queue = ws.counters + NDT_CNT_QUEUE;
    tj.publish_level = -1;
    ctx->kt->trace(s, ctx->d_blob.as<double>(), ctx->sd, ws, tj, ctx->tier, ctx->sd.mask_words, nullptr, nullptr);
    ctx->kt->hitpoints(s, ctx->d_blob.as<double>(), ctx->sd, ws.ray_o, ws.ray_v, ws.cap, ws.hit_prim, ws.hit_p, ws.hit_n, cnt);
    FeatureDst d;
    d.id = dst.id; d.position = dst.position; d.normal = dst.normal; d.ray_o = dst.ray_o; d.ray_v = dst.ray_v;
    hipLaunchKernelGGL(k_features_gather, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, (const int *)ws.hit_obj,
                       (const double *)ws.ray_o, (const double *)ws.ray_v, (const double *)ws.hit_p, (const double *)ws.hit_n, n, rg.width,
                       rg.tiles_x, n_pixels, d);
    HIP_TRY(hipGetLastError());
    ctx->features.launches = 4;
    return NDT_OK;
}

int ndt_impl::features_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, int features, bool with_rays,
                           ndt_feature_planes *own)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const int rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    const size_t pixels = (size_t)rows * (size_t)p->width, vec = pixels * (size_t)ctx->dims * sizeof(double);
    FeatureState &f = ctx->features;
    *own = ndt_feature_planes{};
    int rc;
    if (features & NDT_FEATURE_ID) {
        if ((rc = f.d_id.reserve(pixels * sizeof(int32_t), ctx->stream, who))) return rc;
        own->id = f.d_id.as<int32_t>();
    }
    if (features & NDT_FEATURE_POSITION) {
        if ((rc = f.d_position.reserve(vec, ctx->stream, who))) return rc;
        own->position = f.d_position.as<double>();
    }
    if (features & NDT_FEATURE_NORMAL) {
        if ((rc = f.d_normal.reserve(vec, ctx->stream, who))) return rc;
        own->normal = f.d_normal.as<double>();
    }
    if (with_rays) {
        if ((rc = f.d_ray_o.reserve(vec, ctx->stream, who))) return rc;
        if ((rc = f.d_ray_v.reserve(vec, ctx->stream, who))) return rc;
        own->ray_o = f.d_ray_o.as<double>();
        own->ray_v = f.d_ray_v.as<double>();
    }
    return features_pass(ctx, who, p, *own);
}

static void feature_stats(const ndt_render_params *p, int rows, ndt_render_stats *stats)
{
    if (!stats) return;
    *stats = ndt_render_stats{};
    if (p->max_optic_depth <= 0) return;
    stats->rays_primary = (int64_t)rows * p->width;
    stats->trace_launches = 1;
}

extern "C" int ndt_hip_render_features_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_feature_planes *d_planes,
                                              ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_features_device";
    int rows = 0;
    if (!d_planes) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    int rc = features_check(who, ctx, p, &rows);
    if (rc) return rc;
    if (!d_planes->id && !d_planes->position && !d_planes->normal && !d_planes->ray_o && !d_planes->ray_v)
        return fail(NDT_E_INVALID, "%s: no plane is asked for", who);
    if (((uintptr_t)d_planes->id & 3u) != 0 ||
        (((uintptr_t)d_planes->position | (uintptr_t)d_planes->normal | (uintptr_t)d_planes->ray_o | (uintptr_t)d_planes->ray_v) & 7u) != 0)
        return fail(NDT_E_INVALID, "%s: a plane is not aligned to its elements", who);
    if ((rc = features_pass(ctx, who, p, *d_planes))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    feature_stats(p, rows, stats);
    return NDT_OK;
}

extern "C" int ndt_hip_render_features(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_feature_planes *planes, ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_features";
    int rows = 0;
    if (!planes) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    int rc = features_check(who, ctx, p, &rows);
    if (rc) return rc;
    if (!planes->id && !planes->position && !planes->normal && !planes->ray_o && !planes->ray_v)
        return fail(NDT_E_INVALID, "%s: no plane is asked for", who);
    if ((planes->ray_o == nullptr) != (planes->ray_v == nullptr)) return fail(NDT_E_INVALID, "%s: ray_o and ray_v come together", who);
    const int features = (planes->id ? NDT_FEATURE_ID : 0) | (planes->position ? NDT_FEATURE_POSITION : 0) | (planes->normal ? NDT_FEATURE_NORMAL : 0);
    ndt_feature_planes own;
    if ((rc = features_own(ctx, who, p, features, planes->ray_o != nullptr, &own))) return rc;
    hipStream_t s = ctx->stream;
    const size_t pixels = (size_t)rows * (size_t)p->width, vec = pixels * (size_t)ctx->dims * sizeof(double);
    if (planes->id) HIP_TRY(hipMemcpyAsync(planes->id, own.id, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (planes->position) HIP_TRY(hipMemcpyAsync(planes->position, own.position, vec, hipMemcpyDeviceToHost, s));
    if (planes->normal) HIP_TRY(hipMemcpyAsync(planes->normal, own.normal, vec, hipMemcpyDeviceToHost, s));
    if (planes->ray_o) HIP_TRY(hipMemcpyAsync(planes->ray_o, own.ray_o, vec, hipMemcpyDeviceToHost, s));
    if (planes->ray_v) HIP_TRY(hipMemcpyAsync(planes->ray_v, own.ray_v, vec, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    feature_stats(p, rows, stats);
    return NDT_OK;
}

extern "C" int ndt_hip_features_launches(ndt_hip_ctx *ctx) { return ctx ? ctx->features.launches : 0; }
