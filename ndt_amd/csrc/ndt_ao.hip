// ndt_ao.hip -- ambient occlusion of a frame on the device (`ndt_hip --ao`): for every pixel that shows something, K rays from the
// N-D hit point of its primary ray, uniform over the hemisphere of the N-D normal there that faces the viewer, and the cosine-weighted
// share of them that get away.  Geometry only.  ndt_hip_ao_device / ndt_hip_render_ao* / ndt_hip_ao_apply_device /
// ndt_hip_render_ao_shaded* / ndt_hip_render_exr_ao; include/ndt_hip.h has the definition to the bit.
//
// A batch of `per` samples is one pass over per * n_primary workspace slots (n_primary: the shard's 8 x 8 tiles, 64 slots each, the
// slots of primary_node; sample kk of the batch stands at kk * n_primary):
//   k_ao_rays<N>               one lane a slot: the sample's direction from its counter-based stream, the ray into ws.ray_o / ray_v
//                              (store_soa's tiles: a wavefront stores 512 contiguous bytes a component), the slot's valid flag, its
//                              dist_limit and its cosine; the direction also to the optional output [K][N][rows * width]
//   NdtKernelTable::trace      the dense job as it is, the per-ray limit and the valid mask in use
//   NdtKernelTable::hitpoints  radius > 0 only: the hit point of every answer
//   k_ao_fold                  one lane a pixel slot: the batch's answers in sample order into the pixel's num / den, carried from
//                              batch to batch in slot order; behind the last sample the plane [rows * width] in pixel order
// and k_ao_apply multiplies a framebuffer's colour by the plane.  Everything on the context's stream, grow-only buffers, no atomics,
// no LDS, no kernel waits for another workgroup, trip counts come from sizes.
#include "ndt_ctx.hpp"
#include <limits.h>

namespace {

constexpr int AO_LANES = 256;
constexpr int FEATURES_ALL = NDT_FEATURE_ID | NDT_FEATURE_POSITION | NDT_FEATURE_NORMAL;
// option "ao_batch" 0: as many samples a launch as fit this many slots (a 1080p frame: four; the frames of the tests: all of them).
// Measured at 1080p, K = 16 (profiles/ao_on_device.txt): 1, 4, 16 samples a launch take 2.70, 1.80, 1.67 ms in 4-D and 30.0, 20.2,
// 18.2 ms in 8-D -- most of what there is to gain comes with four, at a quarter of the workspace sixteen would need
constexpr long long AO_AUTO_SLOTS = 1LL << 23;
// keeps the streams of the AO samples apart from those of `-n` (ns_sample_key: the same hash of pixel and sample number)
constexpr unsigned long long AO_DOMAIN = 0x616f2d72617973ull;

struct AoGeom {
    int width, rows, row_begin, row_step, tiles_x;
    long long n_primary, n_pixels;      // slots of one sample (tiles * 64); pixels of the shard
};

// slot g of a sample <-> lane (g % 64) of 8 x 8 pixel tile (g / 64) (primary_node); false: a padding slot
__device__ __forceinline__ bool ao_pixel_of(const AoGeom &geo, long long g, int &py, int &px)
{
    const long long tile = g >> 6;
    const int lane = (int)(g & 63);
    py = (int)(tile / geo.tiles_x) * 8 + (lane >> 3);
    px = (int)(tile % geo.tiles_x) * 8 + (lane & 7);
    return py < geo.rows && px < geo.width;
}

template <int N>
__global__ void __launch_bounds__(AO_LANES) k_ao_rays(const int *__restrict__ id, const double *__restrict__ position,
                                                      const double *__restrict__ normal, const double *__restrict__ view, AoGeom geo, int k0,
                                                      int per, unsigned long long seed_key, double lim, double *__restrict__ ray_o,
                                                      double *__restrict__ ray_v, int *__restrict__ valid, double *__restrict__ lims,
                                                      double *__restrict__ cosines, double *__restrict__ dirs)
{
    const long long s = (long long)blockIdx.x * AO_LANES + threadIdx.x;
    if (s >= geo.n_primary * per) return;
    const int kk = (int)(s / geo.n_primary);
    const long long g = s - (long long)kk * geo.n_primary;
    int py, px;
    if (!ao_pixel_of(geo, g, py, px)) {
        valid[s] = 0;
        cosines[s] = 0.0;
        return;
    }
    const long long i = (long long)py * geo.width + px;
    const int k = k0 + kk;
    bool live = id[i] != 0;
    double n[N];
    if (live) {
        double len2 = 0.0;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            n[c] = normal[(long long)c * geo.n_pixels + i];
            len2 = len2 + n[c] * n[c];
        }
        const double len = sqrt(len2);
        live = len > 0 && isfinite(len);
        if (live) {
            double facing = 0.0;
#pragma unroll
            for (int c = 0; c < N; ++c) {
                n[c] = n[c] / len;
                facing = facing + n[c] * view[(long long)c * geo.n_pixels + i];
            }
            if (facing > 0) {
#pragma unroll
                for (int c = 0; c < N; ++c) n[c] = -n[c];
            }
        }
    }
    double *const dir_out = dirs ? dirs + (long long)k * N * geo.n_pixels + i : nullptr;
    if (!live) {
        // shows nothing, or a normal without a direction: the pixel's value is 1.0, and it sends no rays
        valid[s] = 0;
        cosines[s] = 0.0;
        if (dir_out) {
#pragma unroll
            for (int c = 0; c < N; ++c) dir_out[(long long)c * geo.n_pixels] = 0.0;
        }
        return;
    }
    // the sample's stream: the image pixel and the sample number, whatever the shard, the batch and K are
    const unsigned long long pixel = (unsigned long long)((long long)(geo.row_begin + py * geo.row_step) * geo.width + px);
    const unsigned long long key = ndt_rng_mix(ndt_rng_mix(pixel * 0x100000001b3ull + (unsigned long long)k) ^ AO_DOMAIN ^ seed_key);
    double d[N];
    double gg = 0.0;
#pragma unroll
    for (int m = 0; m < (N + 1) / 2; ++m) {
        // Box-Muller: two Gaussians from two uniforms
        const double u0 = ndt_rng_uniform(key, 2 * m), u1 = ndt_rng_uniform(key, 2 * m + 1);
        const double r = sqrt(-2.0 * log(1.0 - u0)), a = (2.0 * NDT_PI) * u1;
        d[2 * m] = r * cos(a);
        if (2 * m + 1 < N) d[2 * m + 1] = r * sin(a);
    }
#pragma unroll
    for (int c = 0; c < N; ++c) gg = gg + d[c] * d[c];
    const double norm = sqrt(gg);
    double cs = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        d[c] = d[c] / norm;
        cs = cs + d[c] * n[c];
    }
    if (cs < 0) {
        cs = -cs;
#pragma unroll
        for (int c = 0; c < N; ++c) d[c] = -d[c];
    }
    // store_soa's layout: tiles of 64 slots, component-major inside the tile
    const long long at = (s >> 6) * (long long)(N * 64) + (s & 63);
#pragma unroll
    for (int c = 0; c < N; ++c) {
        ray_o[at + c * 64] = position[(long long)c * geo.n_pixels + i];    // the hit point itself, as a reflection ray's origin (ndt.c:398-402)
        ray_v[at + c * 64] = d[c];
        if (dir_out) dir_out[(long long)c * geo.n_pixels] = d[c];
    }
    valid[s] = 1;
    lims[s] = lim;
    cosines[s] = cs;
}

// acc: [2][n_primary] num and den of every slot between the batches of a call
__global__ void __launch_bounds__(AO_LANES) k_ao_fold(const int *__restrict__ valid, const int *__restrict__ hit_obj,
                                                      const double *__restrict__ cosines, const double *__restrict__ ray_o,
                                                      const double *__restrict__ hit_p, int n, AoGeom geo, int per, int first, int last,
                                                      double radius, double *__restrict__ acc, double *__restrict__ plane)
{
    const long long g = (long long)blockIdx.x * AO_LANES + threadIdx.x;
    if (g >= geo.n_primary) return;
    int py, px;
    if (!ao_pixel_of(geo, g, py, px)) return;
    double num = 0.0, den = 0.0;
    if (!first) {
        num = acc[g];
        den = acc[geo.n_primary + g];
    }
    for (int kk = 0; kk < per; ++kk) {
        const long long s = (long long)kk * geo.n_primary + g;
        if (valid[s] <= 0) continue;
        const double cs = cosines[s];
        bool occluded = hit_obj[s] >= 0;
        if (occluded && radius > 0) {
            // v_dist(hit, origin) in k_features_gather's order: the even components' sum, the odd ones', then the root
            const long long at = (s >> 6) * (long long)(n * 64) + (s & 63);
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
            occluded = sqrt(s0 + s1) < radius;
        }
        den = den + cs;
        if (!occluded) num = num + cs;
    }
    if (last) {
        plane[(long long)py * geo.width + px] = den > 0 ? num / den : 1.0;
    } else {
        acc[g] = num;
        acc[geo.n_primary + g] = den;
    }
}

// one lane a pixel: two 16-byte loads, two 16-byte stores
__global__ void __launch_bounds__(AO_LANES) k_ao_apply(const double2 *__restrict__ in, const double *__restrict__ ao, long long n_pixels,
                                                       double strength, double2 *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * AO_LANES + threadIdx.x;
    if (i >= n_pixels) return;
    const double f = (1.0 - strength) + strength * ao[i];
    const double2 rg = in[2 * i], ba = in[2 * i + 1];
    out[2 * i] = make_double2(rg.x * f, rg.y * f);
    out[2 * i + 1] = make_double2(ba.x * f, ba.y);
}

template <int N>
void launch_rays(hipStream_t s, unsigned grid, const ndt_feature_planes &pl, const AoGeom &geo, int k0, int per, unsigned long long seed_key,
                 double lim, const Workspace &ws, double *cosines, double *dirs)
{
    hipLaunchKernelGGL(k_ao_rays<N>, dim3(grid), dim3(AO_LANES), 0, s, (const int *)pl.id, (const double *)pl.position, (const double *)pl.normal,
                       (const double *)pl.ray_v, geo, k0, per, seed_key, lim, ws.ray_o, ws.ray_v, ws.depth_left, ws.frac, cosines, dirs);
}

ndt_ao_params params_of(const ndt_ao_params *ap)
{
    if (ap) return *ap;
    ndt_ao_params a;
    a.samples = 16;
    a.reserved = 0;
    a.radius = 0.0;
    a.seed = 0;
    a.strength = 1.0;
    return a;
}

int check_params(const char *who, const ndt_ao_params &a)
{
    if (a.samples < 1 || a.samples > 256) return fail(NDT_E_INVALID, "%s: %d samples are outside 1 .. 256", who, a.samples);
    if (a.reserved != 0) return fail(NDT_E_INVALID, "%s: reserved ambient-occlusion parameter set", who);
    if (!(a.radius >= 0) || !isfinite(a.radius)) return fail(NDT_E_INVALID, "%s: radius %g: a finite number, 0 (no limit) or above", who, a.radius);
    if (!(a.strength >= 0 && a.strength <= 1)) return fail(NDT_E_INVALID, "%s: strength %g is outside 0 .. 1", who, a.strength);
    return NDT_OK;
}

// What every entry that takes a frame refuses, before any device work; *a the parameters in force, *v the frame's width and the shard's rows.  any_samples:
// the entry renders `p` as given and takes the AO pass of its deterministic twin (samples = 1)
int refuse(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, const void *out, bool any_samples,
           ndt_ao_params *a, FrameView *v)
{
    if (!ctx || !p || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    *v = FrameView{ nullptr, nullptr, nullptr, p->width, 0 };
    *a = params_of(ap);
    int rc = check_params(who, *a);
    if (rc) return rc;
    if (!ctx->have_scene) return fail(NDT_E_STATE, "%s: no scene uploaded", who);
    if (ctx->dims < NDT_MIN_DIMS || ctx->dims > NDT_MAX_DIMS)
        return fail(NDT_E_INVALID, "%s: %d dimensions are outside %d .. %d", who, ctx->dims, NDT_MIN_DIMS, NDT_MAX_DIMS);
    if (p->recursive_aa)
        return fail(NDT_E_UNSUPPORTED, "%s: no ambient occlusion with recursive_aa: its pixels are averages of corner samples, not one primary ray's hit", who);
    if (p->stereo == NDT_STEREO_ANAGLYPH)
        return fail(NDT_E_UNSUPPORTED, "%s: no ambient occlusion with NDT_STEREO_ANAGLYPH: two primary rays a pixel", who);
    if (p->stereo == NDT_STEREO_HIDEF) return fail(NDT_E_UNSUPPORTED, "%s: no ambient occlusion with NDT_STEREO_HIDEF (frame packing)", who);
    if (p->samples < 1) return fail(NDT_E_INVALID, "%s: samples=%d", who, p->samples);
    if (!any_samples && p->samples > 1)
        return fail(NDT_E_UNSUPPORTED, "%s: samples = %d: the pass starts from the one primary ray of a deterministic frame", who, p->samples);
    ndt_render_params q = *p;
    q.samples = 1;
    return features_check(who, ctx, &q, &v->rows);
}

// The pass for checked arguments, asynchronous on the context's stream: the planes of `pl` (device memory: id, position, normal and
// ray_v of the rows `p` selects) to d_ao, rows * width doubles, and the directions to d_dirs unless that is nullptr.
int ao_pass(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, const ndt_feature_planes &pl, const ndt_ao_params &a, double *d_ao,
            double *d_dirs)
{
    if (!ctx->have_scene || !ctx->kt) return fail(NDT_E_STATE, "%s: no scene uploaded", who);
    HIP_TRY(hipSetDevice(ctx->device));
    AoState &ao = ctx->ao;
    hipStream_t s = ctx->stream;
    ao.launches = 0;
    ao.ms = 0.0;
    ao.timed = false;
    const int n = ctx->dims, K = a.samples;
    AoGeom geo{};
    geo.width = p->width;
    geo.rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    geo.row_begin = p->row_begin;
    geo.row_step = p->row_step;
    geo.tiles_x = (geo.width + 7) / 8;
    geo.n_primary = (long long)geo.tiles_x * ((geo.rows + 7) / 8) * 64;
    geo.n_pixels = (long long)geo.rows * geo.width;
    long long per = ctx->ao_batch > 0 ? ctx->ao_batch : AO_AUTO_SLOTS / geo.n_primary;
    if (per < 1) per = 1;
    if (per > K) per = K;
    const long long cnt_max = per * geo.n_primary;
    if (cnt_max > 0x3fffffffLL)
        return fail(NDT_E_UNSUPPORTED, "%s: %lld samples of %lld slots each are more than one launch takes: a smaller ao_batch", who, per, geo.n_primary);
    int rc = ensure_workspace(ctx, cnt_max > ctx->ws.cap ? cnt_max : ctx->ws.cap, ctx->ws.sh_cap > 0 ? ctx->ws.sh_cap : 4096);
    if (rc) return rc;
    if ((rc = ao.d_cos.reserve((size_t)cnt_max * sizeof(double), s, who))) return rc;
    if ((rc = ao.d_acc.reserve((size_t)geo.n_primary * 2 * sizeof(double), s, who))) return rc;
    if (!ao.ev[0])
        for (hipEvent_t &e : ao.ev) HIP_TRY(hipEventCreate(&e));
    const Workspace ws = ctx->ws;
    // radius 0: any hit occludes, and the trace may stop at the first (dist_limit 0).  radius > 0: the closest hit (dist_limit -1)
    // and its v_dist against the radius.  (object.c:730 leaves early only on a hit with dist < limit, so handing the radius to the
    // trace as its limit would decide the same ray the same way; the closest hit is kept because it is the very query the tests
    // pose through ndt_hip_trace_rays, whose distance is compared here in the same arithmetic.)
    const double lim = a.radius > 0 ? -1.0 : 0.0;
    // ndt_rng_mix(seed), on the host
    unsigned long long seed_key = (unsigned long long)a.seed + 0x9e3779b97f4a7c15ull;
    seed_key = (seed_key ^ (seed_key >> 30)) * 0xbf58476d1ce4e5b9ull;
    seed_key = (seed_key ^ (seed_key >> 27)) * 0x94d049bb133111ebull;
    seed_key = seed_key ^ (seed_key >> 31);
    HIP_TRY(hipEventRecord(ao.ev[0], s));
    for (int k0 = 0; k0 < K; k0 += (int)per) {
        const int here = K - k0 < (int)per ? K - k0 : (int)per;
        const long long cnt = (long long)here * geo.n_primary;
        const unsigned grid = (unsigned)((cnt + AO_LANES - 1) / AO_LANES);
        switch (n) {
        case 3: launch_rays<3>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 4: launch_rays<4>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 5: launch_rays<5>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 6: launch_rays<6>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 7: launch_rays<7>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 8: launch_rays<8>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 9: launch_rays<9>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 10: launch_rays<10>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        case 11: launch_rays<11>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        default: launch_rays<12>(s, grid, pl, geo, k0, here, seed_key, lim, ws, ao.d_cos.as<double>(), d_dirs); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(ws.counters + NDT_CNT_QUEUE, 0, NDT_QUEUE_INTS * sizeof(int), s));
        // (the trace launch leaves the primitive of a slot without a ray alone, and k_hitpoints reads every slot's)
        if (a.radius > 0) HIP_TRY(hipMemsetAsync(ws.hit_prim, 0xff, (size_t)cnt * sizeof(int), s));
        TraceJob tj{};
        tj.n_seg = 0;
        tj.dense.o = ws.ray_o; tj.dense.v = ws.ray_v; tj.dense.stride = ws.cap; tj.dense.lim = ws.frac; tj.dense.valid = ws.depth_left;
        tj.dense.out_obj = ws.hit_obj; tj.dense.out_prim = ws.hit_prim; tj.begin = 0; tj.count = cnt; tj.levels = nullptr;
        tj.queue = ws.counters + NDT_CNT_QUEUE;
        tj.publish_level = -1;
        ctx->kt->trace(s, ctx->d_blob.as<double>(), ctx->sd, ws, tj, ctx->tier, ctx->sd.mask_words, nullptr, nullptr);
        ++ao.launches;
        if (a.radius > 0) {
            ctx->kt->hitpoints(s, ctx->d_blob.as<double>(), ctx->sd, ws.ray_o, ws.ray_v, ws.cap, ws.hit_prim, ws.hit_p, ws.hit_n, cnt);
            ++ao.launches;
        }
        hipLaunchKernelGGL(k_ao_fold, dim3((unsigned)((geo.n_primary + AO_LANES - 1) / AO_LANES)), dim3(AO_LANES), 0, s, (const int *)ws.depth_left,
                           (const int *)ws.hit_obj, (const double *)ao.d_cos.as<double>(), (const double *)ws.ray_o, (const double *)ws.hit_p, n, geo,
                           here, k0 == 0 ? 1 : 0, k0 + here == K ? 1 : 0, a.radius, ao.d_acc.as<double>(), d_ao);
        HIP_TRY(hipGetLastError());
        ao.launches += 2;
    }
    HIP_TRY(hipEventRecord(ao.ev[1], s));
    ao.timed = true;
    return NDT_OK;
}

// after the stream has been synchronised: the device time of the last pass
int collect_ms(ndt_hip_ctx *ctx)
{
    AoState &ao = ctx->ao;
    if (!ao.timed) return NDT_OK;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ao.ev[0], ao.ev[1]));
    ao.ms = ms;
    return NDT_OK;
}

int apply(ndt_hip_ctx *ctx, const void *d_in, const void *d_ao, long long n_pixels, double strength, void *d_out)
{
    hipLaunchKernelGGL(k_ao_apply, dim3((unsigned)((n_pixels + AO_LANES - 1) / AO_LANES)), dim3(AO_LANES), 0, ctx->stream, (const double2 *)d_in,
                       (const double *)d_ao, n_pixels, strength, (double2 *)d_out);
    HIP_TRY(hipGetLastError());
    return NDT_OK;
}

// The feature pass of the deterministic twin of `p` into the context's planes (*planes names them), then the AO pass into d_ao (and
// d_dirs); not synchronised
int features_then_ao(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, const ndt_ao_params &a, double *d_ao, double *d_dirs,
                     ndt_feature_planes *planes)
{
    ndt_render_params q = *p;
    q.samples = 1;
    int rc = features_own(ctx, who, &q, FEATURES_ALL, true, planes);
    if (rc) return rc;
    return ao_pass(ctx, who, &q, *planes, a, d_ao, d_dirs);
}

} // namespace

void ndt_impl::free_ao(ndt_hip_ctx *ctx)
{
    AoState &ao = ctx->ao;
    ao.d_cos.release();
    ao.d_acc.release();
    ao.d_plane.release();
    ao.d_dirs.release();
    ao.d_frame.release();
    for (hipEvent_t &e : ao.ev)
        if (e) (void)hipEventDestroy(e);
    ao = AoState();
}

extern "C" int ndt_hip_ao_launches(ndt_hip_ctx *ctx) { return ctx ? ctx->ao.launches : 0; }
extern "C" double ndt_hip_ao_ms(ndt_hip_ctx *ctx) { return ctx ? ctx->ao.ms : 0.0; }

extern "C" int ndt_hip_ao_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_feature_planes *d_planes, const ndt_ao_params *ap,
                                 void *d_ao, void *d_dirs)
{
    const char *who = "ndt_hip_ao_device";
    if (!d_planes || !d_ao) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, d_ao, false, &a, &v);
    if (rc) return rc;
    if (!d_planes->id || !d_planes->position || !d_planes->normal || !d_planes->ray_v)
        return fail(NDT_E_INVALID, "%s: a NULL plane: the pass starts from id, position, normal and ray_v", who);
    if (((uintptr_t)d_planes->id & 3u) != 0 ||
        (((uintptr_t)d_planes->position | (uintptr_t)d_planes->normal | (uintptr_t)d_planes->ray_v | (uintptr_t)d_ao | (uintptr_t)d_dirs) & 7u) != 0)
        return fail(NDT_E_INVALID, "%s: misaligned: every plane to its elements", who);
    if ((rc = ao_pass(ctx, who, p, *d_planes, a, (double *)d_ao, (double *)d_dirs))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return collect_ms(ctx);
}

extern "C" int ndt_hip_render_ao_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, void *d_ao, void *d_dirs,
                                        ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_ao_device";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, d_ao, true, &a, &v);
    if (rc) return rc;
    if ((((uintptr_t)d_ao | (uintptr_t)d_dirs) & 7u) != 0) return fail(NDT_E_INVALID, "%s: misaligned: the plane and the directions to 8 bytes", who);
    ndt_feature_planes planes;
    if ((rc = features_then_ao(ctx, who, p, a, (double *)d_ao, (double *)d_dirs, &planes))) return rc;
    ctx->ao.launches += ctx->features.launches;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (stats) {
        *stats = ndt_render_stats{};
        stats->rays_primary = p->max_optic_depth > 0 ? (int64_t)v.rows * p->width : 0;
        stats->trace_launches = p->max_optic_depth > 0 ? 1 : 0;
    }
    return collect_ms(ctx);
}

extern "C" int ndt_hip_render_ao(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, double *ao_plane, double *dirs,
                                 ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_ao";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, ao_plane, true, &a, &v);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    AoState &ao = ctx->ao;
    const size_t pixels = (size_t)v.rows * (size_t)p->width, dir_bytes = pixels * (size_t)a.samples * (size_t)ctx->dims * sizeof(double);
    if ((rc = ao.d_plane.reserve(pixels * sizeof(double), ctx->stream, who))) return rc;
    if (dirs && (rc = ao.d_dirs.reserve(dir_bytes, ctx->stream, who))) return rc;
    if ((rc = ndt_hip_render_ao_device(ctx, p, &a, ao.d_plane.p, dirs ? ao.d_dirs.p : nullptr, stats))) return rc;
    HIP_TRY(hipMemcpyAsync(ao_plane, ao.d_plane.p, pixels * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (dirs) HIP_TRY(hipMemcpyAsync(dirs, ao.d_dirs.p, dir_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

extern "C" int ndt_hip_ao_apply_device(ndt_hip_ctx *ctx, const void *d_rgba_in, const void *d_ao, int64_t n_pixels, double strength,
                                       void *d_rgba_out)
{
    const char *who = "ndt_hip_ao_apply_device";
    if (!ctx || !d_rgba_in || !d_ao || !d_rgba_out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (n_pixels < 0 || n_pixels > (int64_t)INT_MAX * AO_LANES) return fail(NDT_E_INVALID, "%s: %lld pixels", who, (long long)n_pixels);
    if (!(strength >= 0 && strength <= 1)) return fail(NDT_E_INVALID, "%s: strength %g is outside 0 .. 1", who, strength);
    if (((uintptr_t)d_rgba_in & 15u) != 0 || ((uintptr_t)d_rgba_out & 15u) != 0 || ((uintptr_t)d_ao & 7u) != 0)
        return fail(NDT_E_INVALID, "%s: misaligned: the images to 16 bytes, the plane to 8", who);
    HIP_TRY(hipSetDevice(ctx->device));
    if (n_pixels == 0) return NDT_OK;
    int rc = apply(ctx, d_rgba_in, d_ao, n_pixels, strength, d_rgba_out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

extern "C" int ndt_hip_render_ao_shaded_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, void *d_rgba, void *d_ao,
                                               ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_ao_shaded_device";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, d_rgba, true, &a, &v);
    if (rc) return rc;
    if (((uintptr_t)d_rgba & 15u) != 0 || ((uintptr_t)d_ao & 7u) != 0)
        return fail(NDT_E_INVALID, "%s: misaligned: the image to 16 bytes, the plane to 8", who);
    HIP_TRY(hipSetDevice(ctx->device));
    const long long pixels = (long long)v.rows * p->width;
    if (!d_ao) {
        if ((rc = ctx->ao.d_plane.reserve((size_t)pixels * sizeof(double), ctx->stream, who))) return rc;
        d_ao = ctx->ao.d_plane.p;
    }
    if ((rc = ndt_hip_render_device(ctx, p, d_rgba, stats))) return rc;
    ndt_feature_planes planes;
    if ((rc = features_then_ao(ctx, who, p, a, (double *)d_ao, nullptr, &planes))) return rc;
    if ((rc = apply(ctx, d_rgba, d_ao, pixels, a.strength, d_rgba))) return rc;
    ctx->ao.launches += ctx->features.launches + 1;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return collect_ms(ctx);
}

// ndt_hip_render_ao_shaded_device into ao.d_frame (*v: sized by refuse), the plane where that entry keeps its own: ao.d_plane
static int render_ao_shaded_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, const ndt_ao_params &a, ndt_render_stats *stats, FrameView *v)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ctx->ao.d_frame.reserve(v->pixels() * 4 * sizeof(double), ctx->stream, who);
    if (rc) return rc;
    v->d_rgba = ctx->ao.d_frame.p;
    return ndt_hip_render_ao_shaded_device(ctx, p, &a, ctx->ao.d_frame.p, nullptr, stats);
}

// The delivering entries (the 8-bit image of those that want one: quantised into ao.d_rgba8 by the tail)
extern "C" int ndt_hip_render_ao_shaded(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, double *rgba, double *ao_plane,
                                        ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_ao_shaded";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, rgba, true, &a, &v);
    if (rc) return rc;
    if ((rc = render_ao_shaded_own(ctx, who, p, a, stats, &v))) return rc;
    // (the plane is no frame: its copy stays here, in front of the frame's on the same stream)
    if (ao_plane) HIP_TRY(hipMemcpyAsync(ao_plane, ctx->ao.d_plane.p, v.pixels() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return deliver_doubles(ctx, v, rgba, nullptr);
}

extern "C" int ndt_hip_render_ao_shaded_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, uint8_t *rgba8,
                                              ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_ao_shaded_rgba8";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, rgba8, true, &a, &v);
    if (rc) return rc;
    if ((rc = render_ao_shaded_own(ctx, who, p, a, stats, &v))) return rc;
    return deliver_rgba8(ctx, who, v, ctx->ao.d_rgba8, rgba8);
}

extern "C" int ndt_hip_render_ao_shaded_png(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, uint8_t *png, int64_t cap,
                                            ndt_png_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_ao_shaded_png";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, png, true, &a, &v);
    if (rc) return rc;
    if ((rc = refuse_png(who, p->width, v.rows, 4))) return rc;
    if ((rc = render_ao_shaded_own(ctx, who, p, a, render_stats, &v))) return rc;
    return deliver_png(ctx, who, v, ctx->ao.d_rgba8, png, cap, stats);
}

extern "C" int ndt_hip_render_ao_shaded_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, const ndt_jpeg_params *jp,
                                             uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_ao_shaded_jpeg";
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, jpg, true, &a, &v);
    if (rc) return rc;
    if ((rc = refuse_jpeg(who, p->width, v.rows, jp))) return rc;
    if ((rc = render_ao_shaded_own(ctx, who, p, a, render_stats, &v))) return rc;
    return deliver_jpeg(ctx, who, v, ctx->ao.d_rgba8, jp, jpg, cap, stats);
}

extern "C" int ndt_hip_render_exr_ao(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int32_t with_depth, int32_t features,
                                     const ndt_ao_params *ap, uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_exr_ao";
    if (stats) *stats = ndt_exr_stats{};
    ndt_ao_params a;
    FrameView v;
    int rc = refuse(who, ctx, p, ap, out, true, &a, &v);
    if (rc) return rc;
    if (cap < 0) return fail(NDT_E_INVALID, "%s: cap %lld", who, (long long)cap);
    if (ndt_hip_exr_ao_bound(p->width, v.rows, ep, with_depth, ctx->dims, features) < 0)
        return fail(NDT_E_INVALID, "%s: no EXR of %d x %d with feature mask %d (id 1, position 2, normal 4, or 0) and these parameters (a pixel type other than 0, 1, 2, or samples beyond 2^31 - 1 bytes)",
                    who, p->width, v.rows, features);
    if ((rc = render_plain_own(ctx, who, p, with_depth != 0, render_stats, &v))) return rc;
    if ((rc = ctx->ao.d_plane.reserve(v.pixels() * sizeof(double), ctx->stream, who))) return rc;
    ndt_feature_planes planes;
    if ((rc = features_then_ao(ctx, who, p, a, ctx->ao.d_plane.as<double>(), nullptr, &planes))) return rc;
    ctx->ao.launches += ctx->features.launches;
    // (strength 0: the colour keeps the bits of the file without AO, whatever they are)
    if (a.strength != 0) {
        if ((rc = apply(ctx, ctx->d_out.p, ctx->ao.d_plane.p, (long long)v.pixels(), a.strength, ctx->d_out.p))) return rc;
        ++ctx->ao.launches;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if ((rc = collect_ms(ctx))) return rc;
    return exr_encode_ao_device(ctx, who, v.d_rgba, v.d_depth, &planes, ctx->ao.d_plane.p, ctx->dims, features, p->width, v.rows, ep, out, cap, stats);
}
