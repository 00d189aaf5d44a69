// ndt_render.hip -- ndt_hip_render*: render_image (ndt.c:900) behind the C ABI: argument checks, and the choice between
// the deterministic pass, recursive anti-aliasing and the sampled paths; and the delivery of frames staged on the device (FrameView).
#include "ndt_ctx.hpp"

// true anaglyph (ndt.c:643-647): red = luminance of the left eye's colour, blue = of the right eye's
__global__ void k_anaglyph(const double *left, const double *right, double *out, long long n_pixels)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const double *l = left + 4 * i, *r = right + 4 * i;
    out[4 * i + 0] = 0.299 * l[0] + 0.587 * l[1] + 0.114 * l[2];
    out[4 * i + 1] = 0;
    out[4 * i + 2] = 0.299 * r[0] + 0.587 * r[1] + 0.114 * r[2];
    out[4 * i + 3] = 1.0;
}

void ndt_impl::launch_anaglyph(hipStream_t s, const double *left, const double *right, double *out, long long n_pixels)
{
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_anaglyph, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, left, right, out, n_pixels);
}

// The moments of a frame that does not go through the sampled loop: one sample a pixel, the pixel itself
__global__ void k_moments_single(const double *rgba, int *count, double *sum_sq, long long n_pixels)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    count[i] = 1;
    for (int c = 0; c < 3; ++c) sum_sq[c * n_pixels + i] = rgba[4 * i + c] * rgba[4 * i + c];
}

// ndt_hip_render_depth_device; mo (ndt_hip_render_moments*, whose refusals the caller has made): the frame's sample moments too
static int render_frame(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, void *d_depth, ndt_render_stats *stats, const SampleMoments *mo)
{
    if (!ctx || !p || !d_rgba) return fail(NDT_E_INVALID, "NULL argument");
    if (!ctx->have_scene) return fail(NDT_E_STATE, "no scene uploaded");
    if (p->samples < 1) return fail(NDT_E_INVALID, "samples=%d", p->samples);
    const bool stochastic = p->samples > 1 || ctx->has_area_lights;
    // (a stochastic anti-aliased render -- a lens, area lights or -n > 1 under -a -- has no depth map here: the map would be
    // the last lens sample's of every first-pass corner)
    if (p->recursive_aa && d_depth && (stochastic || ctx->aperture_radius != 0.0))
        return fail(NDT_E_UNSUPPORTED, "no depth map beside a stochastic anti-aliased render (lens, area lights or samples > 1 with recursive_aa)");
    if (p->samples > 1 && ctx->aperture_radius != 0.0 && !ctx->have_local_axes)
        return fail(NDT_E_INVALID, "depth of field needs the camera's local axes (camera.h:69-71) in the flat scene");
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0) return fail(NDT_E_INVALID, "bad geometry");
    if (p->stereo < NDT_STEREO_MONO || p->stereo > NDT_STEREO_HIDEF) return fail(NDT_E_UNSUPPORTED, "stereo mode %d", p->stereo);
    if (p->stereo != NDT_STEREO_MONO && !ctx->have_eyes) return fail(NDT_E_INVALID, "stereo needs leftEye / rightEye (camera.h:60-61) in the flat scene");
    for (int k = 0; k < 4; ++k)
        if (p->reserved[k] != 0) return fail(NDT_E_INVALID, "reserved render parameter set");
    if (p->recursive_aa && ctx->aperture_radius != 0.0 && !ctx->have_local_axes)
        return fail(NDT_E_INVALID, "depth of field needs the camera's local axes (camera.h:69-71) in the flat scene");
    if (p->recursive_aa && (p->aa_diff < 0 || p->aa_depth > 24)) return fail(NDT_E_INVALID, "bad anti-aliasing parameters");
    // (the reference's recursive_resample averages the alpha of its samples, and the samples that fall on the 45 blank lines
    // of a frame-packed image come back with an alpha nobody set, ndt.c:662, 625-627: there is nothing to be equal to)
    if (p->recursive_aa && p->stereo == NDT_STEREO_HIDEF)
        return fail(NDT_E_UNSUPPORTED, "recursive anti-aliasing of a frame-packed image reads uninitialised alpha in the reference (ndt.c:662)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    ndt_render_stats st{};
    if (rows == 0) {
        if (stats) *stats = st;
        return NDT_OK;
    }
    const long long n_pixels = (long long)rows * p->width;
    if (p->max_optic_depth <= 0) {
        // get_ray_color returns black without tracing (ndt.c:340); averages of black are black
        launch_fill_black(s, (double *)d_rgba, n_pixels);
        if (d_depth) HIP_TRY(hipMemsetAsync(d_depth, 0, (size_t)n_pixels * sizeof(double), s));
        if (mo) hipLaunchKernelGGL(k_moments_single, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, (const double *)d_rgba, (int *)mo->d_count, (double *)mo->d_sum_sq, n_pixels);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        if (stats) *stats = st;
        return NDT_OK;
    }
    int rc;
    // the reference's switch: -a with depth >= 0 and diff < 256 resamples, otherwise the first pass is copied (ndt.c:1040)
    if (p->recursive_aa) {
        rc = render_antialiased(ctx, p, d_rgba, st, d_depth);
    } else if (stochastic) {
        rc = render_sampled(ctx, p, d_rgba, st, d_depth, mo);
    } else {
        RenderGeom rg{};
        rg.width = p->width;
        rg.height = p->height;
        rg.row_begin = p->row_begin;
        rg.row_step = p->row_step;
        rg.rows = rows;
        rg.tiles_x = (rg.width + 7) / 8;
        rg.tiles_y = (rg.rows + 7) / 8;
        const long long n_primary = (long long)rg.tiles_x * rg.tiles_y * 64;
        if (n_primary > 0x3fffffffLL) return fail(NDT_E_UNSUPPORTED, "image too large for one call");
        rg.n_primary = (int)n_primary;
        rg.max_depth = p->max_optic_depth;
        rg.specular = p->specular ? 1 : 0;
        rg.img_w = p->width;
        rg.img_h = p->height;
        rg.aspect_w = p->width;
        rg.aspect_h = p->height;
        rg.eye = 1;
        if (p->stereo == NDT_STEREO_ANAGLYPH) {
            // two full renders, one per eye (ndt.c:636-647); the depth map is the left eye's
            AaBuffers buf(ctx);
            double *left = nullptr, *right = nullptr;
            if ((rc = buf.get(&left, (size_t)n_pixels * 4))) return rc;
            if ((rc = buf.get(&right, (size_t)n_pixels * 4))) return rc;
            ndt_render_stats one{};
            rg.eye = 0;
            if ((rc = render_pass(ctx, rg, p->profile != 0, left, one, d_depth))) return rc;
            add_stats(st, one);
            rg.eye = 2;
            if ((rc = render_pass(ctx, rg, p->profile != 0, right, one))) return rc;
            add_stats(st, one);
            launch_anaglyph(s, left, right, (double *)d_rgba, n_pixels);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
            rc = NDT_OK;
        } else {
            rg.stereo = p->stereo;
            if (p->stereo == NDT_STEREO_HIDEF) {
                // frame packing (ndt.c:614-631, 927-928): the aspect is width/1080 and the 45 blank lines between the
                // eyes stay black (the reference leaves their alpha unset; 1 here)
                rg.aspect_h = 1080;
                launch_fill_black(s, (double *)d_rgba, n_pixels);
                if (d_depth) HIP_TRY(hipMemsetAsync(d_depth, 0, (size_t)n_pixels * sizeof(double), s));
            }
            rc = render_pass(ctx, rg, p->profile != 0, d_rgba, st, d_depth);
        }
        if (!rc && mo) {
            // no sampled loop, no such state: one sample a pixel, the pixel itself
            hipLaunchKernelGGL(k_moments_single, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, (const double *)d_rgba, (int *)mo->d_count, (double *)mo->d_sum_sq, n_pixels);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    if (rc) return rc;
    if (stats) *stats = st;
    return NDT_OK;
}

extern "C" int ndt_hip_render_depth_device(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, void *d_depth,
                                           ndt_render_stats *stats)
{
    return render_frame(ctx, p, d_rgba, d_depth, stats, nullptr);
}

int ndt_impl::moments_refuse(const char *who, const ndt_render_params *p)
{
    if (p->recursive_aa)
        return fail(NDT_E_UNSUPPORTED, "%s: no sample moments of a recursive_aa frame: its pixels are averages of corner samples, not of the loop's samples", who);
    if (p->stereo == NDT_STEREO_ANAGLYPH) return fail(NDT_E_UNSUPPORTED, "%s: no sample moments of an NDT_STEREO_ANAGLYPH frame: a pixel mixes two loops", who);
    if (p->stereo == NDT_STEREO_HIDEF) return fail(NDT_E_UNSUPPORTED, "%s: no sample moments of an NDT_STEREO_HIDEF (frame-packed) frame", who);
    return NDT_OK;
}

extern "C" int ndt_hip_render_moments_device(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, void *d_count, void *d_sum_sq,
                                             ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_moments_device";
    if (!ctx || !p || !d_rgba || !d_count || !d_sum_sq) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (((uintptr_t)d_count & 3u) != 0 || ((uintptr_t)d_sum_sq & 7u) != 0) return fail(NDT_E_INVALID, "%s: misaligned: the counts to 4 bytes, the sums to 8", who);
    const int rc = moments_refuse(who, p);
    if (rc) return rc;
    const SampleMoments mo{ d_count, d_sum_sq };
    return render_frame(ctx, p, d_rgba, nullptr, stats, &mo);
}

extern "C" int ndt_hip_render_moments(ndt_hip_ctx *ctx, const ndt_render_params *p, double *rgba, int32_t *count, double *sum_sq,
                                      ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_moments";
    if (!ctx || !p || !rgba || !count || !sum_sq) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    int rc = moments_refuse(who, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rows = p->width > 0 && p->height > 0 && p->row_step > 0 && p->row_begin >= 0 ? ndt_hip_shard_rows(p->height, p->row_begin, p->row_step) : 0;
    if (rows == 0) return render_frame(ctx, p, (void *)ctx, nullptr, stats, nullptr);      // no pixels: the render call's word on `p`
    const size_t pixels = (size_t)rows * (size_t)p->width;
    if ((rc = ctx->d_out.reserve(pixels * 4 * sizeof(double), ctx->stream, who))) return rc;
    if ((rc = ctx->d_moments.reserve(pixels * (3 * sizeof(double) + sizeof(int32_t)), ctx->stream, who))) return rc;
    const SampleMoments mo{ ctx->d_moments.as<char>() + pixels * 3 * sizeof(double), ctx->d_moments.p };
    if ((rc = render_frame(ctx, p, ctx->d_out.p, nullptr, stats, &mo))) return rc;
    HIP_TRY(hipMemcpyAsync(rgba, ctx->d_out.p, pixels * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(count, mo.d_count, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(sum_sq, mo.d_sum_sq, pixels * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

extern "C" int ndt_hip_render_device(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, ndt_render_stats *stats)
{
    return ndt_hip_render_depth_device(ctx, p, d_rgba, nullptr, stats);
}

extern "C" int ndt_hip_render(ndt_hip_ctx *ctx, const ndt_render_params *p, double *rgba, ndt_render_stats *stats)
{
    return ndt_hip_render_depth(ctx, p, rgba, nullptr, stats);
}

extern "C" int ndt_hip_render_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, double *rgba, double *depth, ndt_render_stats *stats)
{
    if (!ctx || !p || !rgba) return fail(NDT_E_INVALID, "NULL argument");
    FrameView v;
    const int rc = render_plain_own(ctx, "ndt_hip_render", p, depth != nullptr, stats, &v);
    if (rc || v.rows == 0) return rc;
    return deliver_doubles(ctx, v, rgba, depth);
}

int ndt_impl::render_plain_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, bool want_depth, ndt_render_stats *stats, FrameView *v)
{
    HIP_TRY(hipSetDevice(ctx->device));
    *v = FrameView{ nullptr, nullptr, nullptr, p->width, p->width > 0 ? ndt_hip_shard_rows(p->height, p->row_begin, p->row_step) : 0 };
    if (v->rows == 0) return ndt_hip_render_depth_device(ctx, p, (void *)ctx, nullptr, stats);
    const size_t img_bytes = v->pixels() * 4 * sizeof(double);
    const int rc = ctx->d_out.reserve(img_bytes + (want_depth ? img_bytes / 4 : 0), ctx->stream, who);      // the map sits behind the image
    if (rc) return rc;
    v->d_rgba = ctx->d_out.p;
    if (want_depth) v->d_depth = ctx->d_out.as<char>() + img_bytes;
    return ndt_hip_render_depth_device(ctx, p, ctx->d_out.p, (void *)v->d_depth, stats);
}

int ndt_impl::refuse_empty_shard(const char *who, int rows) { return rows < 1 ? fail(NDT_E_INVALID, "%s: the shard has no rows", who) : NDT_OK; }

int ndt_impl::refuse_png(const char *who, int32_t width, int32_t rows, int bpp)
{
    if (rows < 1) return refuse_empty_shard(who, rows);
    if ((bpp == 4 ? ndt_hip_png_bound(width, rows) : ndt_hip_png16_bound(width, rows, bpp == 8 ? 4 : 1)) < 0)
        return fail(NDT_E_INVALID, "%s: the filtered stream of a %d x %d image exceeds 2^31 - 1 bytes", who, width, rows);
    return NDT_OK;
}

int ndt_impl::refuse_jpeg(const char *who, int32_t width, int32_t rows, const ndt_jpeg_params *jp)
{
    if (rows < 1) return refuse_empty_shard(who, rows);
    if (ndt_hip_jpeg_bound(width, rows, jp) < 0)
        return fail(NDT_E_INVALID, "%s: no JPEG of %d x %d with these parameters (a side above 65535, a quality outside 0 .. 100, a sampling outside 0 .. 1 or a reserved word set)",
                    who, width, rows);
    return NDT_OK;
}

// v.d_rgba8 becomes the frame's 8-bit image -- the producer's, or quantised into stage8 -- behind, where the sink takes the map, the
// finished 8-bit map in *stage_depth8 and its range in range_out.  Queued, not synchronised.
static int images8(ndt_hip_ctx *ctx, const char *who, FrameView &v, DeviceBuffer &stage8, DeviceBuffer *stage_depth8, double *range_out)
{
    int rc;
    if (stage_depth8) {
        if ((rc = stage_depth8->reserve(v.pixels() * 4, ctx->stream, who))) return rc;
        if ((rc = ndt_hip_depth_rgba8_device(ctx, v.d_depth, (int64_t)v.pixels(), stage_depth8->p, range_out))) return rc;
    }
    if (v.d_rgba8) return NDT_OK;
    if ((rc = stage8.reserve(v.pixels() * 4, ctx->stream, who))) return rc;
    v.d_rgba8 = stage8.p;
    return ndt_hip_quantize_device(ctx, v.d_rgba, stage8.p, (int64_t)v.pixels());
}

int ndt_impl::deliver_doubles(ndt_hip_ctx *ctx, const FrameView &v, double *rgba, double *depth)
{
    const size_t img_bytes = v.pixels() * 4 * sizeof(double);
    HIP_TRY(hipMemcpyAsync(rgba, v.d_rgba, img_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (depth) HIP_TRY(hipMemcpyAsync(depth, v.d_depth, img_bytes / 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

int ndt_impl::deliver_rgba8(ndt_hip_ctx *ctx, const char *who, FrameView v, DeviceBuffer &stage8, uint8_t *rgba8, DeviceBuffer *stage_depth8,
                            uint8_t *depth8, double *range_out)
{
    const int rc = images8(ctx, who, v, stage8, stage_depth8, range_out);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(rgba8, v.d_rgba8, v.pixels() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (stage_depth8) HIP_TRY(hipMemcpyAsync(depth8, stage_depth8->p, v.pixels() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

int ndt_impl::deliver_png(ndt_hip_ctx *ctx, const char *who, FrameView v, DeviceBuffer &stage8, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                          DeviceBuffer *stage_depth8, uint8_t *depth_png, int64_t depth_cap, uint8_t *depth8, double *range_out)
{
    int rc = images8(ctx, who, v, stage8, stage_depth8, range_out);
    if (rc) return rc;
    if ((rc = ndt_hip_encode_png_device(ctx, v.d_rgba8, v.width, v.rows, png, cap, stats)) || !stage_depth8) return rc;
    if (depth_png) return ndt_hip_encode_png_device(ctx, stage_depth8->p, v.width, v.rows, depth_png, depth_cap, stats ? &stats[1] : nullptr);
    HIP_TRY(hipMemcpyAsync(depth8, stage_depth8->p, v.pixels() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

int ndt_impl::deliver_png16(ndt_hip_ctx *ctx, const char *who, const FrameView &v, DeviceBuffer &stage16, DeviceBuffer &stage_grey16,
                            uint8_t *png, int64_t cap, uint8_t *depth_png, int64_t depth_cap, ndt_png_stats *stats, double *range_out)
{
    int rc = stage16.reserve(v.pixels() * 8, ctx->stream, who);
    if (rc) return rc;
    if ((rc = ndt_hip_quantize16_device(ctx, v.d_rgba, stage16.p, (int64_t)v.pixels()))) return rc;
    if (depth_png) {
        if ((rc = stage_grey16.reserve((v.pixels() * 2 + 3) & ~(size_t)3, ctx->stream, who))) return rc;
        if ((rc = ndt_hip_depth_grey16_device(ctx, v.d_depth, (int64_t)v.pixels(), stage_grey16.p, range_out))) return rc;
    }
    if ((rc = ndt_hip_encode_png16_device(ctx, stage16.p, v.width, v.rows, 4, png, cap, stats)) || !depth_png) return rc;
    return ndt_hip_encode_png16_device(ctx, stage_grey16.p, v.width, v.rows, 1, depth_png, depth_cap, stats ? &stats[1] : nullptr);
}

int ndt_impl::deliver_jpeg(ndt_hip_ctx *ctx, const char *who, FrameView v, DeviceBuffer &stage8, const ndt_jpeg_params *jp, uint8_t *jpg,
                           int64_t cap, ndt_jpeg_stats *stats)
{
    const int rc = images8(ctx, who, v, stage8, nullptr, nullptr);
    return rc ? rc : ndt_hip_encode_jpeg_device(ctx, v.d_rgba8, v.width, v.rows, jp, jpg, cap, stats);
}

int ndt_impl::deliver_exr(ndt_hip_ctx *ctx, const FrameView &v, const ndt_exr_params *ep, uint8_t *out, int64_t cap, ndt_exr_stats *stats)
{
    return ndt_hip_encode_exr_device(ctx, v.d_rgba, v.d_depth, v.width, v.rows, ep, out, cap, stats);
}
