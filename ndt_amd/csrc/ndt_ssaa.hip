// ndt_ssaa.hip -- regular K x K supersampling of a frame on the device (`ndt_hip --ssaa K`): the W x H frame is the K W x K H frame
// of the same scene and camera, averaged over K x K blocks in doubles, in linear light, before pixel_d2c.
//
// Sub-row a of the output rows of a shard (row_begin = b, row_step = S) is the set of large-frame rows { K (b + k S) + a }: the
// cyclic shard row_begin = K b + a, row_step = K S of the K W x K H frame.  A frame is therefore K ordinary renders through
// ndt_hip_render_depth_device -- no kernel of the render path changes -- each followed by one launch of
//
//   k_ssaa_fold    adds the pass's K sub-columns into the W x rows accumulator: out = (((s00 + s01) + ... + s0,K-1) + s10 + ...),
//                  strictly left to right, sub-row outer, sub-column inner.  The first pass writes instead of adding (0.0 + -0.0
//                  is not -0.0), the last one divides by (double)(K * K) and, when asked, writes pixel_d2c of the result beside
//                  the doubles, one 32-bit store a pixel.  Pass 0 also copies sub-sample (0, 0) of its depth map: the map of an
//                  ssaa frame is the plain W x H frame's, not an average of 1 / distance with zeros for misses.
//
// Memory is that of a frame K times as wide, not K * K times as large.  The pass buffer and the accumulator belong to the context,
// only grow and are reused.
#include "ndt_ctx.hpp"
#include <limits.h>

namespace {

constexpr int FOLD_LANES = 256;
constexpr int FOLD_PIXELS = FOLD_LANES / 2;     // output pixels a workgroup folds: a lane owns two channels of one pixel

// pixel_d2c (image.h:36-39), as k_quantize has it
__device__ __forceinline__ unsigned int ssaa_d2c(double d)
{
    double m = (1.0 < d) ? 1.0 : d;
    m = (0.0 > m) ? 0.0 : m;
    return (unsigned int)(unsigned char)(sqrt(m) * 255);
}

// One workgroup folds FOLD_PIXELS output pixels of one row.  Their K sub-samples are FOLD_PIXELS * K * 32 contiguous bytes of the
// pass: the workgroup reads them with consecutive lanes on consecutive 16 bytes (K loads a lane, all in flight before the first
// is used) and parks them in LDS, where the lane that owns channels 2h, 2h + 1 of pixel i reads its K values in order.  In LDS
// a pixel's sub-samples start K 32-byte pixels after its neighbour's; for an even K the lane pairs of a ds_read_b128 group
// (pairs 0, 1, 6, 7, 10 .. 13 of a 32-lane half: 16 lanes on the 16 slots of 16 bytes of a bank row) would fall on K * p mod 8 --
// two to eight of them on one slot.  One pixel of padding after every K makes the stride odd, and K' * p mod 8 a permutation.
// The accumulator is read and written by consecutive lanes on consecutive 16 bytes as it lies.
template <int K>
__global__ void __launch_bounds__(FOLD_LANES) k_ssaa_fold(const double2 *__restrict__ pass, double2 *acc, int width, int tiles_x,
                                                          int first, int last, unsigned int *rgba8,
                                                          const double *__restrict__ pass_depth, double *depth_out)
{
    constexpr int PAD = (K & 1) ? 0 : 1;
    constexpr int KP = K + PAD;
    __shared__ double2 tile[FOLD_PIXELS * KP * 2];
    const int tid = (int)threadIdx.x;
    const long long row = (long long)(blockIdx.x / (unsigned)tiles_x);
    const int i0 = (int)(blockIdx.x % (unsigned)tiles_x) * FOLD_PIXELS;
    const int n_pix = width - i0 < FOLD_PIXELS ? width - i0 : FOLD_PIXELS;
    const int n_units = n_pix * K * 2;                      // 16-byte units of the pass this workgroup takes
    const long long pixel0 = row * width + i0;              // the workgroup's first output pixel
    const double2 *src = pass + pixel0 * (2 * K);           // = (row * K * width + K * i0) * 2
    double2 v[K];
#pragma unroll
    for (int m = 0; m < K; ++m) {
        const int j = m * FOLD_LANES + tid;
        v[m] = make_double2(0.0, 0.0);
        if (j < n_units) v[m] = src[j];
    }
#pragma unroll
    for (int m = 0; m < K; ++m) {
        const int j = m * FOLD_LANES + tid;
        if (j < n_units) tile[j + 2 * PAD * ((j >> 1) / K)] = v[m];
    }
    __syncthreads();
    const int i = tid >> 1, h = tid & 1;
    const bool live = i < n_pix;
    unsigned int half8 = 0;
    if (live) {
        const double2 *s = tile + i * (KP * 2) + h;
        const long long at = (pixel0 + i) * 2 + h;
        double2 sum = s[0];
        if (!first) {
            const double2 before = acc[at];
            sum.x = before.x + sum.x;
            sum.y = before.y + sum.y;
        }
#pragma unroll
        for (int b = 1; b < K; ++b) {
            sum.x = sum.x + s[2 * b].x;
            sum.y = sum.y + s[2 * b].y;
        }
        if (last) {
            sum.x = sum.x / (double)(K * K);
            sum.y = sum.y / (double)(K * K);
            if (rgba8) half8 = ssaa_d2c(sum.x) | (ssaa_d2c(sum.y) << 8);
        }
        acc[at] = sum;
        if (first && depth_out && h == 0) depth_out[pixel0 + i] = pass_depth[(pixel0 + i) * K];
    }
    if (last && rgba8) {                                    // (uniform: every lane of the wavefront takes part in the exchange)
        const unsigned int other = (unsigned int)__shfl_xor((int)half8, 1, 64);
        if (live && h == 0) rgba8[pixel0 + i] = half8 | (other << 16);
    }
}

template <int K>
void launch_fold(hipStream_t s, unsigned grid, const void *pass, void *acc, int width, int tiles_x, int first, int last, void *rgba8,
                 const void *pass_depth, void *depth_out)
{
    hipLaunchKernelGGL(k_ssaa_fold<K>, dim3(grid), dim3(FOLD_LANES), 0, s, (const double2 *)pass, (double2 *)acc, width, tiles_x, first, last,
                       (unsigned int *)rgba8, (const double *)pass_depth, (double *)depth_out);
}

// one fold step, arguments checked by the callers; asynchronous on the context's stream
int fold(ndt_hip_ctx *ctx, const void *d_pass, void *d_acc, int width, int rows, int K, int a, void *d_rgba8, const void *d_pass_depth,
         void *d_depth_out)
{
    const int tiles_x = (width + FOLD_PIXELS - 1) / FOLD_PIXELS;
    const long long grid = (long long)tiles_x * rows;
    if (grid > INT_MAX) return fail(NDT_E_UNSUPPORTED, "supersampling: %d x %d pixels are more than one fold launch takes", width, rows);
    const int first = a == 0, last = a == K - 1;
    hipStream_t s = ctx->stream;
    switch (K) {
    case 1: launch_fold<1>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    case 2: launch_fold<2>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    case 3: launch_fold<3>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    case 4: launch_fold<4>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    case 5: launch_fold<5>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    case 6: launch_fold<6>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    case 7: launch_fold<7>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    default: launch_fold<8>(s, (unsigned)grid, d_pass, d_acc, width, tiles_x, first, last, d_rgba8, d_pass_depth, d_depth_out); break;
    }
    HIP_TRY(hipGetLastError());
    ++ctx->ssaa.launches;
    return NDT_OK;
}

// what every whole-frame call refuses, before any device work
int refuse(const char *who, const ndt_hip_ctx *ctx, const ndt_render_params *p, int K, const void *out)
{
    if (!ctx || !p || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (K < 1 || K > 8) return fail(NDT_E_INVALID, "%s: supersampling factor %d is outside 1 .. 8", who, K);
    if (p->recursive_aa) return fail(NDT_E_INVALID, "%s: supersampling is not combined with recursive_aa (-a): take one of the two", who);
    if (p->stereo == NDT_STEREO_HIDEF)
        return fail(NDT_E_INVALID, "%s: supersampling of a frame-packed image (NDT_STEREO_HIDEF): its 1080-line packing is not scalable", who);
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0) return fail(NDT_E_INVALID, "%s: bad geometry", who);
    if ((long long)K * p->width > INT32_MAX || (long long)K * p->height > INT32_MAX || (long long)K * p->row_step > INT32_MAX ||
        (long long)K * p->row_begin + K > INT32_MAX)
        return fail(NDT_E_INVALID, "%s: %d times %d x %d is beyond INT32_MAX", who, K, p->width, p->height);
    if (p->stereo == NDT_STEREO_SIDE_SIDE && (p->width & 1))
        return fail(NDT_E_INVALID, "%s: side by side at an odd width (%d): the halves would not line up with the large frame's", who, p->width);
    if (p->stereo == NDT_STEREO_OVER_UNDER && (p->height & 1))
        return fail(NDT_E_INVALID, "%s: over/under at an odd height (%d): the halves would not line up with the large frame's", who, p->height);
    return NDT_OK;
}

// The frame for checked arguments: doubles into d_rgba (16-byte aligned), the map into d_depth and the bytes into d_rgba8 when
// those are given.  Returns when the frame is complete.
int render_ssaa(ndt_hip_ctx *ctx, const ndt_render_params *p, int K, void *d_rgba, void *d_depth, void *d_rgba8, ndt_render_stats *stats)
{
    HIP_TRY(hipSetDevice(ctx->device));
    SsaaState &ss = ctx->ssaa;
    ss.launches = 0;
    ss.fold_ms = 0.0;
    ss.factor = K;
    const int rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    const size_t pixels = (size_t)rows * (size_t)p->width;
    ndt_render_stats total{};
    if (K == 1 || rows == 0) {
        // the plain frame (or no rows at all: the render call says what is wrong with the rest, or that nothing is)
        int rc = ndt_hip_render_depth_device(ctx, p, d_rgba, d_depth, &total);
        if (rc) return rc;
        if (d_rgba8 && pixels && (rc = ndt_hip_quantize_device(ctx, d_rgba, d_rgba8, (int64_t)pixels))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (stats) *stats = total;
        return NDT_OK;
    }
    const size_t pass_bytes = pixels * K * 4 * sizeof(double);
    int rc;
    if ((rc = ss.d_pass.reserve(pass_bytes + (d_depth ? pass_bytes / 4 : 0), ctx->stream, "ndt_hip_render_ssaa*"))) return rc;
    if (!ss.ev[0])
        for (hipEvent_t &e : ss.ev) HIP_TRY(hipEventCreate(&e));
    void *d_pass_depth = d_depth ? (void *)(ss.d_pass.as<char>() + pass_bytes) : nullptr;
    ndt_render_params q = *p;
    q.width = K * p->width;
    q.height = K * p->height;
    q.row_step = K * p->row_step;
    for (int a = 0; a < K; ++a) {
        // rows { K (b + k S) + a } of the large frame: as many as the shard has output rows
        q.row_begin = K * p->row_begin + a;
        ndt_render_stats one{};
        if ((rc = ndt_hip_render_depth_device(ctx, &q, ss.d_pass.p, a == 0 ? d_pass_depth : nullptr, &one))) return rc;
        add_stats(total, one);
        total.pixels_resampled += one.pixels_resampled;
        total.aa_samples += one.aa_samples;
        HIP_TRY(hipEventRecord(ss.ev[2 * a], ctx->stream));
        if ((rc = fold(ctx, ss.d_pass.p, d_rgba, p->width, rows, K, a, d_rgba8, d_pass_depth, d_depth))) return rc;
        HIP_TRY(hipEventRecord(ss.ev[2 * a + 1], ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int a = 0; a < K; ++a) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ss.ev[2 * a], ss.ev[2 * a + 1]));
        ss.fold_ms += ms;
    }
    if (stats) *stats = total;
    return NDT_OK;
}

// the frame into the context's own buffers, named by *v: ss.d_acc (doubles, the map behind them when wanted) and ss.d_rgba8
int render_ssaa_own(ndt_hip_ctx *ctx, const ndt_render_params *p, int K, bool want_depth, bool want_rgba8, ndt_render_stats *stats, FrameView *v)
{
    HIP_TRY(hipSetDevice(ctx->device));
    SsaaState &ss = ctx->ssaa;
    *v = FrameView{ nullptr, nullptr, nullptr, p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step) };
    const size_t pixels = v->pixels(), img_bytes = pixels * 4 * sizeof(double);
    int rc;
    if ((rc = ss.d_acc.reserve((img_bytes ? img_bytes : 32) + (want_depth ? img_bytes / 4 : 0), ctx->stream, "ndt_hip_render_ssaa*"))) return rc;
    if (want_rgba8 && (rc = ss.d_rgba8.reserve(pixels ? pixels * 4 : 4, ctx->stream, "ndt_hip_render_ssaa*"))) return rc;
    *v = FrameView{ ss.d_acc.p, want_depth ? ss.d_acc.as<char>() + img_bytes : nullptr, want_rgba8 ? ss.d_rgba8.p : nullptr, v->width, v->rows };
    return render_ssaa(ctx, p, K, ss.d_acc.p, (void *)v->d_depth, (void *)v->d_rgba8, stats);
}

} // namespace

void ndt_impl::free_ssaa(ndt_hip_ctx *ctx)
{
    SsaaState &ss = ctx->ssaa;
    ss.d_pass.release();
    ss.d_acc.release();
    ss.d_rgba8.release();
    ss.d_depth8.release();
    ss.d_rgba16.release();
    ss.d_grey16.release();
    for (hipEvent_t &e : ss.ev)
        if (e) (void)hipEventDestroy(e);
    ss = SsaaState();
}

extern "C" int ndt_hip_ssaa_fold_device(ndt_hip_ctx *ctx, const void *d_pass, void *d_acc, int32_t width_out, int32_t rows, int32_t K, int32_t a,
                                        void *d_rgba8)
{
    if (!ctx || !d_pass || !d_acc) return fail(NDT_E_INVALID, "ndt_hip_ssaa_fold_device: NULL argument");
    if (K < 1 || K > 8) return fail(NDT_E_INVALID, "ndt_hip_ssaa_fold_device: supersampling factor %d is outside 1 .. 8", K);
    if (a < 0 || a >= K) return fail(NDT_E_INVALID, "ndt_hip_ssaa_fold_device: sub-row %d of %d", a, K);
    if (width_out < 1 || rows < 1) return fail(NDT_E_INVALID, "ndt_hip_ssaa_fold_device: an accumulator of %d x %d pixels", width_out, rows);
    if ((long long)K * width_out > INT32_MAX) return fail(NDT_E_INVALID, "ndt_hip_ssaa_fold_device: %d times %d is beyond INT32_MAX", K, width_out);
    if (((uintptr_t)d_pass & 15u) != 0 || ((uintptr_t)d_acc & 15u) != 0 || ((uintptr_t)d_rgba8 & 3u) != 0)
        return fail(NDT_E_INVALID, "ndt_hip_ssaa_fold_device: the pass and the accumulator must be aligned to 16 bytes, the image to its 4-byte pixels");
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->ssaa.launches = 0;
    int rc = fold(ctx, d_pass, d_acc, width_out, rows, K, a, d_rgba8, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

extern "C" int ndt_hip_ssaa_launches(ndt_hip_ctx *ctx) { return ctx ? ctx->ssaa.launches : 0; }
extern "C" double ndt_hip_ssaa_ms(ndt_hip_ctx *ctx) { return ctx ? ctx->ssaa.fold_ms : 0.0; }

extern "C" int ndt_hip_render_ssaa_device(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, void *d_rgba, void *d_depth,
                                          ndt_render_stats *stats)
{
    int rc = refuse("ndt_hip_render_ssaa_device", ctx, p, K, d_rgba);
    if (rc) return rc;
    if (((uintptr_t)d_rgba & 15u) != 0 || ((uintptr_t)d_depth & 7u) != 0)
        return fail(NDT_E_INVALID, "ndt_hip_render_ssaa_device: the image must be aligned to 16 bytes, the map to its doubles");
    return render_ssaa(ctx, p, K, d_rgba, d_depth, nullptr, stats);
}

// The delivering entries (a shard without rows: the host-memory sinks have nothing to write, the file sinks refuse it)
extern "C" int ndt_hip_render_ssaa(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, double *rgba, double *depth, ndt_render_stats *stats)
{
    int rc = refuse("ndt_hip_render_ssaa", ctx, p, K, rgba);
    if (rc) return rc;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, depth != nullptr, false, stats, &v)) || v.rows == 0) return rc;
    return deliver_doubles(ctx, v, rgba, depth);
}

extern "C" int ndt_hip_render_ssaa_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *rgba8, ndt_render_stats *stats)
{
    int rc = refuse("ndt_hip_render_ssaa_rgba8", ctx, p, K, rgba8);
    if (rc) return rc;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, false, true, stats, &v)) || v.rows == 0) return rc;
    return deliver_rgba8(ctx, "ndt_hip_render_ssaa_rgba8", v, ctx->ssaa.d_rgba8, rgba8);
}

int ndt_impl::render_ssaa_rgba8_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, int K, ndt_render_stats *stats,
                                    const void **d_rgba8)
{
    int rc = refuse(who, ctx, p, K, d_rgba8);
    if (rc) return rc;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, false, true, stats, &v))) return rc;
    *d_rgba8 = v.d_rgba8;
    return NDT_OK;
}

extern "C" int ndt_hip_render_ssaa_png(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                                       ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_ssaa_png";
    int rc = refuse(who, ctx, p, K, png);
    if (rc) return rc;
    if ((rc = refuse_png(who, p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step), 4))) return rc;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, false, true, render_stats, &v))) return rc;
    return deliver_png(ctx, who, v, ctx->ssaa.d_rgba8, png, cap, stats);
}

extern "C" int ndt_hip_render_ssaa_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_jpeg_params *jp, uint8_t *jpg,
                                        int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_ssaa_jpeg";
    int rc = refuse(who, ctx, p, K, jpg);
    if (rc) return rc;
    if ((rc = refuse_jpeg(who, p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step), jp))) return rc;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, false, true, render_stats, &v))) return rc;
    return deliver_jpeg(ctx, who, v, ctx->ssaa.d_rgba8, jp, jpg, cap, stats);
}

extern "C" int ndt_hip_render_ssaa_rgba8_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *rgba8, uint8_t *depth8,
                                               double *range_out, ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_ssaa_rgba8_depth";
    int rc = refuse(who, ctx, p, K, rgba8);
    if (rc) return rc;
    if (!depth8) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (range_out) range_out[0] = range_out[1] = 0.0;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, true, true, stats, &v)) || v.rows == 0) return rc;
    return deliver_rgba8(ctx, who, v, ctx->ssaa.d_rgba8, rgba8, &ctx->ssaa.d_depth8, depth8, range_out);
}

// the 16-bit files: the finished accumulator through ndt_hip_quantize16_device (one launch behind the last fold, which is left as
// it is), the map of sub-sample (0, 0) through ndt_hip_depth_grey16_device
static int ssaa_png16(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap, uint8_t *depth_png,
                      int64_t depth_cap, ndt_png_stats *stats, double *range_out, ndt_render_stats *render_stats)
{
    int rc = refuse(who, ctx, p, K, png);
    if (rc) return rc;
    if ((rc = refuse_png(who, p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step), 8))) return rc;
    if (range_out) range_out[0] = range_out[1] = 0.0;
    FrameView v;
    if ((rc = render_ssaa_own(ctx, p, K, depth_png != nullptr, false, render_stats, &v))) return rc;
    return deliver_png16(ctx, who, v, ctx->ssaa.d_rgba16, ctx->ssaa.d_grey16, png, cap, depth_png, depth_cap, stats, range_out);
}

extern "C" int ndt_hip_render_ssaa_png16(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                                         ndt_render_stats *render_stats)
{
    return ssaa_png16("ndt_hip_render_ssaa_png16", ctx, p, K, png, cap, nullptr, 0, stats, nullptr, render_stats);
}

extern "C" int ndt_hip_render_ssaa_png16_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap,
                                               uint8_t *depth_png, int64_t depth_cap, ndt_png_stats *stats, double *range_out,
                                               ndt_render_stats *render_stats)
{
    if (!depth_png) return fail(NDT_E_INVALID, "ndt_hip_render_ssaa_png16_depth: NULL argument");
    if (stats) stats[0] = stats[1] = ndt_png_stats{};
    return ssaa_png16("ndt_hip_render_ssaa_png16_depth", ctx, p, K, png, cap, depth_png, depth_cap, stats, range_out, render_stats);
}
