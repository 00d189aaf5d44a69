// ndt_depth.hip -- the depth map of `-z` finished on the device: what the driver does to the map render_image fills before it
// saves it (dbl_image_normalize, image.c:1025-1065: stretch to 0 .. 1; then pixel_d2c on a grey image), in two launches.
//
//   k_depth_range    every workgroup reduces its share of the map to one {lo, hi, bad} record
//   k_depth_finish   every workgroup folds the records itself (no third launch, nobody waits for anybody), then normalises and
//                    quantises its share of the map: one 32-bit store a pixel (g, g, g, 255), or -- SIXTEEN -- one 16-bit grey
//                    sample a lane in a PNG file's byte order, two lanes' samples in one 32-bit store
//
// The host loop compares `x < lo` and `x > hi` starting from element 0.  For a map without NaN that is the minimum and the
// maximum, whatever the order (signed zeros compare equal: which zero's sign the range carries is the fold order's, and no byte
// depends on it).  A map with a NaN or an infinity is refused: the host loop's answer would depend on where the NaN sits.
#include "ndt_ctx.hpp"
#include <chrono>

namespace {

constexpr int DEPTH_RANGE_LANES = 512;      // k_depth_range: one workgroup of eight wavefronts a CU
constexpr int DEPTH_MAX_RECORDS = 256;      // ... of at most this many workgroups: k_depth_finish folds one record a lane
constexpr int DEPTH_FINISH_LANES = 256;
constexpr int DEPTH_FINISH_GROUPS = 2048;
constexpr int DEPTH_UNROLL = 4;             // loads in flight a lane

struct DepthRecord {
    double lo, hi;
    long long bad;          // index of a NaN / infinity of the share (the lowest), or -1
    long long pad;
};

__device__ __forceinline__ void fold(double &lo, double &hi, long long &bad, double lo2, double hi2, long long bad2)
{
    if (lo2 < lo) lo = lo2;
    if (hi2 > hi) hi = hi2;
    if (bad2 >= 0 && (bad < 0 || bad2 < bad)) bad = bad2;
}

// the fold over a wavefront (six butterfly steps: every lane ends with the result), then over the workgroup through LDS;
// every lane of the workgroup calls it and returns the workgroup's record
template <int LANES>
__device__ __forceinline__ DepthRecord block_fold(double lo, double hi, long long bad)
{
    __shared__ DepthRecord part[LANES / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        fold(lo, hi, bad, __shfl_xor(lo, d, 64), __shfl_xor(hi, d, 64), __shfl_xor(bad, d, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = DepthRecord{ lo, hi, bad, 0 };
    __syncthreads();
    DepthRecord r = part[0];
#pragma unroll
    for (int w = 1; w < LANES / 64; ++w) fold(r.lo, r.hi, r.bad, part[w].lo, part[w].hi, part[w].bad);
    return r;
}

__global__ void __launch_bounds__(DEPTH_RANGE_LANES) k_depth_range(const double *__restrict__ depth, long long n, DepthRecord *records)
{
    const long long stride = (long long)gridDim.x * DEPTH_RANGE_LANES;
    const long long first = (long long)blockIdx.x * DEPTH_RANGE_LANES + threadIdx.x;
    // the trip count is the map size's alone: ceil(n / (stride * unroll)) for every lane, the tail guarded per element
    const long long trips = (n + stride * DEPTH_UNROLL - 1) / (stride * DEPTH_UNROLL);
    double lo = INFINITY, hi = -INFINITY;
    long long bad = -1;
    for (long long t = 0; t < trips; ++t) {
        double x[DEPTH_UNROLL];
        const long long at = first + t * stride * DEPTH_UNROLL;
#pragma unroll
        for (int u = 0; u < DEPTH_UNROLL; ++u) x[u] = at + u * stride < n ? depth[at + u * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < DEPTH_UNROLL; ++u) {
            const long long i = at + u * stride;
            if (i < n) {
                if (x[u] < lo) lo = x[u];
                if (x[u] > hi) hi = x[u];
                if (!(fabs(x[u]) < INFINITY) && bad < 0) bad = i;     // (a lane's indices ascend: its first is its lowest)
            }
        }
    }
    const DepthRecord r = block_fold<DEPTH_RANGE_LANES>(lo, hi, bad);
    if (threadIdx.x == 0) records[blockIdx.x] = r;
}

// pixel_d2c (image.h:36-39), as k_quantize has it
__device__ __forceinline__ unsigned int depth_d2c(double d)
{
    double m = (1.0 < d) ? 1.0 : d;
    m = (0.0 > m) ? 0.0 : m;
    return (unsigned int)(unsigned char)(sqrt(m) * 255);
}

// `out`: n 4-byte pixels, or -- SIXTEEN -- n 2-byte samples from a 4-byte aligned address
template <bool SIXTEEN>
__global__ void __launch_bounds__(DEPTH_FINISH_LANES) k_depth_finish(const double *__restrict__ depth, long long n,
                                                                     const DepthRecord *__restrict__ records, int n_records,
                                                                     void *out, DepthRecord *result)
{
    double lo = INFINITY, hi = -INFINITY;
    long long bad = -1;
    if ((int)threadIdx.x < n_records) {             // n_records <= DEPTH_MAX_RECORDS == the workgroup's lanes
        const DepthRecord r = records[threadIdx.x];
        lo = r.lo; hi = r.hi; bad = r.bad;
    }
    const DepthRecord all = block_fold<DEPTH_FINISH_LANES>(lo, hi, bad);
    if (blockIdx.x == 0 && threadIdx.x == 0) *result = all;
    if (all.bad >= 0) return;                       // refused: no pixel is written
    lo = all.lo; hi = all.hi;
    const bool spread = hi > lo;
    const double width = hi - lo;
    const long long stride = (long long)gridDim.x * DEPTH_FINISH_LANES;
    const long long first = (long long)blockIdx.x * DEPTH_FINISH_LANES + threadIdx.x;
    const long long trips = (n + stride * DEPTH_UNROLL - 1) / (stride * DEPTH_UNROLL);
    for (long long t = 0; t < trips; ++t) {
        double x[DEPTH_UNROLL];
        const long long at = first + t * stride * DEPTH_UNROLL;
#pragma unroll
        for (int u = 0; u < DEPTH_UNROLL; ++u) x[u] = at + u * stride < n ? depth[at + u * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < DEPTH_UNROLL; ++u) {
            const long long i = at + u * stride;
            if (SIXTEEN) {
                // every lane of the wavefront is here (the trip count is the map size's alone) and pixel i is even where the
                // lane is (the stride is even): lane 2k takes lane 2k + 1's sample and stores the two as one word
                const unsigned int v16 = q16_file_order(spread ? (x[u] - lo) / width : 0.0);
                const unsigned int next = __shfl_down(v16, 1, 64);
                if ((i & 1) == 0) {
                    if (i + 1 < n) reinterpret_cast<unsigned int *>(out)[i >> 1] = v16 | (next << 16);
                    else if (i < n) reinterpret_cast<unsigned short *>(out)[i] = (unsigned short)v16;       // the last of an odd n
                }
            } else if (i < n) {
                const double v = spread ? (x[u] - lo) / width : 0.0;
                const unsigned int v8 = depth_d2c(v);
                reinterpret_cast<unsigned int *>(out)[i] = v8 | (v8 << 8) | (v8 << 16) | (255u << 24);      // depth_d2c(1.0) = 255: the alpha
            }
        }
    }
}

// the two launches over a map of n_pixels doubles; `who` names the entry point in errors
int finish_map(ndt_hip_ctx *ctx, const char *who, bool sixteen, const void *d_depth, int64_t n_pixels, void *d_out, double *range_out)
{
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(ctx->device));
    DepthState &ds = ctx->depth;
    ds.launches = 0;
    ds.finish_ms = 0.0;
    int rc;
    // the records of the largest map there is, and behind them the record the host reads
    if ((rc = ds.d_records.reserve((size_t)(DEPTH_MAX_RECORDS + 1) * sizeof(DepthRecord), ctx->stream, who))) return rc;
    if (!ds.h_result) HIP_TRY(hipHostMalloc(&ds.h_result, sizeof(DepthRecord), hipHostMallocDefault));
    DepthRecord *records = ds.d_records.as<DepthRecord>(), *result = records + DEPTH_MAX_RECORDS;
    const long long n = n_pixels;
    const long long want_records = (n + DEPTH_RANGE_LANES * DEPTH_UNROLL - 1) / (DEPTH_RANGE_LANES * DEPTH_UNROLL);
    const int n_records = (int)(want_records < DEPTH_MAX_RECORDS ? want_records : DEPTH_MAX_RECORDS);
    const long long want_groups = (n + DEPTH_FINISH_LANES * DEPTH_UNROLL - 1) / (DEPTH_FINISH_LANES * DEPTH_UNROLL);
    const int n_groups = (int)(want_groups < DEPTH_FINISH_GROUPS ? want_groups : DEPTH_FINISH_GROUPS);
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_depth_range, dim3((unsigned)n_records), dim3(DEPTH_RANGE_LANES), 0, s, (const double *)d_depth, n, records);
    if (sixteen)
        hipLaunchKernelGGL(k_depth_finish<true>, dim3((unsigned)n_groups), dim3(DEPTH_FINISH_LANES), 0, s, (const double *)d_depth, n,
                           (const DepthRecord *)records, n_records, d_out, result);
    else
        hipLaunchKernelGGL(k_depth_finish<false>, dim3((unsigned)n_groups), dim3(DEPTH_FINISH_LANES), 0, s, (const double *)d_depth, n,
                           (const DepthRecord *)records, n_records, d_out, result);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ds.h_result, result, sizeof(DepthRecord), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ds.launches = 2;
    ds.finish_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const DepthRecord r = *(const DepthRecord *)ds.h_result;
    if (r.bad >= 0)
        return fail(NDT_E_UNSUPPORTED, "%s: the depth map holds a NaN or an infinity (pixel %lld): there is no range to stretch", who, r.bad);
    if (range_out) {
        range_out[0] = r.lo;
        range_out[1] = r.hi;
    }
    return NDT_OK;
}

} // namespace

void ndt_impl::free_depth(ndt_hip_ctx *ctx)
{
    DepthState &ds = ctx->depth;
    ds.d_records.release();
    ds.d_rgba8.release();
    ds.d_depth8.release();
    ds.d_rgba16.release();
    ds.d_grey16.release();
    if (ds.h_result) (void)hipHostFree(ds.h_result);
    ds = DepthState();
}

extern "C" int ndt_hip_depth_rgba8_device(ndt_hip_ctx *ctx, const void *d_depth, int64_t n_pixels, void *d_rgba8, double *range_out)
{
    if (!ctx || !d_depth || !d_rgba8) return fail(NDT_E_INVALID, "ndt_hip_depth_rgba8_device: NULL argument");
    if (n_pixels < 1) return fail(NDT_E_INVALID, "ndt_hip_depth_rgba8_device: a map of %lld pixels", (long long)n_pixels);
    if (((uintptr_t)d_depth & 7u) != 0 || ((uintptr_t)d_rgba8 & 3u) != 0)
        return fail(NDT_E_INVALID, "ndt_hip_depth_rgba8_device: the map is not aligned to its doubles, or the image not to its 4-byte pixels");
    return finish_map(ctx, "ndt_hip_depth_rgba8_device", false, d_depth, n_pixels, d_rgba8, range_out);
}

extern "C" int ndt_hip_depth_grey16_device(ndt_hip_ctx *ctx, const void *d_depth, int64_t n_pixels, void *d_grey16, double *range_out)
{
    if (!ctx || !d_depth || !d_grey16) return fail(NDT_E_INVALID, "ndt_hip_depth_grey16_device: NULL argument");
    if (n_pixels < 1) return fail(NDT_E_INVALID, "ndt_hip_depth_grey16_device: a map of %lld pixels", (long long)n_pixels);
    if (((uintptr_t)d_depth & 7u) != 0 || ((uintptr_t)d_grey16 & 3u) != 0)
        return fail(NDT_E_INVALID, "ndt_hip_depth_grey16_device: the map is not aligned to its doubles, or the samples not to 4 bytes");
    return finish_map(ctx, "ndt_hip_depth_grey16_device", true, d_depth, n_pixels, d_grey16, range_out);
}

extern "C" int ndt_hip_depth_launches(ndt_hip_ctx *ctx) { return ctx ? ctx->depth.launches : 0; }
extern "C" double ndt_hip_depth_ms(ndt_hip_ctx *ctx) { return ctx ? ctx->depth.finish_ms : 0.0; }

static const char WHO[] = "ndt_hip_render_*_depth";     // below: the plain frame and its map into ctx->d_out, then a tail of ndt_render.hip

extern "C" int ndt_hip_render_rgba8_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *rgba8, uint8_t *depth8, double *range_out,
                                          ndt_render_stats *stats)
{
    if (!ctx || !p || !rgba8 || !depth8) return fail(NDT_E_INVALID, "ndt_hip_render_rgba8_depth: NULL argument");
    if (range_out) range_out[0] = range_out[1] = 0.0;
    FrameView v;
    const int rc = render_plain_own(ctx, WHO, p, true, stats, &v);
    if (rc || v.rows == 0) return rc;
    return deliver_rgba8(ctx, WHO, v, ctx->depth.d_rgba8, rgba8, &ctx->depth.d_depth8, depth8, range_out);
}

extern "C" int ndt_hip_render_png_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, uint8_t *depth_png,
                                        int64_t depth_cap, uint8_t *depth8, ndt_png_stats *stats, double *range_out,
                                        ndt_render_stats *render_stats)
{
    if (!ctx || !p || !png) return fail(NDT_E_INVALID, "ndt_hip_render_png_depth: NULL argument");
    if ((depth_png != nullptr) == (depth8 != nullptr))
        return fail(NDT_E_INVALID, "ndt_hip_render_png_depth: the map goes to depth_png or to depth8: one of the two");
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0) return fail(NDT_E_INVALID, "bad geometry");
    int rc = refuse_png("ndt_hip_render_png_depth", p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step), 4);
    if (rc) return rc;
    if (stats) stats[0] = stats[1] = ndt_png_stats{};
    if (range_out) range_out[0] = range_out[1] = 0.0;
    FrameView v;
    if ((rc = render_plain_own(ctx, WHO, p, true, render_stats, &v))) return rc;
    return deliver_png(ctx, WHO, v, ctx->depth.d_rgba8, png, cap, stats, &ctx->depth.d_depth8, depth_png, depth_cap, depth8, range_out);
}

extern "C" int ndt_hip_render_png16_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, uint8_t *depth_png,
                                          int64_t depth_cap, ndt_png_stats *stats, double *range_out, ndt_render_stats *render_stats)
{
    if (!ctx || !p || !png || !depth_png) return fail(NDT_E_INVALID, "ndt_hip_render_png16_depth: NULL argument");
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0)
        return fail(NDT_E_INVALID, "ndt_hip_render_png16_depth: bad geometry: %d x %d, rows %d by %d", p->width, p->height, p->row_begin, p->row_step);
    int rc = refuse_png("ndt_hip_render_png16_depth", p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step), 8);
    if (rc) return rc;
    if (stats) stats[0] = stats[1] = ndt_png_stats{};
    if (range_out) range_out[0] = range_out[1] = 0.0;
    FrameView v;
    if ((rc = render_plain_own(ctx, WHO, p, true, render_stats, &v))) return rc;
    return deliver_png16(ctx, WHO, v, ctx->depth.d_rgba16, ctx->depth.d_grey16, png, cap, depth_png, depth_cap, stats, range_out);
}
