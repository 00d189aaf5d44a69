// ndt_apng.hip -- a frame sequence as one animated PNG, the difference between consecutive frames found on the device:
// ndt_hip_apng_bound / ndt_hip_apng_begin / ndt_hip_apng_add_device / ndt_hip_apng_add / ndt_hip_render_apng_frame /
// ndt_hip_apng_end.  Frame 0 is the still file's image; a later frame is the bounding rectangle of the pixels that differ from
// the canvas (the previous frame, kept in the context's device memory), compressed by the still file's encoder run on the
// rectangle.  What leaves the device per frame is the plan record and the rectangle's zlib stream.
//
//   k_apng_rows    one workgroup a row: the frame's row against the canvas's as 32-bit pixels; per lane the first and the last
//                  changed column, the number changed and the number changed with an alpha other than 255, folded over the
//                  wavefront and then over the workgroup's wavefronts in LDS; one lane writes the row's 16-byte record
//   k_apng_plan    one workgroup: the row records folded into the plan record { x, y, w, h, blend, changed, translucent }.
//                  Nothing changed: the 1 x 1 pixel at (0, 0), blend SOURCE.  Blend OVER when no changed pixel is translucent
//   k_apng_crop    one workgroup a row of the rectangle: the compact w x h image the encoder takes (under OVER an unchanged
//                  pixel becomes 0: alpha 0 keeps the canvas, and runs of zeros cost the distance-1 matcher nothing), and the
//                  frame's pixels of the rectangle into the canvas -- outside it the canvas is the frame already
//   then ndt_png.hip's k_png_filter -> k_png_deflate -> k_png_assemble -> k_png_place on the compact image (png_file_device)
//
// No kernel waits for another workgroup, there are no global atomics, every trip count comes from the image size, and lanes
// work on consecutive addresses.  The host reads the plan record (it sizes the encoder's grids), then the zlib stream, and
// wraps it: the fcTL, the sequence number and the chunks' CRC-32s are host code.
#include "ndt_ctx.hpp"
#include <chrono>
#include <limits.h>

namespace {

struct RowRecord { int first, last, changed, translucent; };        // first = INT_MAX, last = -1: nothing changed in the row

struct PlanRecord {
    int x, y, w, h, blend, pad;
    long long changed, translucent;
};

constexpr int APNG_LANES = 256;
constexpr int BLEND_SOURCE = 0, BLEND_OVER = 1;
constexpr int CHUNK_EXTRA = 12;                 // a chunk's length, type and CRC-32
constexpr int FCTL_BODY = 26;
constexpr int FIRST_HEAD = 8 + (CHUNK_EXTRA + 13) + (CHUNK_EXTRA + 8);      // signature, IHDR, acTL

__global__ void __launch_bounds__(APNG_LANES) k_apng_rows(const unsigned *__restrict__ frame, const unsigned *__restrict__ canvas, int width,
                                                          RowRecord *records)
{
    __shared__ int wave_rec[APNG_LANES / 64][4];
    const int row = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned *cur = frame + (long long)row * width, *old = canvas + (long long)row * width;
    int first = INT_MAX, last = -1, changed = 0, translucent = 0;
    for (int x = tid; x < width; x += APNG_LANES) {
        const unsigned p = cur[x];
        if (p != old[x]) {
            first = x < first ? x : first;
            last = x;                           // a lane's columns ascend
            ++changed;
            translucent += (p >> 24) != 255u ? 1 : 0;       // alpha is the pixel's fourth byte
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int f = __shfl_down(first, d, 64), l = __shfl_down(last, d, 64);
        first = f < first ? f : first;
        last = l > last ? l : last;
        changed += __shfl_down(changed, d, 64);
        translucent += __shfl_down(translucent, d, 64);
    }
    if (lane == 0) { wave_rec[wave][0] = first; wave_rec[wave][1] = last; wave_rec[wave][2] = changed; wave_rec[wave][3] = translucent; }
    __syncthreads();
    if (tid == 0) {
        RowRecord r = { INT_MAX, -1, 0, 0 };
        for (int w = 0; w < APNG_LANES / 64; ++w) {
            r.first = wave_rec[w][0] < r.first ? wave_rec[w][0] : r.first;
            r.last = wave_rec[w][1] > r.last ? wave_rec[w][1] : r.last;
            r.changed += wave_rec[w][2];
            r.translucent += wave_rec[w][3];
        }
        records[row] = r;
    }
}

__global__ void __launch_bounds__(APNG_LANES) k_apng_plan(const RowRecord *__restrict__ records, int rows, PlanRecord *plan)
{
    __shared__ int wave_box[APNG_LANES / 64][4];
    __shared__ long long wave_count[APNG_LANES / 64][2];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    long long changed = 0, translucent = 0;
    for (int r = tid; r < rows; r += APNG_LANES) {
        const RowRecord rec = records[r];
        if (rec.changed > 0) {
            x0 = rec.first < x0 ? rec.first : x0;
            x1 = rec.last > x1 ? rec.last : x1;
            y0 = r < y0 ? r : y0;
            y1 = r;                             // a lane's rows ascend
            changed += rec.changed;
            translucent += rec.translucent;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_down(x0, d, 64), b = __shfl_down(x1, d, 64), c = __shfl_down(y0, d, 64), e = __shfl_down(y1, d, 64);
        x0 = a < x0 ? a : x0;
        x1 = b > x1 ? b : x1;
        y0 = c < y0 ? c : y0;
        y1 = e > y1 ? e : y1;
        changed += __shfl_down(changed, d, 64);
        translucent += __shfl_down(translucent, d, 64);
    }
    if (lane == 0) {
        wave_box[wave][0] = x0; wave_box[wave][1] = x1; wave_box[wave][2] = y0; wave_box[wave][3] = y1;
        wave_count[wave][0] = changed; wave_count[wave][1] = translucent;
    }
    __syncthreads();
    if (tid == 0) {
        x0 = INT_MAX; x1 = -1; y0 = INT_MAX; y1 = -1; changed = 0; translucent = 0;
        for (int w = 0; w < APNG_LANES / 64; ++w) {
            x0 = wave_box[w][0] < x0 ? wave_box[w][0] : x0;
            x1 = wave_box[w][1] > x1 ? wave_box[w][1] : x1;
            y0 = wave_box[w][2] < y0 ? wave_box[w][2] : y0;
            y1 = wave_box[w][3] > y1 ? wave_box[w][3] : y1;
            changed += wave_count[w][0];
            translucent += wave_count[w][1];
        }
        PlanRecord p;
        if (changed == 0) { p.x = 0; p.y = 0; p.w = 1; p.h = 1; p.blend = BLEND_SOURCE; }
        else { p.x = x0; p.y = y0; p.w = x1 - x0 + 1; p.h = y1 - y0 + 1; p.blend = translucent == 0 ? BLEND_OVER : BLEND_SOURCE; }
        p.pad = 0;
        p.changed = changed;
        p.translucent = translucent;
        *plan = p;
    }
}

// x, y, w, blend: the plan's, checked against the canvas by the host; the grid is the rectangle's h rows
__global__ void __launch_bounds__(APNG_LANES) k_apng_crop(const unsigned *__restrict__ frame, unsigned *canvas, int width, int x, int y, int w,
                                                          int blend, unsigned *compact)
{
    const int r = (int)blockIdx.x;
    const long long at = (long long)(y + r) * width + x;
    const unsigned *cur = frame + at;
    unsigned *old = canvas + at, *out = compact + (long long)r * w;
    for (int i = (int)threadIdx.x; i < w; i += APNG_LANES) {
        const unsigned p = cur[i];
        out[i] = (blend == BLEND_OVER && p == old[i]) ? 0u : p;
        old[i] = p;
    }
}

// ------------------------------------------------------------------ host

void put_be32(uint8_t *q, unsigned v) { q[0] = (uint8_t)(v >> 24); q[1] = (uint8_t)(v >> 16); q[2] = (uint8_t)(v >> 8); q[3] = (uint8_t)v; }
void put_be16(uint8_t *q, unsigned v) { q[0] = (uint8_t)(v >> 8); q[1] = (uint8_t)v; }

// a chunk whose `len` body bytes stand at q + 8 already: its length, type and CRC-32 around them; returns the chunk's end
uint8_t *wrap_chunk(uint8_t *q, const char *type, size_t len)
{
    put_be32(q, (unsigned)len);
    memcpy(q + 4, type, 4);
    put_be32(q + 8 + len, crc32_of(q + 4, 4 + len));
    return q + CHUNK_EXTRA + len;
}

// ends the session with the error `rc` the caller has set the text of
int drop(ndt_hip_ctx *ctx, int rc)
{
    ctx->apng.open = false;
    return rc;
}

// what every `add` refuses before any device work; the frame itself is checked by the caller
int refuse_add(const char *who, ndt_hip_ctx *ctx, const void *out, int64_t cap)
{
    if (!ctx || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (!ctx->apng.open) return fail(NDT_E_INVALID, "%s: no session open: call ndt_hip_apng_begin first", who);
    if (cap < 0) return drop(ctx, fail(NDT_E_INVALID, "%s: cap %lld", who, (long long)cap));
    if (ctx->apng.next_frame >= ctx->apng.n_frames)
        return drop(ctx, fail(NDT_E_INVALID, "%s: the session was opened for %d frames and has them all", who, ctx->apng.n_frames));
    return NDT_OK;
}

// The session's next frame from d_frame (the context's device memory, aligned to 4, arguments checked by the callers): the bytes
// to append into `out`.  An error closes the session.
int add_frame(ndt_hip_ctx *ctx, const char *who, const void *d_frame, uint8_t *out, int64_t cap, ndt_apng_stats *stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    ApngState &as = ctx->apng;
    const int W = as.width, R = as.rows, index = as.next_frame;
    const size_t image_bytes = (size_t)W * (size_t)R * 4;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return drop(ctx, fail(NDT_E_DEVICE, "%s: hipSetDevice: %s", who, hipGetErrorString(e)));
    hipStream_t s = ctx->stream;
    int rc;
    PlanRecord plan = { 0, 0, W, R, BLEND_SOURCE, 0, 0, 0 };
    const void *d_image = d_frame;
    int launches = 4;
    if (index == 0) {
        // the canvas has no contents worth keeping before frame 0: the one place its buffer may grow
        if ((rc = as.d_canvas.reserve(image_bytes, s, who))) return drop(ctx, rc);
        e = hipMemcpyAsync(as.d_canvas.p, d_frame, image_bytes, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return drop(ctx, fail(NDT_E_DEVICE, "%s: the copy into the canvas: %s", who, hipGetErrorString(e)));
    } else {
        if (as.d_canvas.bytes < image_bytes) return drop(ctx, fail(NDT_E_DEVICE, "%s: the session has no canvas", who));
        if ((rc = as.d_rows.reserve((size_t)R * sizeof(RowRecord), s, who))) return drop(ctx, rc);
        if ((rc = as.d_plan.reserve(sizeof(PlanRecord), s, who))) return drop(ctx, rc);
        if ((rc = as.d_crop.reserve(image_bytes, s, who))) return drop(ctx, rc);
        if (!as.h_plan && (e = hipHostMalloc(&as.h_plan, sizeof(PlanRecord), hipHostMallocDefault)) != hipSuccess)
            return drop(ctx, fail(NDT_E_NOMEM, "%s: hipHostMalloc: %s", who, hipGetErrorString(e)));
        hipLaunchKernelGGL(k_apng_rows, dim3((unsigned)R), dim3(APNG_LANES), 0, s, (const unsigned *)d_frame, as.d_canvas.as<const unsigned>(), W,
                           as.d_rows.as<RowRecord>());
        hipLaunchKernelGGL(k_apng_plan, dim3(1), dim3(APNG_LANES), 0, s, as.d_rows.as<const RowRecord>(), R, as.d_plan.as<PlanRecord>());
        if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpyAsync(as.h_plan, as.d_plan.p, sizeof(PlanRecord), hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess)
            return drop(ctx, fail(NDT_E_DEVICE, "%s: the frame's plan: %s", who, hipGetErrorString(e)));
        plan = *(const PlanRecord *)as.h_plan;
        // the record sizes a grid and places stores: nothing is launched on one that does not lie inside the canvas
        if (plan.x < 0 || plan.y < 0 || plan.w < 1 || plan.h < 1 || plan.x > W - plan.w || plan.y > R - plan.h ||
            (plan.blend != BLEND_SOURCE && plan.blend != BLEND_OVER))
            return drop(ctx, fail(NDT_E_DEVICE, "%s: the device plans a rectangle of %d x %d at %d,%d (blend %d) on a canvas of %d x %d", who, plan.w,
                                  plan.h, plan.x, plan.y, plan.blend, W, R));
        hipLaunchKernelGGL(k_apng_crop, dim3((unsigned)plan.h), dim3(APNG_LANES), 0, s, (const unsigned *)d_frame, as.d_canvas.as<unsigned>(), W, plan.x,
                           plan.y, plan.w, plan.blend, as.d_crop.as<unsigned>());
        if ((e = hipGetLastError()) != hipSuccess) return drop(ctx, fail(NDT_E_DEVICE, "%s: k_apng_crop: %s", who, hipGetErrorString(e)));
        d_image = as.d_crop.p;
        launches = 7;
    }
    long long zlib_bytes = 0;
    if ((rc = png_file_device(ctx, who, d_image, plan.w, plan.h, &zlib_bytes))) return drop(ctx, rc);
    // frame 0: signature, IHDR, acTL, fcTL, IDAT(stream); later: fcTL, fdAT(sequence number, stream)
    const long long head = index == 0 ? FIRST_HEAD + (CHUNK_EXTRA + FCTL_BODY) + 8 : (CHUNK_EXTRA + FCTL_BODY) + 8 + 4;
    const long long total = head + zlib_bytes + 4;
    if (stats) {
        *stats = ndt_apng_stats{};
        stats->frame = index;
        stats->bytes = total;
        stats->zlib_bytes = zlib_bytes;
        stats->x = plan.x; stats->y = plan.y; stats->w = plan.w; stats->h = plan.h;
        stats->blend = plan.blend;
        stats->changed = plan.changed;
        stats->translucent = plan.translucent;
        stats->launches = launches;
    }
    if (total > cap) return drop(ctx, fail(NDT_E_NOMEM, "%s: frame %d appends %lld bytes, the buffer holds %lld", who, index, total, (long long)cap));
    if ((e = hipMemcpyAsync(out + head, ctx->png.d_file.as<const unsigned char>() + PNG_ZLIB_AT, (size_t)zlib_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return drop(ctx, fail(NDT_E_DEVICE, "%s: the copy of the zlib stream: %s", who, hipGetErrorString(e)));
    uint8_t *q = out;
    if (index == 0) {
        static const uint8_t signature[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
        memcpy(q, signature, 8);
        q += 8;
        put_be32(q + 8, (unsigned)W);
        put_be32(q + 12, (unsigned)R);
        q[16] = 8; q[17] = 6; q[18] = 0; q[19] = 0; q[20] = 0;         // 8 bits, RGBA, deflate, adaptive filters, no interlace
        q = wrap_chunk(q, "IHDR", 13);
        put_be32(q + 8, (unsigned)as.n_frames);
        put_be32(q + 12, (unsigned)as.n_plays);
        q = wrap_chunk(q, "acTL", 8);
    }
    put_be32(q + 8, as.seq++);
    put_be32(q + 12, (unsigned)plan.w);
    put_be32(q + 16, (unsigned)plan.h);
    put_be32(q + 20, (unsigned)plan.x);
    put_be32(q + 24, (unsigned)plan.y);
    put_be16(q + 28, (unsigned)as.delay_num);
    put_be16(q + 30, (unsigned)as.delay_den);
    q[32] = 0;                                  // dispose NONE
    q[33] = (uint8_t)plan.blend;
    q = wrap_chunk(q, "fcTL", FCTL_BODY);
    if (index == 0) q = wrap_chunk(q, "IDAT", (size_t)zlib_bytes);
    else {
        put_be32(q + 8, as.seq++);
        q = wrap_chunk(q, "fdAT", 4 + (size_t)zlib_bytes);
    }
    if (q - out != total) return drop(ctx, fail(NDT_E_DEVICE, "%s: frame %d wrote %lld bytes of %lld", who, index, (long long)(q - out), total));
    ++as.next_frame;
    if (stats) stats->encode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return NDT_OK;
}

} // namespace

void ndt_impl::free_apng(ndt_hip_ctx *ctx)
{
    ApngState &as = ctx->apng;
    as.d_canvas.release();
    as.d_frame.release();
    as.d_crop.release();
    as.d_rows.release();
    as.d_plan.release();
    if (as.h_plan) (void)hipHostFree(as.h_plan);
    as = ApngState();
}

extern "C" int64_t ndt_hip_apng_bound(int32_t width, int32_t rows)
{
    // frame 0 is the largest: the still file without its IEND, with an acTL and an fcTL; a later frame's rectangle is no larger
    // than the canvas and carries a sequence number
    const int64_t still = ndt_hip_png_bound(width, rows);
    return still < 0 ? still : still + (FIRST_HEAD + (CHUNK_EXTRA + FCTL_BODY) + 4);
}

extern "C" int ndt_hip_apng_begin(ndt_hip_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, int32_t delay_num, int32_t delay_den,
                                  int32_t n_plays)
{
    if (!ctx) return fail(NDT_E_INVALID, "ndt_hip_apng_begin: NULL argument");
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "ndt_hip_apng_begin: a canvas of %d x %d pixels", width, rows);
    if (int rc = refuse_png("ndt_hip_apng_begin", width, rows, 4)) return rc;
    if (n_frames < 1) return fail(NDT_E_INVALID, "ndt_hip_apng_begin: n_frames %d: an animation has at least one frame", n_frames);
    if (delay_den < 1) return fail(NDT_E_INVALID, "ndt_hip_apng_begin: delay_den %d: the delay's denominator is at least 1", delay_den);
    if (delay_num < 0 || delay_num > 65535 || delay_den > 65535)
        return fail(NDT_E_INVALID, "ndt_hip_apng_begin: a delay of %d / %d: both are 16-bit fields (at most 65535)", delay_num, delay_den);
    if (n_plays < 0) return fail(NDT_E_INVALID, "ndt_hip_apng_begin: n_plays %d (0: for ever)", n_plays);
    ApngState &as = ctx->apng;
    as.open = true;
    as.width = width; as.rows = rows; as.n_frames = n_frames;
    as.delay_num = delay_num; as.delay_den = delay_den; as.n_plays = n_plays;
    as.next_frame = 0;
    as.seq = 0;
    return NDT_OK;
}

extern "C" int ndt_hip_apng_add_device(ndt_hip_ctx *ctx, const void *d_rgba8, uint8_t *out, int64_t cap, ndt_apng_stats *stats)
{
    int rc = refuse_add("ndt_hip_apng_add_device", ctx, out, cap);
    if (rc) return rc;
    if (!d_rgba8) return drop(ctx, fail(NDT_E_INVALID, "ndt_hip_apng_add_device: NULL argument"));
    if (((uintptr_t)d_rgba8 & 3u) != 0)
        return drop(ctx, fail(NDT_E_INVALID, "ndt_hip_apng_add_device: the image is not aligned to its 4-byte pixels"));
    return add_frame(ctx, "ndt_hip_apng_add_device", d_rgba8, out, cap, stats);
}

extern "C" int ndt_hip_apng_add(ndt_hip_ctx *ctx, const uint8_t *rgba8, uint8_t *out, int64_t cap, ndt_apng_stats *stats)
{
    int rc = refuse_add("ndt_hip_apng_add", ctx, out, cap);
    if (rc) return rc;
    if (!rgba8) return drop(ctx, fail(NDT_E_INVALID, "ndt_hip_apng_add: NULL argument"));
    ApngState &as = ctx->apng;
    const size_t bytes = (size_t)as.width * (size_t)as.rows * 4;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return drop(ctx, fail(NDT_E_DEVICE, "ndt_hip_apng_add: hipSetDevice: %s", hipGetErrorString(e)));
    if ((rc = as.d_frame.reserve(bytes, ctx->stream, "ndt_hip_apng_add"))) return drop(ctx, rc);
    if ((e = hipMemcpyAsync(as.d_frame.p, rgba8, bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
        return drop(ctx, fail(NDT_E_DEVICE, "ndt_hip_apng_add: the upload: %s", hipGetErrorString(e)));
    return add_frame(ctx, "ndt_hip_apng_add", as.d_frame.p, out, cap, stats);
}

extern "C" int ndt_hip_render_apng_frame(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t ssaa, uint8_t *out, int64_t cap,
                                         ndt_apng_stats *stats, ndt_render_stats *render_stats)
{
    static const char who[] = "ndt_hip_render_apng_frame";
    int rc = refuse_add(who, ctx, out, cap);
    if (rc) return rc;
    if (!p) return drop(ctx, fail(NDT_E_INVALID, "%s: NULL argument", who));
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0)
        return drop(ctx, fail(NDT_E_INVALID, "%s: bad geometry: %d x %d, rows %d by %d", who, p->width, p->height, p->row_begin, p->row_step));
    ApngState &as = ctx->apng;
    const int rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    if (p->width != as.width || rows != as.rows)
        return drop(ctx, fail(NDT_E_INVALID, "%s: the shard is %d x %d pixels, the session's canvas %d x %d", who, p->width, rows, as.width, as.rows));
    const void *d_image = nullptr;
    if (ssaa == 1) {
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return drop(ctx, fail(NDT_E_DEVICE, "%s: hipSetDevice: %s", who, hipGetErrorString(e)));
        if ((rc = as.d_frame.reserve((size_t)as.width * (size_t)as.rows * 4, ctx->stream, who))) return drop(ctx, rc);
        ndt_hip_ctx *one[1] = { ctx };
        if ((rc = ndt_hip_render_multi_device(one, 1, p, NDT_IMAGE_RGBA8, as.d_frame.p, render_stats))) return drop(ctx, rc);
        d_image = as.d_frame.p;
    } else if ((rc = render_ssaa_rgba8_own(ctx, who, p, ssaa, render_stats, &d_image)))      // (says what is wrong with 0, 9, ...)
        return drop(ctx, rc);
    return add_frame(ctx, who, d_image, out, cap, stats);
}

extern "C" int ndt_hip_apng_end(ndt_hip_ctx *ctx, uint8_t *out, int64_t cap, int64_t *bytes)
{
    if (!ctx || !out || !bytes) return fail(NDT_E_INVALID, "ndt_hip_apng_end: NULL argument");
    ApngState &as = ctx->apng;
    if (!as.open) return fail(NDT_E_INVALID, "ndt_hip_apng_end: no session open: call ndt_hip_apng_begin first");
    if (as.next_frame < as.n_frames)
        return fail(NDT_E_INVALID, "ndt_hip_apng_end: the session was opened for %d frames and has %d", as.n_frames, as.next_frame);
    *bytes = CHUNK_EXTRA;
    if (cap < CHUNK_EXTRA) return fail(NDT_E_NOMEM, "ndt_hip_apng_end: IEND is %d bytes, the buffer holds %lld", CHUNK_EXTRA, (long long)cap);
    (void)wrap_chunk(out, "IEND", 0);
    as.open = false;
    return NDT_OK;
}
