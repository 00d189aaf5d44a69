// ndt_png.hip -- a frame's PNG file made on the device: ndt_hip_png_bound / ndt_hip_encode_png_device / ndt_hip_encode_png /
// ndt_hip_render_png, and their 16-bit twins ndt_hip_png16_bound / ndt_hip_encode_png16* / ndt_hip_render_png16.  The quantised
// image is in HBM already; what leaves the device is the finished file.
//
//   k_png_filter    one workgroup a scanline: filter 0 (None), 1 (Sub) or 2 (Up) by the smallest sum of |filtered byte as int8|
//                   (ties to the lower number; row 0 has zeros above it), then the filtered stream, written as aligned words
//   k_png_filter_wide<BPP>   the same for pixels of 8 bytes (16-bit RGBA) and 2 bytes (16-bit grey): the row as words, Sub
//                   against the bytes BPP to the left
//   k_png_deflate   one workgroup an independent 32 KiB chunk of that stream: distance-1 matches, a dynamic Huffman code of
//                   its own, the bits packed into an LDS image with ds_or; a chunk the code does not shrink is stored; every
//                   chunk but the last ends on a byte boundary (an empty stored block: 00 00 FF FF).  Its body is deflate_chunk
//                   of ndt_deflate.hpp, which the OpenEXR file's blocks (ndt_exr.hip) are compressed with too
//   k_png_assemble  one workgroup: the chunks' places (a scan of their byte counts), the Adler-32 of the whole stream folded from
//                   the chunks' pairs, signature / IHDR / IDAT header / Adler-32 / IEND
//   k_png_place     one workgroup a chunk: its bytes to their place in the file
//
// No kernel waits for another workgroup, every loop's trip count comes from the chunk size (or the image size in the filter and
// the assembler), and the only atomics are LDS atomics inside a workgroup.  The host reads the info record, then exactly the
// file's bytes, and sets the IDAT chunk's CRC-32 over what arrived; it never sees the uncompressed image.
#include "ndt_ctx.hpp"
#include "ndt_deflate.hpp"
#include <chrono>

namespace {

constexpr int PNG_FILE_HEAD = 8 + 25 + 8 + 2;   // signature, IHDR chunk, IDAT length + type, zlib header
constexpr int PNG_FILE_EXTRA = PNG_FILE_HEAD + 4 + 4 + 12;      // ... Adler-32, IDAT CRC, IEND chunk

struct PngInfo {
    long long png_bytes, idat_bytes;
    int chunks_stored, rows_filter[3];
    int pad[8];
};

__constant__ unsigned char png_signature[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
__constant__ unsigned char png_iend[12] = { 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82 };

// ------------------------------------------------------------------ the row filter

// per byte a - b mod 256
__device__ __forceinline__ unsigned bytes_sub(unsigned a, unsigned b)
{
    const unsigned h = 0x80808080u;
    return ((a | h) - (b & ~h)) ^ ((a ^ ~b) & h);
}
// sum over the word's bytes of |byte as int8|
__device__ __forceinline__ unsigned bytes_abs_sum(unsigned x)
{
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned b = (x >> (8 * k)) & 255u;
        s += b < 128u ? b : 256u - b;
    }
    return s;
}

// the filtered bytes of pixel x of a row as one word; pixel -1 ends in the row's filter byte, pixels from `width` on are zero
__device__ __forceinline__ unsigned filtered_pixel(const unsigned *cur, const unsigned *up, int width, int filter, int x)
{
    if (x < 0) return (unsigned)filter << 24;
    if (x >= width) return 0u;
    const unsigned p = cur[x];
    if (filter == 0) return p;
    if (filter == 1) return bytes_sub(p, x > 0 ? cur[x - 1] : 0u);
    return bytes_sub(p, up ? up[x] : 0u);
}

__global__ void __launch_bounds__(256) k_png_filter(const unsigned *__restrict__ image, unsigned char *out, unsigned char *row_filter,
                                                    int width, int rows)
{
    __shared__ unsigned long long wave_sum[4][3];
    __shared__ int chosen;
    const int row = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned *cur = image + (long long)row * width, *up = row > 0 ? cur - width : nullptr;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    for (int x = tid; x < width; x += 256) {
        const unsigned p = cur[x], l = x > 0 ? cur[x - 1] : 0u, u = up ? up[x] : 0u;
        s0 += bytes_abs_sum(p);
        s1 += bytes_abs_sum(bytes_sub(p, l));
        s2 += bytes_abs_sum(bytes_sub(p, u));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_down(s0, d, 64);
        s1 += __shfl_down(s1, d, 64);
        s2 += __shfl_down(s2, d, 64);
    }
    if (lane == 0) { wave_sum[wave][0] = s0; wave_sum[wave][1] = s1; wave_sum[wave][2] = s2; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long t[3];
        for (int f = 0; f < 3; ++f) t[f] = wave_sum[0][f] + wave_sum[1][f] + wave_sum[2][f] + wave_sum[3][f];
        int f = 0;
        unsigned long long best = t[0];
        if (t[1] < best) { best = t[1]; f = 1; }
        if (t[2] < best) f = 2;
        chosen = f;
        row_filter[row] = (unsigned char)f;
    }
    __syncthreads();
    const int filter = chosen;
    // the row is bytes [g0, g0 + stride) of the stream: whole aligned words from a0 on, single bytes before and after them
    const long long stride = 1 + 4LL * width, g0 = (long long)row * stride, a0 = (g0 + 3) & ~3LL;
    const long long n_words = (g0 + stride - a0) >> 2;      // stride >= 5 > a0 - g0
    unsigned *out32 = reinterpret_cast<unsigned *>(out);
    for (long long j = tid; j < n_words; j += 256) {
        const long long q = a0 + 4 * j - g0 - 1;            // the word's first byte is byte q & 3 of pixel q >> 2 (q = -1: the filter byte)
        const int xa = (int)(q >> 2), b = (int)(q & 3);
        const unsigned lo = filtered_pixel(cur, up, width, filter, xa);
        unsigned val = lo;
        if (b) val = (lo >> (8 * b)) | (filtered_pixel(cur, up, width, filter, xa + 1) << (32 - 8 * b));
        out32[(a0 >> 2) + j] = val;
    }
    if (tid < 6) {
        // up to 3 bytes before the first whole word and up to 3 after the last
        const long long head = a0 - g0, tail0 = head + 4 * n_words;
        const long long i = tid < 3 ? tid : tail0 + (tid - 3);
        if (tid < 3 ? i < head : i < stride) {
            const long long q = i - 1;
            const unsigned f = filtered_pixel(cur, up, width, filter, (int)(q >> 2));
            out[g0 + i] = (unsigned char)(f >> (8 * (int)(q & 3)));
        }
    }
}

// ------------------------------------------------------------------ the row filter for pixels of 2 and 8 bytes

// Word k of a row of n_bytes bytes; every word before the row is zero, and so is every byte from n_bytes on.  A row of 8-byte
// pixels is aligned to them; a row of 2-byte pixels to two bytes only, so its word is two 16-bit loads.
template <int BPP>
__device__ __forceinline__ unsigned row_word(const unsigned char *row, int n_bytes, int k)
{
    if (k < 0 || 4LL * k >= (long long)n_bytes) return 0u;
    if (BPP == 8) return reinterpret_cast<const unsigned *>(row)[k];
    const unsigned short *h = reinterpret_cast<const unsigned short *>(row);
    const unsigned lo = h[2 * k], hi = 4LL * k + 2 < (long long)n_bytes ? (unsigned)h[2 * k + 1] : 0u;
    return lo | (hi << 16);
}

// the row's bytes BPP to the left of word k's: two words back, or the other half of this word and of the one before
template <int BPP>
__device__ __forceinline__ unsigned left_word(const unsigned char *row, int n_bytes, int k, unsigned p)
{
    if (BPP == 8) return row_word<8>(row, n_bytes, k - 2);
    return (p << 16) | (row_word<2>(row, n_bytes, k - 1) >> 16);
}

// the mask of word k's bytes that are inside the row
__device__ __forceinline__ unsigned inside_mask(int n_bytes, int k)
{
    const long long left = (long long)n_bytes - 4LL * k;
    return left >= 4 ? 0xffffffffu : left <= 0 ? 0u : (1u << (8 * (int)left)) - 1u;
}

// the filtered bytes of word k of a row; word -1 ends in the row's filter byte, bytes from n_bytes on are zero
template <int BPP>
__device__ __forceinline__ unsigned filtered_word(const unsigned char *cur, const unsigned char *up, int n_bytes, int filter, int k)
{
    if (k < 0) return (unsigned)filter << 24;
    const unsigned p = row_word<BPP>(cur, n_bytes, k);
    if (filter == 0) return p;
    const unsigned other = filter == 1 ? left_word<BPP>(cur, n_bytes, k, p) : up ? row_word<BPP>(up, n_bytes, k) : 0u;
    return bytes_sub(p, other) & inside_mask(n_bytes, k);
}

// k_png_filter for BPP = 8 or 2 bytes a pixel: the same workgroup a row, the same three sums reduced the same way, the same
// aligned words with up to 3 head and tail bytes.  `image` is aligned to BPP.
template <int BPP>
__global__ void __launch_bounds__(256) k_png_filter_wide(const unsigned char *__restrict__ image, unsigned char *out, unsigned char *row_filter,
                                                         int width, int rows)
{
    static_assert(BPP == 2 || BPP == 8, "16-bit grey or 16-bit RGBA");
    __shared__ unsigned long long wave_sum[4][3];
    __shared__ int chosen;
    const int row = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_bytes = BPP * width, n_row_words = (int)(((long long)n_bytes + 3) >> 2);      // the stream is under 2^31 bytes
    const unsigned char *cur = image + (long long)row * n_bytes, *up = row > 0 ? cur - n_bytes : nullptr;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    for (int k = tid; k < n_row_words; k += 256) {
        const unsigned p = row_word<BPP>(cur, n_bytes, k), l = left_word<BPP>(cur, n_bytes, k, p);
        const unsigned u = up ? row_word<BPP>(up, n_bytes, k) : 0u, inside = inside_mask(n_bytes, k);
        s0 += bytes_abs_sum(p);
        s1 += bytes_abs_sum(bytes_sub(p, l) & inside);
        s2 += bytes_abs_sum(bytes_sub(p, u) & inside);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_down(s0, d, 64);
        s1 += __shfl_down(s1, d, 64);
        s2 += __shfl_down(s2, d, 64);
    }
    if (lane == 0) { wave_sum[wave][0] = s0; wave_sum[wave][1] = s1; wave_sum[wave][2] = s2; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long t[3];
        for (int f = 0; f < 3; ++f) t[f] = wave_sum[0][f] + wave_sum[1][f] + wave_sum[2][f] + wave_sum[3][f];
        int f = 0;
        unsigned long long best = t[0];
        if (t[1] < best) { best = t[1]; f = 1; }
        if (t[2] < best) f = 2;
        chosen = f;
        row_filter[row] = (unsigned char)f;
    }
    __syncthreads();
    const int filter = chosen;
    // the row is bytes [g0, g0 + stride) of the stream: whole aligned words from a0 on, single bytes before and after them
    const long long stride = 1 + (long long)n_bytes, g0 = (long long)row * stride, a0 = (g0 + 3) & ~3LL;
    const long long n_words = (g0 + stride - a0) >> 2;      // stride >= 3 >= a0 - g0
    unsigned *out32 = reinterpret_cast<unsigned *>(out);
    for (long long j = tid; j < n_words; j += 256) {
        const long long q = a0 + 4 * j - g0 - 1;            // the word's first byte is byte q & 3 of row word q >> 2 (q = -1: the filter byte)
        const int ka = (int)(q >> 2), b = (int)(q & 3);
        const unsigned lo = filtered_word<BPP>(cur, up, n_bytes, filter, ka);
        unsigned val = lo;
        if (b) val = (lo >> (8 * b)) | (filtered_word<BPP>(cur, up, n_bytes, filter, ka + 1) << (32 - 8 * b));
        out32[(a0 >> 2) + j] = val;
    }
    if (tid < 6) {
        // up to 3 bytes before the first whole word and up to 3 after the last
        const long long head = a0 - g0, tail0 = head + 4 * n_words;
        const long long i = tid < 3 ? tid : tail0 + (tid - 3);
        if ((tid < 3 ? i < head : true) && i < stride) {
            const long long q = i - 1;
            const unsigned f = filtered_word<BPP>(cur, up, n_bytes, filter, (int)(q >> 2));
            out[g0 + i] = (unsigned char)(f >> (8 * (int)(q & 3)));
        }
    }
}

// ------------------------------------------------------------------ the deflate (ndt_deflate.hpp): chunk k of the one stream

__global__ void __launch_bounds__(PNG_DEFLATE_LANES) k_png_deflate(const unsigned char *__restrict__ filtered, long long n_total,
                                                                   int n_chunks, unsigned char *slots, ChunkMeta *meta)
{
    const int chunk = (int)blockIdx.x;
    const long long base = (long long)chunk * PNG_CHUNK;
    const int n = (int)(n_total - base < PNG_CHUNK ? n_total - base : PNG_CHUNK);
    deflate_chunk<1>(filtered + base, n, chunk == n_chunks - 1, slots + (long long)chunk * PNG_SLOT, meta + chunk);
}

// ------------------------------------------------------------------ the file around the chunks

__device__ __forceinline__ void store_be32(unsigned char *p, unsigned v)
{
    p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

__global__ void __launch_bounds__(1024) k_png_assemble(const ChunkMeta *__restrict__ meta, int n_chunks, long long n_total,
                                                       const unsigned char *__restrict__ row_filter, int width, int rows,
                                                       int bit_depth, int colour_type, unsigned char *png, long long *offsets,
                                                       PngInfo *info)
{
    __shared__ long long wsum[16];
    __shared__ int filter_count[4];
    const int t = (int)threadIdx.x;
    if (t < 4) filter_count[t] = 0;
    const int per = (n_chunks + 1023) / 1024, c0 = t * per, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
    long long bytes = 0, s1 = 0, stored = 0;
    for (int c = c0; c < c1; ++c) {
        const ChunkMeta m = meta[c];
        bytes += m.bytes;
        s1 += m.s1;
        stored += m.stored;
    }
    long long all_bytes = 0, all_s1 = 0, all_stored = 0, all_s2 = 0;
    long long off = block_scan_excl<1>(bytes, 0ll, OpAdd(), wsum, &all_bytes);
    long long before = block_scan_excl<1>(s1, 0ll, OpAdd(), wsum, &all_s1);
    (void)block_scan_excl<1>(stored, 0ll, OpAdd(), wsum, &all_stored);
    // Adler-32 of the stream: s1 = 1 + sum of the chunks' s1; a chunk of n bytes entered with s1 = a adds n * a + its own s2 to s2
    long long s2 = 0;
    for (int c = c0; c < c1; ++c) {
        const ChunkMeta m = meta[c];
        const long long nc = n_total - (long long)c * PNG_CHUNK < PNG_CHUNK ? n_total - (long long)c * PNG_CHUNK : PNG_CHUNK;
        offsets[c] = off;
        s2 += (long long)m.s2 + nc * ((1 + before) % (long long)ADLER_MOD);
        off += m.bytes;
        before += m.s1;
    }
    (void)block_scan_excl<1>(s2 % (long long)ADLER_MOD, 0ll, OpAdd(), wsum, &all_s2);
    int mine[3] = { 0, 0, 0 };
    for (int r = t; r < rows; r += 1024) {
        const int f = row_filter[r];
        mine[0] += f == 0; mine[1] += f == 1; mine[2] += f == 2;
    }
    for (int f = 0; f < 3; ++f)
        if (mine[f]) atomicAdd(&filter_count[f], mine[f]);
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < 8; ++k) png[k] = png_signature[k];
        unsigned char *ihdr = png + 8;
        store_be32(ihdr, 13u);
        ihdr[4] = 'I'; ihdr[5] = 'H'; ihdr[6] = 'D'; ihdr[7] = 'R';
        store_be32(ihdr + 8, (unsigned)width);
        store_be32(ihdr + 12, (unsigned)rows);
        ihdr[16] = (unsigned char)bit_depth; ihdr[17] = (unsigned char)colour_type;     // 8 / 6 (RGBA), 16 / 6 or 16 / 0 (grey)
        ihdr[18] = 0; ihdr[19] = 0; ihdr[20] = 0;                                       // no interlace
        unsigned crc = 0xffffffffu;
        for (int k = 4; k < 21; ++k) {
            crc ^= ihdr[k];
            for (int b = 0; b < 8; ++b) crc = (crc & 1u) ? 0xedb88320u ^ (crc >> 1) : crc >> 1;
        }
        store_be32(ihdr + 21, crc ^ 0xffffffffu);
        const long long idat = 2 + all_bytes + 4;
        unsigned char *q = png + 33;
        store_be32(q, (unsigned)idat);
        q[4] = 'I'; q[5] = 'D'; q[6] = 'A'; q[7] = 'T';
        q[8] = 0x78; q[9] = 0x01;
        unsigned char *z = png + PNG_FILE_HEAD + all_bytes;
        const unsigned a = (unsigned)((1 + all_s1) % (long long)ADLER_MOD), b = (unsigned)(all_s2 % (long long)ADLER_MOD);
        store_be32(z, (b << 16) | a);
        store_be32(z + 4, 0u);          // the IDAT chunk's CRC-32: set by the host over the bytes that arrived
        for (int k = 0; k < 12; ++k) z[8 + k] = png_iend[k];
        info->png_bytes = PNG_FILE_EXTRA + all_bytes;
        info->idat_bytes = idat;
        info->chunks_stored = (int)all_stored;
        for (int f = 0; f < 3; ++f) info->rows_filter[f] = filter_count[f];
    }
}

__global__ void __launch_bounds__(256) k_png_place(const unsigned char *__restrict__ slots, const ChunkMeta *__restrict__ meta,
                                                   const long long *__restrict__ offsets, unsigned char *png)
{
    const int chunk = (int)blockIdx.x;
    const unsigned char *src = slots + (long long)chunk * PNG_SLOT;
    unsigned char *dst = png + PNG_FILE_HEAD + offsets[chunk];
    const int bytes = (int)meta[chunk].bytes;           // at most 5 + 32768
    for (int k = (int)threadIdx.x; k < bytes; k += 256) dst[k] = src[k];
}

// ------------------------------------------------------------------ host

// CRC-32 (the PNG polynomial), eight bytes a step
struct CrcTables {
    unsigned t[8][256];
    CrcTables()
    {
        for (unsigned n = 0; n < 256; ++n) {
            unsigned c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][n] = c;
        }
        for (unsigned n = 0; n < 256; ++n)
            for (int k = 1; k < 8; ++k) t[k][n] = t[0][t[k - 1][n] & 255u] ^ (t[k - 1][n] >> 8);
    }
};

// the filtered stream's length for pixels of bpp bytes, or -1 for a size the encoder does not take
long long stream_bytes(int32_t width, int32_t rows, int bpp = 4)
{
    if (width < 1 || rows < 1) return -1;
    const long long n = (1 + (long long)bpp * width) * (long long)rows;      // < 2^35 * 2^31
    return n > 0x7fffffffLL ? -1 : n;
}

// every chunk stored: 5 bytes a chunk on top of the stream
long long file_bound(long long n) { return PNG_FILE_EXTRA + n + 5 * ((n + PNG_CHUNK - 1) / PNG_CHUNK); }

// what the encoder is told about the image: bytes a pixel, and the IHDR's bit depth and colour type
struct PngFormat { int bpp, bit_depth, colour_type; };
constexpr PngFormat PNG_RGBA8 = { 4, 8, 6 }, PNG_RGBA16 = { 8, 16, 6 }, PNG_GREY16 = { 2, 16, 0 };

// channels 4 -> RGBA16, 1 -> GREY16, anything else -> nullptr
const PngFormat *format16(int32_t channels) { return channels == 4 ? &PNG_RGBA16 : channels == 1 ? &PNG_GREY16 : nullptr; }

// The file of width x rows pixels of format `f` at d_image (the context's device memory; arguments checked by the callers) made in
// ps.d_file: the 4 launches, then its info record in host memory.  `bound`: the largest file the size can give.
int make_file(ndt_hip_ctx *ctx, const char *who, const void *d_image, int32_t width, int32_t rows, const PngFormat &f, PngInfo &info,
              int &n_chunks, long long &bound)
{
    HIP_TRY(hipSetDevice(ctx->device));
    PngState &ps = ctx->png;
    const long long n = stream_bytes(width, rows, f.bpp);
    n_chunks = (int)((n + PNG_CHUNK - 1) / PNG_CHUNK);
    bound = file_bound(n);
    int rc;
    if ((rc = ps.d_filtered.reserve((size_t)n_chunks * PNG_CHUNK, ctx->stream, who))) return rc;
    if ((rc = ps.d_row_filter.reserve((size_t)rows, ctx->stream, who))) return rc;
    if ((rc = ps.d_slots.reserve((size_t)n_chunks * PNG_SLOT, ctx->stream, who))) return rc;
    if ((rc = ps.d_meta.reserve((size_t)n_chunks * sizeof(ChunkMeta), ctx->stream, who))) return rc;
    if ((rc = ps.d_offsets.reserve((size_t)n_chunks * sizeof(long long), ctx->stream, who))) return rc;
    if ((rc = ps.d_file.reserve((size_t)bound, ctx->stream, who))) return rc;
    if ((rc = ps.d_info.reserve(sizeof(PngInfo), ctx->stream, who))) return rc;
    if (!ps.h_info) HIP_TRY(hipHostMalloc(&ps.h_info, sizeof(PngInfo), hipHostMallocDefault));
    hipStream_t s = ctx->stream;
    if (f.bpp == 4)
        hipLaunchKernelGGL(k_png_filter, dim3((unsigned)rows), dim3(256), 0, s, (const unsigned *)d_image, ps.d_filtered.as<unsigned char>(),
                           ps.d_row_filter.as<unsigned char>(), (int)width, (int)rows);
    else if (f.bpp == 8)
        hipLaunchKernelGGL(k_png_filter_wide<8>, dim3((unsigned)rows), dim3(256), 0, s, (const unsigned char *)d_image,
                           ps.d_filtered.as<unsigned char>(), ps.d_row_filter.as<unsigned char>(), (int)width, (int)rows);
    else
        hipLaunchKernelGGL(k_png_filter_wide<2>, dim3((unsigned)rows), dim3(256), 0, s, (const unsigned char *)d_image,
                           ps.d_filtered.as<unsigned char>(), ps.d_row_filter.as<unsigned char>(), (int)width, (int)rows);
    hipLaunchKernelGGL(k_png_deflate, dim3((unsigned)n_chunks), dim3(PNG_DEFLATE_LANES), 0, s, ps.d_filtered.as<const unsigned char>(), n, n_chunks,
                       ps.d_slots.as<unsigned char>(), ps.d_meta.as<ChunkMeta>());
    hipLaunchKernelGGL(k_png_assemble, dim3(1), dim3(1024), 0, s, ps.d_meta.as<const ChunkMeta>(), n_chunks, n, ps.d_row_filter.as<const unsigned char>(),
                       (int)width, (int)rows, f.bit_depth, f.colour_type, ps.d_file.as<unsigned char>(), ps.d_offsets.as<long long>(),
                       ps.d_info.as<PngInfo>());
    hipLaunchKernelGGL(k_png_place, dim3((unsigned)n_chunks), dim3(256), 0, s, ps.d_slots.as<const unsigned char>(), ps.d_meta.as<const ChunkMeta>(),
                       ps.d_offsets.as<const long long>(), ps.d_file.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ps.h_info, ps.d_info.p, sizeof(PngInfo), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    info = *(const PngInfo *)ps.h_info;
    return NDT_OK;
}

// The file of width x rows pixels of format `f` at d_image (the context's device memory) in host memory: made by make_file,
// fetched, its IDAT chunk's CRC-32 set here; `who` names the entry point in errors.
int encode_device(ndt_hip_ctx *ctx, const char *who, const void *d_image, int32_t width, int32_t rows, const PngFormat &f, uint8_t *png,
                  int64_t cap, ndt_png_stats *stats)
{
    if (!ctx || !d_image || !png) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a %d x %d image", who, width, rows);
    int rc = refuse_png(who, width, rows, f.bpp);
    if (rc) return rc;
    if (cap < 0) return fail(NDT_E_INVALID, "%s: cap %lld", who, (long long)cap);
    if (((uintptr_t)d_image & (uintptr_t)(f.bpp - 1)) != 0) return fail(NDT_E_INVALID, "%s: the image is not aligned to its %d-byte pixels", who, f.bpp);
    const auto t0 = std::chrono::steady_clock::now();
    PngInfo info;
    int n_chunks = 0;
    long long bound = 0;
    if ((rc = make_file(ctx, who, d_image, width, rows, f, info, n_chunks, bound))) return rc;
    PngState &ps = ctx->png;
    hipStream_t s = ctx->stream;
    if (stats) {
        *stats = ndt_png_stats{};
        stats->png_bytes = info.png_bytes;
        stats->idat_bytes = info.idat_bytes;
        stats->chunks = n_chunks;
        stats->chunks_stored = info.chunks_stored;
        stats->launches = 4;
        for (int k = 0; k < 3; ++k) stats->rows_filter[k] = info.rows_filter[k];
    }
    if (info.png_bytes < PNG_FILE_EXTRA || info.png_bytes > bound)
        return fail(NDT_E_DEVICE, "%s: the device reports a file of %lld bytes (bound %lld)", who, info.png_bytes, bound);
    if (info.png_bytes > cap)
        return fail(NDT_E_NOMEM, "%s: the file is %lld bytes, the buffer %lld", who, info.png_bytes, (long long)cap);
    HIP_TRY(hipMemcpyAsync(png, ps.d_file.p, (size_t)info.png_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // the IDAT chunk's CRC-32 covers its type and data: bytes 37 .. 41 + idat_bytes of the file
    const unsigned crc = crc32_of(png + 37, (size_t)(4 + info.idat_bytes));
    uint8_t *q = png + 41 + info.idat_bytes;
    q[0] = (uint8_t)(crc >> 24); q[1] = (uint8_t)(crc >> 16); q[2] = (uint8_t)(crc >> 8); q[3] = (uint8_t)crc;
    if (stats) stats->encode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return NDT_OK;
}

// the image of width x rows pixels of format `f` from host memory into the context's upload buffer
int upload_image(ndt_hip_ctx *ctx, const char *who, const void *image, int32_t width, int32_t rows, const PngFormat &f)
{
    if (!ctx || !image) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a %d x %d image", who, width, rows);
    int rc = refuse_png(who, width, rows, f.bpp);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)width * (size_t)rows * (size_t)f.bpp;
    if ((rc = ctx->png.d_rgba8.reserve(bytes, ctx->stream, who))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->png.d_rgba8.p, image, bytes, hipMemcpyHostToDevice, ctx->stream));
    return NDT_OK;
}

} // namespace

unsigned ndt_impl::crc32_of(const unsigned char *p, size_t len)
{
    static const CrcTables tab;
    unsigned c = 0xffffffffu;
    while (len >= 8) {
        unsigned lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = tab.t[7][lo & 255u] ^ tab.t[6][(lo >> 8) & 255u] ^ tab.t[5][(lo >> 16) & 255u] ^ tab.t[4][lo >> 24] ^
            tab.t[3][hi & 255u] ^ tab.t[2][(hi >> 8) & 255u] ^ tab.t[1][(hi >> 16) & 255u] ^ tab.t[0][hi >> 24];
        p += 8;
        len -= 8;
    }
    while (len--) c = tab.t[0][(c ^ *p++) & 255u] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

int ndt_impl::png_file_device(ndt_hip_ctx *ctx, const char *who, const void *d_rgba8, int32_t width, int32_t rows, long long *zlib_bytes)
{
    static_assert(PNG_ZLIB_AT == PNG_FILE_HEAD - 2, "the zlib header follows the IDAT chunk's length and type");
    PngInfo info;
    int n_chunks = 0;
    long long bound = 0;
    int rc = make_file(ctx, who, d_rgba8, width, rows, PNG_RGBA8, info, n_chunks, bound);
    if (rc) return rc;
    if (info.png_bytes < PNG_FILE_EXTRA || info.png_bytes > bound || info.idat_bytes != info.png_bytes - (PNG_FILE_EXTRA - 6))
        return fail(NDT_E_DEVICE, "%s: the device reports a file of %lld bytes with a stream of %lld (bound %lld)", who, info.png_bytes,
                    info.idat_bytes, bound);
    *zlib_bytes = info.idat_bytes;
    return NDT_OK;
}

extern "C" int64_t ndt_hip_png_bound(int32_t width, int32_t rows)
{
    const long long n = stream_bytes(width, rows);
    if (n < 0) return NDT_E_INVALID;
    return file_bound(n);
}

extern "C" int64_t ndt_hip_png16_bound(int32_t width, int32_t rows, int32_t channels)
{
    const PngFormat *f = format16(channels);
    const long long n = f ? stream_bytes(width, rows, f->bpp) : -1;
    if (n < 0) return NDT_E_INVALID;
    return file_bound(n);
}

void ndt_impl::free_png(ndt_hip_ctx *ctx)
{
    PngState &ps = ctx->png;
    ps.d_rgba8.release();
    ps.d_rgba16.release();
    ps.d_filtered.release();
    ps.d_row_filter.release();
    ps.d_slots.release();
    ps.d_meta.release();
    ps.d_offsets.release();
    ps.d_file.release();
    ps.d_info.release();
    if (ps.h_info) (void)hipHostFree(ps.h_info);
    ps = PngState();
}

extern "C" int ndt_hip_encode_png_device(ndt_hip_ctx *ctx, const void *d_rgba8, int32_t width, int32_t rows, uint8_t *png, int64_t cap,
                                         ndt_png_stats *stats)
{
    return encode_device(ctx, "ndt_hip_encode_png", d_rgba8, width, rows, PNG_RGBA8, png, cap, stats);
}

extern "C" int ndt_hip_encode_png(ndt_hip_ctx *ctx, const uint8_t *rgba8, int32_t width, int32_t rows, uint8_t *png, int64_t cap,
                                  ndt_png_stats *stats)
{
    if (!png) return fail(NDT_E_INVALID, "ndt_hip_encode_png: NULL argument");
    int rc = upload_image(ctx, "ndt_hip_encode_png", rgba8, width, rows, PNG_RGBA8);
    if (rc) return rc;
    return ndt_hip_encode_png_device(ctx, ctx->png.d_rgba8.p, width, rows, png, cap, stats);
}

extern "C" int ndt_hip_encode_png16_device(ndt_hip_ctx *ctx, const void *d_samples, int32_t width, int32_t rows, int32_t channels, uint8_t *png,
                                           int64_t cap, ndt_png_stats *stats)
{
    const PngFormat *f = format16(channels);
    if (!f) return fail(NDT_E_INVALID, "ndt_hip_encode_png16: %d channels: a 16-bit file is grey (1) or RGBA (4)", channels);
    return encode_device(ctx, "ndt_hip_encode_png16", d_samples, width, rows, *f, png, cap, stats);
}

extern "C" int ndt_hip_encode_png16(ndt_hip_ctx *ctx, const uint8_t *samples, int32_t width, int32_t rows, int32_t channels, uint8_t *png,
                                    int64_t cap, ndt_png_stats *stats)
{
    const PngFormat *f = format16(channels);
    if (!f) return fail(NDT_E_INVALID, "ndt_hip_encode_png16: %d channels: a 16-bit file is grey (1) or RGBA (4)", channels);
    if (!png) return fail(NDT_E_INVALID, "ndt_hip_encode_png16: NULL argument");
    int rc = upload_image(ctx, "ndt_hip_encode_png16", samples, width, rows, *f);
    if (rc) return rc;
    return encode_device(ctx, "ndt_hip_encode_png16", ctx->png.d_rgba8.p, width, rows, *f, png, cap, stats);
}

extern "C" int ndt_hip_render_png(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                                  ndt_render_stats *render_stats)
{
    if (!ctx || !p || !png) return fail(NDT_E_INVALID, "ndt_hip_render_png: NULL argument");
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0) return fail(NDT_E_INVALID, "bad geometry");
    const int rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    int rc = refuse_png("ndt_hip_render_png", p->width, rows, 4);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ctx->png.d_rgba8.reserve((size_t)p->width * (size_t)rows * 4, ctx->stream, "ndt_hip_render_png"))) return rc;
    ndt_hip_ctx *one[1] = { ctx };
    if ((rc = ndt_hip_render_multi_device(one, 1, p, NDT_IMAGE_RGBA8, ctx->png.d_rgba8.p, render_stats))) return rc;
    return ndt_hip_encode_png_device(ctx, ctx->png.d_rgba8.p, p->width, rows, png, cap, stats);
}

extern "C" int ndt_hip_render_png16(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                                    ndt_render_stats *render_stats)
{
    if (!ctx || !p || !png) return fail(NDT_E_INVALID, "ndt_hip_render_png16: NULL argument");
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0)
        return fail(NDT_E_INVALID, "ndt_hip_render_png16: bad geometry: %d x %d, rows %d by %d", p->width, p->height, p->row_begin, p->row_step);
    int rc = refuse_png("ndt_hip_render_png16", p->width, ndt_hip_shard_rows(p->height, p->row_begin, p->row_step), 8);
    if (rc) return rc;
    // the frame in doubles where ndt_hip_render leaves it, its 16-bit samples beside the encoder's buffers (the encoder under this
    // entry's own name: not deliver_png16)
    FrameView v;
    if ((rc = render_plain_own(ctx, "ndt_hip_render_png16", p, false, render_stats, &v))) return rc;
    if ((rc = ctx->png.d_rgba16.reserve(v.pixels() * 8, ctx->stream, "ndt_hip_render_png16"))) return rc;
    if ((rc = ndt_hip_quantize16_device(ctx, v.d_rgba, ctx->png.d_rgba16.p, (int64_t)v.pixels()))) return rc;
    return encode_device(ctx, "ndt_hip_render_png16", ctx->png.d_rgba16.p, v.width, v.rows, PNG_RGBA16, png, cap, stats);
}
