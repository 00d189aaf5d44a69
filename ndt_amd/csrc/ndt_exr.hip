// ndt_exr.hip -- a frame's OpenEXR file made on the device: ndt_hip_exr_bound / ndt_hip_encode_exr_device / ndt_hip_encode_exr /
// ndt_hip_render_exr / ndt_hip_render_ssaa_exr, and their *_features twins.  The frame's doubles are in HBM; what leaves the
// device is the finished file: a single-part scanline file, channels A B G R (HALF or FLOAT) and, with a depth map, Z (FLOAT), ZIP compression (16 scanlines a
// block, each block a zlib stream of its own), linear light: no clamp to 0 .. 1 and no square root.
//
//   k_exr_pack<SRC>    the doubles (and the map) of a block as the bytes the format compresses: byte planes (the even bytes of the
//                      block's raw bytes, then the odd ones), then the delta predictor -- every output byte is a function of two
//                      source samples, so there is no intermediate image.  Written as aligned words; each block starts on a
//                      32 KiB chunk boundary, so that the deflate's whole-chunk loads stay inside the buffer
//   k_exr_deflate      deflate_chunk of ndt_deflate.hpp (the PNG's deflate): one workgroup a chunk of a block.  Its matches are at
//                      distance 2, not the PNG's 1: the two byte planes give the bytes of equal float samples a period of 2, which
//                      a distance of 1 never matches (a flat float image came out at 28 % of its raw bytes, and comes out under
//                      1 %), and a run of equal bytes -- flat half samples -- is a distance-2 run as well
//   k_exr_assemble     one workgroup: per block the stream's length, its Adler-32 folded from the chunks' pairs and the raw-fallback
//                      decision (a stream that is not shorter than the raw bytes: the block holds those, as the format rules), a
//                      scan of the block sizes, the header, the offset table and the blocks' headers
//   k_exr_place<SRC>   one workgroup a chunk: its compressed bytes -- or, for a fallback block, the raw bytes made from the
//                      doubles again -- to their place in the file
//
// With feature channels (ndt_hip_encode_exr_features_device / ndt_hip_render_exr_features / ndt_hip_render_ssaa_exr_features) the
// samples come from a channel table in device memory (ExrChannels: per channel its name, pixel type, source, stride, element type
// and conversion).  k_exr_pack and k_exr_place are templates over where a raw byte comes from: PlainSource<HALF>, the four
// interleaved colour doubles and the optional map -- the instantiations the plain file had before the table existed, and still
// has: same registers, no scratch (profiles/exr_features_on_device.txt) --, and ListSource, which reads the table.  k_exr_assemble
// takes the table for the header; k_exr_deflate and deflate_chunk<2> need only the sizes.
//
// No kernel waits for another workgroup, every loop's trip count comes from a size, and the only atomics are the deflate's LDS
// atomics.  The host reads the info record, then exactly the file's bytes.
#include "ndt_ctx.hpp"
#include "ndt_deflate.hpp"
#include <chrono>

namespace {

constexpr int EXR_LINES = 16;           // scanlines a block of ZIP compression
constexpr int EXR_UINT = 0, EXR_HALF = 1, EXR_FLOAT = 2;        // the format's pixelType
constexpr int EXR_MAX_CHANNELS = 4 + 1 + 1 + 1 + 2 * NDT_MAX_DIMS;  // A B G R, AO, Z, id, N.* and P.*
constexpr int EXR_ALL_FEATURES = NDT_FEATURE_ID | NDT_FEATURE_POSITION | NDT_FEATURE_NORMAL;

// how a source element becomes a sample: a double to binary16, a double to float, an int32's bits as they are
enum { EXR_TO_HALF = 0, EXR_TO_FLOAT = 1, EXR_AS_UINT = 2 };

// One channel of a file with a channel list, in the file's order.  Pixel i's element is src[i * stride].
struct ExrChannel {
    const void *src;
    int stride;
    int is_int;                         // the element type: 0 double, 1 int32
    int conv;                           // EXR_TO_HALF / EXR_TO_FLOAT / EXR_AS_UINT
    int pixel_type;                     // the format's
    int first_unit, bytes;              // of one pixel: the sample bytes of the channels before it in a scanline; its own (2 or 4)
    char name[8];                       // zero-terminated
};
// ... and the list: in device memory (ExrState::d_channels).  unit_channel[u]: the channel that byte u * width of a scanline is in
struct ExrChannels {
    int n, units;
    unsigned char unit_channel[4 * EXR_MAX_CHANNELS];
    ExrChannel ch[EXR_MAX_CHANNELS];
};

// what the kernels are told about the file: every quantity fits an int because the raw bytes do
struct ExrLayout {
    int width, rows, n_ch;              // channels: 4, or 5 with Z; with a channel table, its entries
    int pixel_type;                     // of A B G R
    int line_bytes, colour_bytes;       // a scanline's raw bytes; those of its colour channels (the plain file's: 0 with a table)
    int n_blocks, cpb, n_chunks;        // blocks; chunks of a full block; chunks of the file (the last block may have fewer)
    int header_bytes;
    long long raw_bytes;
};

struct ExrBlock { long long data_off; int raw, pad; };      // where the block's data stands in the file; 1: the raw fallback

struct ExrInfo {
    long long file_bytes, raw_bytes;
    int blocks, blocks_raw;
    int pad[10];
};

__host__ __device__ inline int exr_put(unsigned char *p, int at, const void *src, int n)
{
    if (p)
        for (int k = 0; k < n; ++k) p[at + k] = ((const unsigned char *)src)[k];
    return at + n;
}
__host__ __device__ inline int exr_put32(unsigned char *p, int at, unsigned v)
{
    if (p) { p[at] = (unsigned char)v; p[at + 1] = (unsigned char)(v >> 8); p[at + 2] = (unsigned char)(v >> 16); p[at + 3] = (unsigned char)(v >> 24); }
    return at + 4;
}
// an attribute's name, type and size (both strings with their terminating zero)
__host__ __device__ inline int exr_attr(unsigned char *p, int at, const char *name, int name_len, const char *type, int type_len, int size)
{
    at = exr_put(p, at, name, name_len + 1);
    at = exr_put(p, at, type, type_len + 1);
    return exr_put32(p, at, (unsigned)size);
}

// what follows the channel list in a header: its closing zero, the other attributes, the header's closing zero
__host__ __device__ inline int exr_header_rest(unsigned char *p, int at, int width, int rows)
{
    const unsigned one = 0x3f800000u;   // 1.0f
    const unsigned char zip[1] = { 3 }, zero[1] = { 0 };
    at = exr_put(p, at, zero, 1);
    at = exr_attr(p, at, "compression", 11, "compression", 11, 1);
    at = exr_put(p, at, zip, 1);
    for (int k = 0; k < 2; ++k) {
        at = k == 0 ? exr_attr(p, at, "dataWindow", 10, "box2i", 5, 16) : exr_attr(p, at, "displayWindow", 13, "box2i", 5, 16);
        at = exr_put32(p, at, 0u);
        at = exr_put32(p, at, 0u);
        at = exr_put32(p, at, (unsigned)(width - 1));
        at = exr_put32(p, at, (unsigned)(rows - 1));
    }
    at = exr_attr(p, at, "lineOrder", 9, "lineOrder", 9, 1);
    at = exr_put(p, at, zero, 1);
    at = exr_attr(p, at, "pixelAspectRatio", 16, "float", 5, 4);
    at = exr_put32(p, at, one);
    at = exr_attr(p, at, "screenWindowCenter", 18, "v2f", 3, 8);
    at = exr_put32(p, at, 0u);
    at = exr_put32(p, at, 0u);
    at = exr_attr(p, at, "screenWindowWidth", 17, "float", 5, 4);
    at = exr_put32(p, at, one);
    return exr_put(p, at, zero, 1);
}

// The header -- magic, version, the attributes, the closing zero -- at p (nullptr: nothing is written); returns its length.
// The one definition: the host takes the length from it, k_exr_assemble the bytes.
__host__ __device__ inline int exr_header(unsigned char *p, int width, int rows, int n_ch, int pixel_type)
{
    int at = exr_put32(p, 0, 0x01312f76u);
    at = exr_put32(p, at, 2u);
    at = exr_attr(p, at, "channels", 8, "chlist", 6, 18 * n_ch + 1);
    const char names[5] = { 'A', 'B', 'G', 'R', 'Z' };
    for (int c = 0; c < n_ch; ++c) {
        const unsigned char name[2] = { (unsigned char)names[c], 0 };
        at = exr_put(p, at, name, 2);
        at = exr_put32(p, at, c == 4 ? (unsigned)EXR_FLOAT : (unsigned)pixel_type);
        at = exr_put32(p, at, 0u);      // pLinear and three reserved bytes
        at = exr_put32(p, at, 1u);
        at = exr_put32(p, at, 1u);
    }
    return exr_header_rest(p, at, width, rows);
}

// ... of a file with a channel list: the table's names and pixel types, in its order
__host__ __device__ inline int exr_header_list(unsigned char *p, int width, int rows, const ExrChannels *C)
{
    int at = exr_put32(p, 0, 0x01312f76u);
    at = exr_put32(p, at, 2u);
    int list = 1;
    for (int c = 0; c < C->n; ++c) {
        int len = 0;
        while (C->ch[c].name[len]) ++len;
        list += len + 1 + 16;
    }
    at = exr_attr(p, at, "channels", 8, "chlist", 6, list);
    for (int c = 0; c < C->n; ++c) {
        int len = 0;
        while (C->ch[c].name[len]) ++len;
        at = exr_put(p, at, C->ch[c].name, len + 1);
        at = exr_put32(p, at, (unsigned)C->ch[c].pixel_type);
        at = exr_put32(p, at, 0u);      // pLinear and three reserved bytes
        at = exr_put32(p, at, 1u);
        at = exr_put32(p, at, 1u);
    }
    return exr_header_rest(p, at, width, rows);
}

// ------------------------------------------------------------------ samples

// The double rounded directly to binary16, to nearest even, after the clamp to +-65504: on the bits, because the device has no
// double -> half conversion and rounding to float first rounds twice (1 + 2^-11 + 2^-30 is a tie as a float).  NaN: 0x7e00.
__device__ __forceinline__ unsigned half_bits(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned sign = (unsigned)(u >> 48) & 0x8000u;
    const unsigned long long a = u & 0x7fffffffffffffffull;
    if (a > 0x7ff0000000000000ull) return 0x7e00u;
    if (a >= 0x40effc0000000000ull) return sign | 0x7bffu;     // 65504 and beyond, the infinities included
    const int e = (int)(a >> 52) - 1023;
    if (e < -25) return sign;                                   // under half of the smallest denormal (the double's own denormals too)
    const unsigned long long m = (a & 0x000fffffffffffffull) | 0x0010000000000000ull;
    const int shift = e >= -14 ? 42 : 42 + (-14 - e);           // 43 .. 53 for a denormal result
    const unsigned long long rem = m & ((1ull << shift) - 1ull), tie = 1ull << (shift - 1);
    unsigned q = (unsigned)(m >> shift);
    q += (rem > tie || (rem == tie && (q & 1u))) ? 1u : 0u;
    // normal: q is 1024 .. 2048, and 2048 carries into the exponent; denormal: q is 0 .. 1024, and 1024 is the smallest normal
    return e >= -14 ? sign | (((unsigned)(e + 15) << 10) + (q - 1024u)) : sign | q;
}

// Where the raw bytes of a block come from.  byte(L, block, r): raw byte r of block `block`: per scanline, per channel in list
// order, `width` samples, little-endian.
// The plain file (A B G R Z): four interleaved colour doubles and an optional map
template <bool HALF>
struct PlainSource {
    const double *__restrict__ rgba, *__restrict__ depth;
    __device__ __forceinline__ unsigned byte(const ExrLayout &L, int block, int r) const
    {
        constexpr int BS = HALF ? 2 : 4;
        const int line = r / L.line_bytes, q = r - line * L.line_bytes;
        const long long row = (long long)EXR_LINES * block + line;
        unsigned bits;
        int b;
        if (q < L.colour_bytes) {
            const int wb = L.width * BS, c = q / wb, rem = q - c * wb, x = rem / BS;
            b = rem - x * BS;
            const double v = rgba[(row * L.width + x) * 4 + (3 - c)];      // the framebuffer is R G B A
            bits = HALF ? half_bits(v) : __float_as_uint((float)v);
        } else {
            const int rem = q - L.colour_bytes;
            b = rem & 3;
            bits = __float_as_uint((float)depth[row * L.width + (rem >> 2)]);
        }
        return (bits >> (8 * b)) & 255u;
    }
};
// A file with a channel list: the table says where every channel's samples are and what they become
struct ListSource {
    const ExrChannels *__restrict__ C;
    __device__ __forceinline__ unsigned byte(const ExrLayout &L, int block, int r) const
    {
        const int line = r / L.line_bytes, q = r - line * L.line_bytes;
        const long long row = (long long)EXR_LINES * block + line;
        const ExrChannel &ch = C->ch[C->unit_channel[q / L.width]];
        const int rem = q - ch.first_unit * L.width, x = ch.bytes == 2 ? rem >> 1 : rem >> 2, b = rem & (ch.bytes - 1);
        const long long at = (row * L.width + x) * ch.stride;
        unsigned bits;
        if (ch.is_int) {
            bits = (unsigned)((const int *)ch.src)[at];
        } else {
            const double v = ((const double *)ch.src)[at];
            bits = ch.conv == EXR_TO_HALF ? half_bits(v) : __float_as_uint((float)v);
        }
        return (bits >> (8 * b)) & 255u;
    }
};

__device__ __forceinline__ int block_bytes(const ExrLayout &L, int block)
{
    const int left = L.rows - EXR_LINES * block;
    return (left < EXR_LINES ? left : EXR_LINES) * L.line_bytes;
}

// ------------------------------------------------------------------ the block's bytes as the format compresses them

// blockIdx.y: the block; the workgroups of a row share its words
template <class SRC>
__global__ void __launch_bounds__(256) k_exr_pack(ExrLayout L, SRC src, unsigned *packed)
{
    const int block = (int)blockIdx.y, n = block_bytes(L, block), half = (n + 1) >> 1, n_words = (n + 3) >> 2;
    unsigned *out = packed + (long long)block * L.cpb * (PNG_CHUNK / 4);
    for (int wd = (int)(blockIdx.x * 256 + threadIdx.x); wd < n_words; wd += (int)gridDim.x * 256) {
        const int i0 = 4 * wd;
        // T[i]: the even raw bytes, then the odd ones
        unsigned before = 0u, val = 0u;
        if (i0 > 0) {
            const int i = i0 - 1;
            before = src.byte(L, block, i < half ? 2 * i : 2 * (i - half) + 1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k;
            if (i < n) {
                const unsigned cur = src.byte(L, block, i < half ? 2 * i : 2 * (i - half) + 1);
                val |= (i == 0 ? cur : (cur - before + 128u) & 255u) << (8 * k);
                before = cur;
            }
        }
        out[wd] = val;      // bytes from n on are zero: the buffer is whole chunks long
    }
}

// ------------------------------------------------------------------ the deflate: chunk c of block b is workgroup b * cpb + c

__global__ void __launch_bounds__(PNG_DEFLATE_LANES) k_exr_deflate(ExrLayout L, const unsigned char *__restrict__ packed, unsigned char *slots,
                                                                   ChunkMeta *meta)
{
    const int idx = (int)blockIdx.x, block = idx / L.cpb, c = idx - block * L.cpb;
    const int left = block_bytes(L, block) - c * PNG_CHUNK;         // >= 1: the grid ends with the last block's last chunk
    deflate_chunk<2>(packed + (long long)idx * PNG_CHUNK, left < PNG_CHUNK ? left : PNG_CHUNK, left <= PNG_CHUNK, slots + (long long)idx * PNG_SLOT,
                  meta + idx);
}

// ------------------------------------------------------------------ the file around the blocks

__device__ __forceinline__ void store_le32(unsigned char *p, unsigned v)
{
    p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24);
}

// block b's zlib stream from its chunks' records: its length (header and Adler-32 included) and its Adler-32.  s1 = 1 + the sum
// of the chunks' s1; a chunk of n bytes entered with s1 = a adds n * a + its own s2 to s2 (the fold of k_png_assemble)
__device__ __forceinline__ long long block_stream(const ExrLayout &L, const ChunkMeta *__restrict__ meta, int b, unsigned &adler)
{
    const int n = block_bytes(L, b), n_c = (n + PNG_CHUNK - 1) / PNG_CHUNK;
    long long bytes = 2 + 4, s1 = 0, s2 = 0;
    for (int c = 0; c < n_c; ++c) {
        const ChunkMeta m = meta[b * L.cpb + c];
        const long long nc = n - c * PNG_CHUNK < PNG_CHUNK ? n - c * PNG_CHUNK : PNG_CHUNK;
        bytes += m.bytes;
        s2 += (long long)m.s2 + nc * ((1 + s1) % (long long)ADLER_MOD);
        s1 += m.s1;
    }
    adler = ((unsigned)(s2 % (long long)ADLER_MOD) << 16) | (unsigned)((1 + s1) % (long long)ADLER_MOD);
    return bytes;
}

// (chans: the channel table of a file with feature channels, or nullptr: the plain file's fixed list)
__global__ void __launch_bounds__(1024) k_exr_assemble(ExrLayout L, const ChunkMeta *__restrict__ meta, unsigned char *file, long long *offsets,
                                                       ExrBlock *blocks, ExrInfo *info, const ExrChannels *chans)
{
    __shared__ long long wsum[16];
    const int t = (int)threadIdx.x;
    const int per = (L.n_blocks + 1023) / 1024, b0 = t * per < L.n_blocks ? t * per : L.n_blocks, b1 = b0 + per < L.n_blocks ? b0 + per : L.n_blocks;
    long long size = 0, raws = 0;
    for (int b = b0; b < b1; ++b) {
        unsigned adler;
        const long long stream = block_stream(L, meta, b, adler), n = block_bytes(L, b);
        size += 8 + (stream < n ? stream : n);
        raws += stream < n ? 0 : 1;
    }
    long long all_size = 0, all_raw = 0;
    long long off = block_scan_excl<1>(size, 0ll, OpAdd(), wsum, &all_size);
    (void)block_scan_excl<1>(raws, 0ll, OpAdd(), wsum, &all_raw);
    const long long first = (long long)L.header_bytes + 8LL * L.n_blocks;      // behind the offset table
    for (int b = b0; b < b1; ++b) {
        unsigned adler;
        const long long stream = block_stream(L, meta, b, adler), n = block_bytes(L, b);
        const bool raw = stream >= n;
        const long long at = first + off, data = raw ? n : stream;
        unsigned char *entry = file + L.header_bytes + 8LL * b, *head = file + at;
        store_le32(entry, (unsigned)at);
        store_le32(entry + 4, (unsigned)(at >> 32));
        store_le32(head, (unsigned)(EXR_LINES * b));
        store_le32(head + 4, (unsigned)data);
        ExrBlock rec;
        rec.data_off = at + 8;
        rec.raw = raw ? 1 : 0;
        rec.pad = 0;
        blocks[b] = rec;
        const int n_c = (int)((n + PNG_CHUNK - 1) / PNG_CHUNK);
        long long pos = at + 8 + 2;
        for (int c = 0; c < n_c; ++c) {
            offsets[b * L.cpb + c] = pos;       // (unused for a fallback block)
            pos += meta[b * L.cpb + c].bytes;
        }
        if (!raw) {
            head[8] = 0x78; head[9] = 0x01;
            unsigned char *z = file + pos;      // the stream's Adler-32, most significant byte first
            z[0] = (unsigned char)(adler >> 24); z[1] = (unsigned char)(adler >> 16); z[2] = (unsigned char)(adler >> 8); z[3] = (unsigned char)adler;
        }
        off += 8 + data;
    }
    if (t == 0) {
        if (chans) (void)exr_header_list(file, L.width, L.rows, chans);
        else (void)exr_header(file, L.width, L.rows, L.n_ch, L.pixel_type);
        info->file_bytes = first + all_size;
        info->raw_bytes = L.raw_bytes;
        info->blocks = L.n_blocks;
        info->blocks_raw = (int)all_raw;
    }
}

template <class SRC>
__global__ void __launch_bounds__(256) k_exr_place(ExrLayout L, SRC src,
                                                   const unsigned char *__restrict__ slots, const ChunkMeta *__restrict__ meta,
                                                   const long long *__restrict__ offsets, const ExrBlock *__restrict__ blocks, unsigned char *file)
{
    const int idx = (int)blockIdx.x, block = idx / L.cpb, c = idx - block * L.cpb;
    const ExrBlock rec = blocks[block];
    if (rec.raw) {
        const int r0 = c * PNG_CHUNK, left = block_bytes(L, block) - r0, n = left < PNG_CHUNK ? left : PNG_CHUNK;
        unsigned char *dst = file + rec.data_off + r0;
        for (int k = (int)threadIdx.x; k < n; k += 256) dst[k] = (unsigned char)src.byte(L, block, r0 + k);
    } else {
        const unsigned char *src = slots + (long long)idx * PNG_SLOT;
        unsigned char *dst = file + offsets[idx];
        const int bytes = (int)meta[idx].bytes;             // at most 5 + 32768
        for (int k = (int)threadIdx.x; k < bytes; k += 256) dst[k] = src[k];
    }
}

// ------------------------------------------------------------------ host

// 1 half, 2 float, 0 = half; anything else -1
int pixel_type_of(const ndt_exr_params *ep)
{
    if (!ep || ep->pixel_type == 0 || ep->pixel_type == EXR_HALF) return EXR_HALF;
    return ep->pixel_type == EXR_FLOAT ? EXR_FLOAT : -1;
}

// the file's layout, or false for a size the encoder does not take: empty, or raw bytes beyond 2^31 - 1
// (C: the channel table of a file with feature channels -- its channels, not A B G R [Z], make the scanline)
bool layout_of(int32_t width, int32_t rows, int pixel_type, bool with_depth, ExrLayout &L, const ExrChannels *C = nullptr)
{
    if (width < 1 || rows < 1 || pixel_type < 0) return false;
    const long long bs = pixel_type == EXR_HALF ? 2 : 4;
    long long colour = 4 * bs * (long long)width, line = colour + (with_depth ? 4LL * width : 0);
    if (C) {
        line = (long long)C->units * width;     // the table's channels
        colour = 0;
    }
    const long long raw = line * (long long)rows;
    if (raw > 0x7fffffffLL) return false;
    const long long n_blocks = ((long long)rows + EXR_LINES - 1) / EXR_LINES;
    const long long full = (rows < EXR_LINES ? rows : EXR_LINES) * line, last = raw - (n_blocks - 1) * EXR_LINES * line;
    const long long cpb = (full + PNG_CHUNK - 1) / PNG_CHUNK;
    L = ExrLayout{};
    L.width = width; L.rows = rows; L.n_ch = with_depth ? 5 : 4; L.pixel_type = pixel_type;
    L.line_bytes = (int)line; L.colour_bytes = (int)colour;
    L.n_blocks = (int)n_blocks; L.cpb = (int)cpb;
    L.n_chunks = (int)((n_blocks - 1) * cpb + (last + PNG_CHUNK - 1) / PNG_CHUNK);
    if (C) L.n_ch = C->n;
    L.header_bytes = C ? exr_header_list(nullptr, width, rows, C) : exr_header(nullptr, width, rows, L.n_ch, pixel_type);
    L.raw_bytes = raw;
    return true;
}

// The channel table of a file with the feature groups of `features`, in the byte-wise order of the names: A B G, N.00 .., P.00 ..,
// R, Z, id.  Indices have two digits, so that order is the numeric one.  planes may be nullptr (the sizes only).  with_ao: the FLOAT
// channel AO of the plane d_ao (ndt_ao.hip) between A and B.
void channel_table(ExrChannels &C, int pixel_type, const void *d_rgba, const void *d_depth, bool with_depth, const ndt_feature_planes *planes,
                   int dims, int features, long long pixels, bool with_ao = false, const void *d_ao = nullptr)
{
    C = ExrChannels{};
    auto add = [&C](const char *name, int index, const void *src, int stride, bool is_int, int conv) {
        ExrChannel &ch = C.ch[C.n];
        ch.src = src;
        ch.stride = stride;
        ch.is_int = is_int ? 1 : 0;
        ch.conv = conv;
        ch.pixel_type = conv == EXR_TO_HALF ? EXR_HALF : conv == EXR_TO_FLOAT ? EXR_FLOAT : EXR_UINT;
        ch.bytes = conv == EXR_TO_HALF ? 2 : 4;
        ch.first_unit = C.units;
        if (index < 0) snprintf(ch.name, sizeof(ch.name), "%s", name);
        else snprintf(ch.name, sizeof(ch.name), "%s.%02d", name, index);
        for (int k = 0; k < ch.bytes; ++k) C.unit_channel[C.units++] = (unsigned char)C.n;
        ++C.n;
    };
    const int colour = pixel_type == EXR_HALF ? EXR_TO_HALF : EXR_TO_FLOAT;
    const double *rgba = (const double *)d_rgba;
    add("A", -1, rgba ? rgba + 3 : nullptr, 4, false, colour);      // the framebuffer is R G B A
    if (with_ao) add("AO", -1, d_ao, 1, false, EXR_TO_FLOAT);
    add("B", -1, rgba ? rgba + 2 : nullptr, 4, false, colour);
    add("G", -1, rgba ? rgba + 1 : nullptr, 4, false, colour);
    if (features & NDT_FEATURE_NORMAL)
        for (int c = 0; c < dims; ++c) add("N", c, planes && planes->normal ? planes->normal + c * pixels : nullptr, 1, false, EXR_TO_FLOAT);
    if (features & NDT_FEATURE_POSITION)
        for (int c = 0; c < dims; ++c) add("P", c, planes && planes->position ? planes->position + c * pixels : nullptr, 1, false, EXR_TO_FLOAT);
    add("R", -1, rgba, 4, false, colour);
    if (with_depth) add("Z", -1, d_depth, 1, false, EXR_TO_FLOAT);
    if (features & NDT_FEATURE_ID) add("id", -1, planes ? planes->id : nullptr, 1, true, EXR_AS_UINT);
}

bool features_ok(int dims, int features)
{
    return dims >= NDT_MIN_DIMS && dims <= NDT_MAX_DIMS && features != 0 && (features & ~EXR_ALL_FEATURES) == 0;
}

// every block raw: the header, an offset and a block header a block, the raw bytes
long long file_bound(const ExrLayout &L) { return (long long)L.header_bytes + 16LL * L.n_blocks + L.raw_bytes; }

// (d_chans: the channel table in device memory where SRC reads one, else nullptr)
template <class SRC>
void launch_all(hipStream_t s, const ExrLayout &L, SRC src, const ExrChannels *d_chans, ExrState &ex)
{
    const int words = (int)(((long long)L.cpb * PNG_CHUNK) / 4), across = (words + 255) / 256;
    hipLaunchKernelGGL(k_exr_pack<SRC>, dim3((unsigned)(across < 256 ? across : 256), (unsigned)L.n_blocks), dim3(256), 0, s, L, src,
                       ex.d_packed.as<unsigned>());
    hipLaunchKernelGGL(k_exr_deflate, dim3((unsigned)L.n_chunks), dim3(PNG_DEFLATE_LANES), 0, s, L, ex.d_packed.as<const unsigned char>(),
                       ex.d_slots.as<unsigned char>(), ex.d_meta.as<ChunkMeta>());
    hipLaunchKernelGGL(k_exr_assemble, dim3(1), dim3(1024), 0, s, L, ex.d_meta.as<const ChunkMeta>(), ex.d_file.as<unsigned char>(),
                       ex.d_offsets.as<long long>(), ex.d_blocks.as<ExrBlock>(), ex.d_info.as<ExrInfo>(), d_chans);
    hipLaunchKernelGGL(k_exr_place<SRC>, dim3((unsigned)L.n_chunks), dim3(256), 0, s, L, src, ex.d_slots.as<const unsigned char>(),
                       ex.d_meta.as<const ChunkMeta>(), ex.d_offsets.as<const long long>(), ex.d_blocks.as<const ExrBlock>(),
                       ex.d_file.as<unsigned char>());
}

// The file of the width x rows doubles at d_rgba (and the map at d_depth, or nullptr) -- the context's device memory -- in host
// memory; `who` names the entry point in errors.  features != 0: with the feature channels of that mask from d_planes.  d_ao: with
// the channel AO of that plane (features may then be 0).
int encode_device(ndt_hip_ctx *ctx, const char *who, const void *d_rgba, const void *d_depth, int32_t width, int32_t rows,
                  const ndt_exr_params *ep, uint8_t *out, int64_t cap, ndt_exr_stats *stats, const ndt_feature_planes *d_planes = nullptr,
                  int dims = 0, int features = 0, const void *d_ao = nullptr)
{
    if (stats) *stats = ndt_exr_stats{};
    if (!ctx || !d_rgba || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a %d x %d image", who, width, rows);
    const int pixel_type = pixel_type_of(ep);
    if (pixel_type < 0) return fail(NDT_E_INVALID, "%s: pixel type %d: 1 is half, 2 float (0: half)", who, ep->pixel_type);
    if (cap < 0) return fail(NDT_E_INVALID, "%s: cap %lld", who, (long long)cap);
    if ((((uintptr_t)d_rgba | (uintptr_t)d_depth) & 7u) != 0) return fail(NDT_E_INVALID, "%s: the doubles are not aligned to 8 bytes", who);
    ExrChannels table;
    const bool listed = features != 0 || d_ao != nullptr;
    if (((uintptr_t)d_ao & 7u) != 0) return fail(NDT_E_INVALID, "%s: the AO plane is not aligned to 8 bytes", who);
    if (d_ao && !features) channel_table(table, pixel_type, d_rgba, d_depth, d_depth != nullptr, nullptr, dims, 0, (long long)width * rows, true, d_ao);
    if (features) {
        if (!features_ok(dims, features))
            return fail(NDT_E_INVALID, "%s: %d dimensions, feature mask %d: 3 .. 12, and a mask of id 1, position 2, normal 4", who, dims, features);
        if (!d_planes || ((features & NDT_FEATURE_ID) && !d_planes->id) || ((features & NDT_FEATURE_POSITION) && !d_planes->position) ||
            ((features & NDT_FEATURE_NORMAL) && !d_planes->normal))
            return fail(NDT_E_INVALID, "%s: a plane of feature mask %d is NULL", who, features);
        if (((uintptr_t)d_planes->id & 3u) != 0 || (((uintptr_t)d_planes->position | (uintptr_t)d_planes->normal) & 7u) != 0)
            return fail(NDT_E_INVALID, "%s: a feature plane is not aligned to its elements", who);
        channel_table(table, pixel_type, d_rgba, d_depth, d_depth != nullptr, d_planes, dims, features, (long long)width * rows, d_ao != nullptr, d_ao);
    }
    ExrLayout L;
    if (!layout_of(width, rows, pixel_type, d_depth != nullptr, L, listed ? &table : nullptr))
        return fail(NDT_E_INVALID, "%s: the samples of a %d x %d image exceed 2^31 - 1 bytes", who, width, rows);
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(ctx->device));
    ExrState &ex = ctx->exr;
    hipStream_t s = ctx->stream;
    const long long bound = file_bound(L);
    int rc;
    if ((rc = ex.d_packed.reserve((size_t)L.n_chunks * PNG_CHUNK, s, who))) return rc;
    if ((rc = ex.d_slots.reserve((size_t)L.n_chunks * PNG_SLOT, s, who))) return rc;
    if ((rc = ex.d_meta.reserve((size_t)L.n_chunks * sizeof(ChunkMeta), s, who))) return rc;
    if ((rc = ex.d_offsets.reserve((size_t)L.n_chunks * sizeof(long long), s, who))) return rc;
    if ((rc = ex.d_blocks.reserve((size_t)L.n_blocks * sizeof(ExrBlock), s, who))) return rc;
    if ((rc = ex.d_file.reserve((size_t)bound, s, who))) return rc;
    if ((rc = ex.d_info.reserve(sizeof(ExrInfo), s, who))) return rc;
    if (!ex.h_info) HIP_TRY(hipHostMalloc(&ex.h_info, sizeof(ExrInfo), hipHostMallocDefault));
    if (listed) {
        // (the table leaves this frame before the call goes on: it is copied from pageable memory)
        if ((rc = ex.d_channels.reserve(sizeof(ExrChannels), s, who))) return rc;
        HIP_TRY(hipMemcpyAsync(ex.d_channels.p, &table, sizeof(ExrChannels), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        launch_all(s, L, ListSource{ ex.d_channels.as<const ExrChannels>() }, ex.d_channels.as<const ExrChannels>(), ex);
    } else if (pixel_type == EXR_HALF) {
        launch_all(s, L, PlainSource<true>{ (const double *)d_rgba, (const double *)d_depth }, nullptr, ex);
    } else {
        launch_all(s, L, PlainSource<false>{ (const double *)d_rgba, (const double *)d_depth }, nullptr, ex);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ex.h_info, ex.d_info.p, sizeof(ExrInfo), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const ExrInfo info = *(const ExrInfo *)ex.h_info;
    if (stats) {
        stats->file_bytes = info.file_bytes;
        stats->raw_bytes = info.raw_bytes;
        stats->blocks = info.blocks;
        stats->blocks_raw = info.blocks_raw;
        stats->launches = 4;
    }
    if (info.file_bytes < L.header_bytes + 16LL * L.n_blocks || info.file_bytes > bound || info.blocks != L.n_blocks)
        return fail(NDT_E_DEVICE, "%s: the device reports a file of %lld bytes in %d blocks (bound %lld, %d blocks)", who, info.file_bytes,
                    info.blocks, bound, L.n_blocks);
    if (info.file_bytes > cap)
        return fail(NDT_E_NOMEM, "%s: the file is %lld bytes, the buffer %lld", who, info.file_bytes, (long long)cap);
    HIP_TRY(hipMemcpyAsync(out, ex.d_file.p, (size_t)info.file_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (stats) stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return NDT_OK;
}

// the frame (K = 0: plain; K >= 1: supersampled K x K) in doubles in ctx->d_out, its map behind it if wanted, then the file of those
// features != 0: behind the render the feature pass of the plain frame, on the same stream, and its planes as channels
int render_file(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_exr_params *ep, int32_t with_depth,
                uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats, int features = 0)
{
    if (stats) *stats = ndt_exr_stats{};
    int rows = 0;
    int rc = refuse_exr(who, ctx, p, ep, with_depth, out, &rows);
    if (rc) return rc;
    if (features) {
        if ((features & ~EXR_ALL_FEATURES) != 0) return fail(NDT_E_INVALID, "%s: feature mask %d: id 1, position 2, normal 4", who, features);
        int feature_rows = 0;
        if ((rc = features_check(who, ctx, p, &feature_rows))) return rc;
        ExrChannels table;
        ExrLayout L;
        channel_table(table, pixel_type_of(ep), nullptr, nullptr, with_depth != 0, nullptr, ctx->dims, features, 0);
        if (!layout_of(p->width, rows, pixel_type_of(ep), with_depth != 0, L, &table))
            return fail(NDT_E_INVALID, "%s: the samples of a %d x %d image exceed 2^31 - 1 bytes", who, p->width, rows);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t pixels = (size_t)p->width * (size_t)rows, img_bytes = pixels * 4 * sizeof(double);
    if ((rc = ctx->d_out.reserve(img_bytes + (with_depth ? pixels * sizeof(double) : 0), ctx->stream, who))) return rc;
    void *d_depth = with_depth ? (void *)(ctx->d_out.as<char>() + img_bytes) : nullptr;
    rc = K ? ndt_hip_render_ssaa_device(ctx, p, K, ctx->d_out.p, d_depth, render_stats)
           : ndt_hip_render_depth_device(ctx, p, ctx->d_out.p, d_depth, render_stats);
    if (rc) return rc;
    if (!features) return encode_device(ctx, who, ctx->d_out.p, d_depth, p->width, rows, ep, out, cap, stats);
    ndt_feature_planes planes;
    if ((rc = features_own(ctx, who, p, features, false, &planes))) return rc;
    return encode_device(ctx, who, ctx->d_out.p, d_depth, p->width, rows, ep, out, cap, stats, &planes, ctx->dims, features);
}

} // namespace

// what the render entries check before any device work; *rows: the shard's
int ndt_impl::refuse_exr(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int with_depth, uint8_t *out, int *rows)
{
    if (!ctx || !p || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0)
        return fail(NDT_E_INVALID, "%s: bad geometry: %d x %d, rows %d by %d", who, p->width, p->height, p->row_begin, p->row_step);
    *rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    if (*rows < 1) return refuse_empty_shard(who, *rows);
    const int pixel_type = pixel_type_of(ep);
    if (pixel_type < 0) return fail(NDT_E_INVALID, "%s: pixel type %d: 1 is half, 2 float (0: half)", who, ep->pixel_type);
    ExrLayout L;
    if (!layout_of(p->width, *rows, pixel_type, with_depth != 0, L))
        return fail(NDT_E_INVALID, "%s: the samples of a %d x %d image exceed 2^31 - 1 bytes", who, p->width, *rows);
    return NDT_OK;
}

void ndt_impl::free_exr(ndt_hip_ctx *ctx)
{
    ExrState &ex = ctx->exr;
    ex.d_in.release();
    ex.d_packed.release();
    ex.d_slots.release();
    ex.d_meta.release();
    ex.d_offsets.release();
    ex.d_blocks.release();
    ex.d_file.release();
    ex.d_info.release();
    ex.d_channels.release();
    if (ex.h_info) (void)hipHostFree(ex.h_info);
    ex = ExrState();
}

extern "C" int64_t ndt_hip_exr_bound(int32_t width, int32_t rows, const ndt_exr_params *ep, int32_t with_depth)
{
    ExrLayout L;
    if (!layout_of(width, rows, pixel_type_of(ep), with_depth != 0, L)) return NDT_E_INVALID;
    return file_bound(L);
}

extern "C" int ndt_hip_encode_exr_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_depth, int32_t width, int32_t rows,
                                         const ndt_exr_params *ep, uint8_t *out, int64_t cap, ndt_exr_stats *stats)
{
    return encode_device(ctx, "ndt_hip_encode_exr", d_rgba, d_depth, width, rows, ep, out, cap, stats);
}

extern "C" int ndt_hip_encode_exr(ndt_hip_ctx *ctx, const double *rgba, const double *depth, int32_t width, int32_t rows, const ndt_exr_params *ep,
                                  uint8_t *out, int64_t cap, ndt_exr_stats *stats)
{
    const char *who = "ndt_hip_encode_exr";
    if (stats) *stats = ndt_exr_stats{};
    if (!ctx || !rgba || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a %d x %d image", who, width, rows);
    const int pixel_type = pixel_type_of(ep);
    if (pixel_type < 0) return fail(NDT_E_INVALID, "%s: pixel type %d: 1 is half, 2 float (0: half)", who, ep->pixel_type);
    ExrLayout L;
    if (!layout_of(width, rows, pixel_type, depth != nullptr, L))
        return fail(NDT_E_INVALID, "%s: the samples of a %d x %d image exceed 2^31 - 1 bytes", who, width, rows);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t pixels = (size_t)width * (size_t)rows, img_bytes = pixels * 4 * sizeof(double);
    int rc = ctx->exr.d_in.reserve(img_bytes + (depth ? pixels * sizeof(double) : 0), ctx->stream, who);
    if (rc) return rc;
    char *d_in = ctx->exr.d_in.as<char>();
    HIP_TRY(hipMemcpyAsync(d_in, rgba, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (depth) HIP_TRY(hipMemcpyAsync(d_in + img_bytes, depth, pixels * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return encode_device(ctx, who, d_in, depth ? d_in + img_bytes : nullptr, width, rows, ep, out, cap, stats);
}

extern "C" int ndt_hip_render_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int32_t with_depth, uint8_t *out,
                                  int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats)
{
    return render_file("ndt_hip_render_exr", ctx, p, 0, ep, with_depth, out, cap, stats, render_stats);
}

extern "C" int ndt_hip_render_ssaa_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_exr_params *ep, int32_t with_depth,
                                       uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats)
{
    if (K < 1 || K > 8) return fail(NDT_E_INVALID, "ndt_hip_render_ssaa_exr: ssaa %d is outside 1 .. 8", K);
    return render_file("ndt_hip_render_ssaa_exr", ctx, p, K, ep, with_depth, out, cap, stats, render_stats);
}

extern "C" int64_t ndt_hip_exr_features_bound(int32_t width, int32_t rows, const ndt_exr_params *ep, int32_t with_depth, int32_t dims,
                                              int32_t features)
{
    const int pixel_type = pixel_type_of(ep);
    if (pixel_type < 0 || !features_ok(dims, features)) return NDT_E_INVALID;
    ExrChannels table;
    ExrLayout L;
    channel_table(table, pixel_type, nullptr, nullptr, with_depth != 0, nullptr, dims, features, 0);
    if (!layout_of(width, rows, pixel_type, with_depth != 0, L, &table)) return NDT_E_INVALID;
    return file_bound(L);
}

// what the AO entries take: a mask of the three groups, or none
static bool ao_features_ok(int dims, int features)
{
    return dims >= NDT_MIN_DIMS && dims <= NDT_MAX_DIMS && features >= 0 && (features & ~EXR_ALL_FEATURES) == 0;
}

extern "C" int64_t ndt_hip_exr_ao_bound(int32_t width, int32_t rows, const ndt_exr_params *ep, int32_t with_depth, int32_t dims, int32_t features)
{
    const int pixel_type = pixel_type_of(ep);
    if (pixel_type < 0 || !ao_features_ok(dims, features)) return NDT_E_INVALID;
    ExrChannels table;
    ExrLayout L;
    channel_table(table, pixel_type, nullptr, nullptr, with_depth != 0, nullptr, dims, features, 0, true, nullptr);
    if (!layout_of(width, rows, pixel_type, with_depth != 0, L, &table)) return NDT_E_INVALID;
    return file_bound(L);
}

int ndt_impl::exr_encode_ao_device(ndt_hip_ctx *ctx, const char *who, const void *d_rgba, const void *d_depth, const ndt_feature_planes *d_planes,
                                   const void *d_ao, int dims, int features, int32_t width, int32_t rows, const ndt_exr_params *ep, uint8_t *out,
                                   int64_t cap, ndt_exr_stats *stats)
{
    if (stats) *stats = ndt_exr_stats{};
    if (!d_ao) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (!ao_features_ok(dims, features))
        return fail(NDT_E_INVALID, "%s: %d dimensions, feature mask %d: 3 .. 12, and a mask of id 1, position 2, normal 4, or 0", who, dims, features);
    return encode_device(ctx, who, d_rgba, d_depth, width, rows, ep, out, cap, stats, d_planes, dims, features, d_ao);
}

extern "C" int ndt_hip_encode_exr_ao_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_depth, const ndt_feature_planes *d_planes,
                                            const void *d_ao, int32_t dims, int32_t features, int32_t width, int32_t rows,
                                            const ndt_exr_params *ep, uint8_t *out, int64_t cap, ndt_exr_stats *stats)
{
    return exr_encode_ao_device(ctx, "ndt_hip_encode_exr_ao_device", d_rgba, d_depth, d_planes, d_ao, dims, features, width, rows, ep, out, cap, stats);
}

extern "C" int ndt_hip_encode_exr_features_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_depth, const ndt_feature_planes *d_planes,
                                                  int32_t dims, int32_t features, int32_t width, int32_t rows, const ndt_exr_params *ep,
                                                  uint8_t *out, int64_t cap, ndt_exr_stats *stats)
{
    const char *who = "ndt_hip_encode_exr_features_device";
    if (stats) *stats = ndt_exr_stats{};
    if (!features_ok(dims, features))
        return fail(NDT_E_INVALID, "%s: %d dimensions, feature mask %d: 3 .. 12, and a mask of id 1, position 2, normal 4", who, dims, features);
    return encode_device(ctx, who, d_rgba, d_depth, width, rows, ep, out, cap, stats, d_planes, dims, features);
}

extern "C" int ndt_hip_render_exr_features(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int32_t with_depth,
                                           int32_t features, uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_exr_features";
    if (features == 0) return fail(NDT_E_INVALID, "%s: feature mask 0: id 1, position 2, normal 4", who);
    return render_file(who, ctx, p, 0, ep, with_depth, out, cap, stats, render_stats, features);
}

extern "C" int ndt_hip_render_ssaa_exr_features(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_exr_params *ep,
                                                int32_t with_depth, int32_t features, uint8_t *out, int64_t cap, ndt_exr_stats *stats,
                                                ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_ssaa_exr_features";
    if (K < 1 || K > 8) return fail(NDT_E_INVALID, "%s: ssaa %d is outside 1 .. 8", who, K);
    if (features == 0) return fail(NDT_E_INVALID, "%s: feature mask 0: id 1, position 2, normal 4", who);
    return render_file(who, ctx, p, K, ep, with_depth, out, cap, stats, render_stats, features);
}
