// ndt_jpeg.hip -- a frame's JPEG file made on the device: ndt_hip_jpeg_bound / ndt_hip_encode_jpeg_device / ndt_hip_encode_jpeg /
// ndt_hip_render_jpeg.  The quantised image is in HBM already; what leaves the device is the finished file: the baseline JFIF
// file libjpeg writes for the image (quality q, 4:2:0 or 4:4:4, its default tables, one restart interval per MCU row), byte
// for byte -- every step is libjpeg's integer arithmetic.
//
//   k_jpeg_blocks    one wavefront an MCU: its pixels staged in LDS, Y Cb Cr, the 4:2:0 average, the two passes of the slow
//                    integer DCT with one lane per 8-point transform, the quantiser; int16 coefficients in zigzag order,
//                    block-major in scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU under 4:2:0)
//   k_jpeg_entropy   one workgroup a restart interval (an MCU row): a lane a block -- its bits counted, a scan for its place,
//                    its bits OR-ed into an LDS bit buffer; the buffer's bytes then go to the interval's staging slot with
//                    0x00 behind every 0xFF.  A slab of blocks whose bits the buffer cannot hold waits for the next pass
//   k_jpeg_assemble  one workgroup: the intervals' places (a scan of their byte counts and the RSTm between them), the header
//                    segments SOI .. SOS
//   k_jpeg_place     one workgroup an interval: its bytes to their place in the file, RSTm behind it, EOI behind the last
//
// No kernel waits for another workgroup, every loop's trip count comes from the image size, and the only atomics are LDS
// atomics inside a workgroup.  The host reads the info record, then exactly the file's bytes.
//
// Edges are libjpeg's: a component's blocks are filled with the last column of the source and the last row of the component
// (for 4:2:0 chroma: of the down-sampled component, whose last row averages source rows 2k and min(2k + 1, rows - 1)), and a
// luminance block wholly outside the image is a dummy -- no AC, the DC of the block before it in its MCU (jccoefct.c).
//
// The bound.  A block costs at most 22 + 63 * 26 = 1660 bits: a DC code of at most 11 bits with 11 extra bits, and per AC
// coefficient at most a 16-bit code with 10 extra bits (ZRL, 11 bits for 16 coefficients, and EOB, 4 bits for at least one, cost
// less per coefficient).  An interval of B blocks is ceil((1660 B + 7) / 8) bytes with its padding, at most twice that with every
// byte stuffed: its staging slot.  The file: 629 bytes SOI .. SOS, the slots, 2 bytes of RSTm or EOI behind each, 2 to spare.
#include "ndt_ctx.hpp"
#include <chrono>

namespace {

constexpr int JPEG_HEAD = 629;                  // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
constexpr int JPEG_BLOCK_BITS = 22 + 63 * 26;
constexpr int JPEG_LANES = 256;                 // lanes of k_jpeg_entropy: blocks of a slab
constexpr int JPEG_BUF_WORDS = 4096;            // its bit buffer: 16 KiB -- 256 blocks of 512 bits; denser blocks take more passes
constexpr unsigned JPEG_BUF_BITS = 32u * JPEG_BUF_WORDS - 64u;

// what the kernels need to know of the image (scalars only: indexed tables live in constant memory)
struct JpegGeom {
    int width, rows, scale;         // scale: libjpeg's quality scaling, 5000 / q or 200 - 2 q
    int side, blocks_per_mcu;       // 16 and 6 (4:2:0) or 8 and 3 (4:4:4)
    int mcu_w, mcu_h;               // MCUs a row = blocks of an interval / blocks_per_mcu; MCU rows = intervals
    int aligned;                    // rows of the image start on 16-byte boundaries
    long long slot_bytes;           // an interval's staging slot
};

struct IntervalMeta { unsigned bytes, stuffed, passes, pad; };

struct JpegInfo {
    long long jpeg_bytes, scan_bytes, stuffed_bytes;
    int passes_max;
    int pad[9];
};

__constant__ unsigned char jpeg_zigzag[64] = { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
// Annex K.1: luminance, chrominance (natural order)
__constant__ unsigned char jpeg_base_q[2][64] = {
    { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };
// Annex K.3: codes per length and the symbols in code order; the DC symbols are 0 .. 11
__constant__ unsigned char jpeg_dc_bits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
__constant__ unsigned char jpeg_ac_bits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
__constant__ unsigned char jpeg_ac_vals[2][162] = {
    { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa },
    { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa } };

// jpeg_add_quant_table with force_baseline
__device__ __forceinline__ int quant_step(int base, int scale)
{
    const int v = (base * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// exclusive scan over the workgroup's lanes (whole wavefronts); `op` commutes.  Every lane calls it; *total (may be null) gets
// the fold over all lanes.
template <typename Op>
__device__ __forceinline__ long long jpeg_scan_excl(long long v, long long identity, Op op, long long *wsum, long long *total)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(x, d, 64);
        if (lane >= d) x = op(x, o);
    }
    if (lane == 63) wsum[wave] = x;
    long long prev = __shfl_up(x, 1, 64);
    if (lane == 0) prev = identity;
    __syncthreads();
    long long carry = identity, all = identity;
    for (int w = 0; w < n_waves; ++w) {
        const long long s = wsum[w];
        all = op(all, s);
        if (w < wave) carry = op(carry, s);
    }
    __syncthreads();
    if (total) *total = all;
    return op(carry, prev);
}

struct JOpAdd { __device__ long long operator()(long long a, long long b) const { return a + b; } };
struct JOpMax { __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; } };

// ------------------------------------------------------------------ pixels to coefficients

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's slow integer DCT (jfdctint.c: CONST_BITS 13, PASS1_BITS 2) over 8 values; FIRST: the row pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&x)[8])
{
    const int t0 = x[0] + x[7], t7 = x[0] - x[7], t1 = x[1] + x[6], t6 = x[1] - x[6];
    const int t2 = x[2] + x[5], t5 = x[2] - x[5], t3 = x[3] + x[4], t4 = x[3] - x[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int N = FIRST ? 11 : 15;
    x[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    x[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    x[2] = descale(z1 + t13 * 6270, N);
    x[6] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    x[7] = descale(u4 + z1 + z3, N);
    x[5] = descale(u5 + z2 + z4, N);
    x[3] = descale(u6 + z2 + z3, N);
    x[1] = descale(u7 + z1 + z4, N);
}

// jccolor.c's fixed-point Y Cb Cr of a pixel (bytes R, G, B, A from the low end), level-shifted
__device__ __forceinline__ int pixel_y(unsigned p)
{
    const int r = (int)(p & 255u), g = (int)((p >> 8) & 255u), b = (int)((p >> 16) & 255u);
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
}
__device__ __forceinline__ int pixel_cb(unsigned p)
{
    const int r = (int)(p & 255u), g = (int)((p >> 8) & 255u), b = (int)((p >> 16) & 255u);
    return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
}
__device__ __forceinline__ int pixel_cr(unsigned p)
{
    const int r = (int)(p & 255u), g = (int)((p >> 8) & 255u), b = (int)((p >> 16) & 255u);
    return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

constexpr int JPEG_WS_ROW = 9;                  // a block's rows in LDS: 8 values and a pad, so that neither DCT pass meets a bank twice
constexpr int JPEG_WS_BLOCK = 8 * JPEG_WS_ROW;

// luminance block k of MCU (mx, my) under 4:2:0 holds no image
__device__ __forceinline__ bool dummy_block(const JpegGeom &g, int mx, int my, int k)
{
    return 2 * my + (k >> 1) >= ((g.rows + 7) >> 3) || 2 * mx + (k & 1) >= ((g.width + 7) >> 3);
}

__global__ void __launch_bounds__(256) k_jpeg_blocks(const unsigned *__restrict__ image, JpegGeom g, short *__restrict__ coef)
{
    __shared__ __attribute__((aligned(16))) unsigned tile[4][256];
    __shared__ int ws[4][6 * JPEG_WS_BLOCK];
    __shared__ unsigned short qt[2][64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < 128) qt[t >> 6][t & 63] = (unsigned short)quant_step(jpeg_base_q[t >> 6][t & 63], g.scale);
    const int mcu = (int)blockIdx.x * 4 + wave;
    const bool live = mcu < g.mcu_w * g.mcu_h;
    const int my = live ? mcu / g.mcu_w : 0, mx = live ? mcu - my * g.mcu_w : 0;
    const int side = g.side, nb = g.blocks_per_mcu, x0 = mx * side, y0 = my * side;
    unsigned *tl = tile[wave];
    int *w = ws[wave];

    // the MCU's pixels, coordinates clamped to the image: four a lane, one 16-byte load where the row allows it
    if (live && lane < side * side / 4) {
        const int per_row = side >> 2, ly = lane / per_row, lx = (lane - ly * per_row) << 2;
        const int y = y0 + ly < g.rows ? y0 + ly : g.rows - 1, x = x0 + lx;
        const unsigned *row = image + (long long)y * g.width;
        uint4 p;
        if (g.aligned && x + 3 < g.width) p = *reinterpret_cast<const uint4 *>(row + x);
        else {
            const int last = g.width - 1;
            p.x = row[x < last ? x : last];
            p.y = row[x + 1 < last ? x + 1 : last];
            p.z = row[x + 2 < last ? x + 2 : last];
            p.w = row[x + 3 < last ? x + 3 : last];
        }
        *reinterpret_cast<uint4 *>(tl + ly * side + lx) = p;
    }
    __syncthreads();

    if (live) {
        if (nb == 6) {
            for (int i = lane; i < 256; i += 64) {
                const int ly = i >> 4, lx = i & 15, b = ((ly >> 3) << 1) | (lx >> 3);
                w[b * JPEG_WS_BLOCK + (ly & 7) * JPEG_WS_ROW + (lx & 7)] = pixel_y(tl[i]);
            }
            // chroma sample (cx, cy) of the MCU: the average of a 2 x 2 of the source whose rows are those of the component's
            // row -- the last one repeated below the image
            const int cy = lane >> 3, cx = lane & 7;
            const int last_crow = ((g.rows + 1) >> 1) - 1, crow = (y0 >> 1) + cy < last_crow ? (y0 >> 1) + cy : last_crow;
            const int ra = 2 * crow - y0, rb = (2 * crow + 1 < g.rows ? 2 * crow + 1 : g.rows - 1) - y0;
            const unsigned p00 = tl[ra * 16 + 2 * cx], p01 = tl[ra * 16 + 2 * cx + 1], p10 = tl[rb * 16 + 2 * cx], p11 = tl[rb * 16 + 2 * cx + 1];
            const int bias = 1 + (cx & 1);
            w[4 * JPEG_WS_BLOCK + cy * JPEG_WS_ROW + cx] = ((pixel_cb(p00) + pixel_cb(p01) + pixel_cb(p10) + pixel_cb(p11) + bias) >> 2) - 128;
            w[5 * JPEG_WS_BLOCK + cy * JPEG_WS_ROW + cx] = ((pixel_cr(p00) + pixel_cr(p01) + pixel_cr(p10) + pixel_cr(p11) + bias) >> 2) - 128;
        } else {
            const unsigned p = tl[lane];
            const int at = (lane >> 3) * JPEG_WS_ROW + (lane & 7);
            w[at] = pixel_y(p);
            w[JPEG_WS_BLOCK + at] = pixel_cb(p) - 128;
            w[2 * JPEG_WS_BLOCK + at] = pixel_cr(p) - 128;
        }
    }
    __syncthreads();

    // rows, then columns: lane (block, line) transforms its 8 values in place
    const bool works = live && lane < nb * 8;
    int *line = w + (lane >> 3) * JPEG_WS_BLOCK;
    if (works) {
        int x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = line[(lane & 7) * JPEG_WS_ROW + k];
        fdct8<true>(x);
#pragma unroll
        for (int k = 0; k < 8; ++k) line[(lane & 7) * JPEG_WS_ROW + k] = x[k];
    }
    __syncthreads();
    if (works) {
        int x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = line[k * JPEG_WS_ROW + (lane & 7)];
        fdct8<false>(x);
#pragma unroll
        for (int k = 0; k < 8; ++k) line[k * JPEG_WS_ROW + (lane & 7)] = x[k];
    }
    __syncthreads();

    // jcdctmgr.c's quantiser (the divisor is the step << 3: the DCT's outputs are 8 x the coefficients), zigzag order
    if (live) {
        short *out = coef + (long long)mcu * nb * 64;
        for (int i = lane; i < nb * 64; i += 64) {
            const int b = i >> 6, z = i & 63;
            int src = b, n = jpeg_zigzag[z];
            bool dummy = false;
            if (nb == 6 && b > 0 && b < 4 && dummy_block(g, mx, my, b)) {
                dummy = true;
                n = 0;
                src = b - 1;
                if (src > 0 && dummy_block(g, mx, my, src)) --src;
                if (src > 0 && dummy_block(g, mx, my, src)) --src;
            }
            const int c = w[src * JPEG_WS_BLOCK + (n >> 3) * JPEG_WS_ROW + (n & 7)];
            const int qv = (int)qt[b < nb - 2 ? 0 : 1][n] << 3;
            int r = c >= 0 ? (c + (qv >> 1)) / qv : -((-c + (qv >> 1)) / qv);
            if (dummy && z > 0) r = 0;
            out[i] = (short)r;
        }
    }
}

// ------------------------------------------------------------------ coefficients to bits

// `n` bits (1 .. 32; val < 2^n) at bit `pos` of a buffer whose bit 0 is the top bit of word 0
__device__ __forceinline__ void put_be(unsigned *buf, unsigned pos, unsigned val, int n)
{
    const unsigned w = pos >> 5, sh = pos & 31u;
    const unsigned long long x = ((unsigned long long)val << (64 - n)) >> sh;
    atomicOr(&buf[w], (unsigned)(x >> 32));
    const unsigned lo = (unsigned)x;
    if (lo) atomicOr(&buf[w + 1], lo);
}

__device__ __forceinline__ unsigned buf_byte(const unsigned *buf, unsigned i) { return (buf[i >> 2] >> (24u - 8u * (i & 3u))) & 255u; }

// jchuff.c's encode_one_block over 64 coefficients in zigzag order: the bits it takes; EMIT: written at bit `pos` of buf.
// A table entry is code | length << 16.  Sizes are clamped to the tables (11 for DC, 10 for AC: what 8-bit samples can reach).
template <bool EMIT>
__device__ __forceinline__ int code_block(const short *c, int pred, const unsigned *dc_code, const unsigned *ac_code, unsigned *buf, unsigned pos)
{
    int bits = 0, run = 0;
    const uint4 *src = reinterpret_cast<const uint4 *>(c);
    for (int q = 0; q < 8; ++q) {
        const uint4 v = src[q];
        const unsigned wd[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int val = (int)(short)(wd[j >> 1] >> (16 * (j & 1)));
            const bool is_dc = q == 0 && j == 0;
            if (is_dc) val -= pred;
            if (!is_dc && val == 0) {
                ++run;
                continue;
            }
            const unsigned mag = (unsigned)(val < 0 ? -val : val);
            int size = mag ? 32 - __clz(mag) : 0;
            unsigned entry;
            if (is_dc) {
                size = size > 11 ? 11 : size;
                entry = dc_code[size];
            } else {
                for (int k = 0; k < 3 && run > 15; ++k) {       // ZRL: at most 62 zeros lie before a coefficient
                    const unsigned zrl = ac_code[0xF0];
                    if (EMIT) put_be(buf, pos + (unsigned)bits, zrl & 0xffffu, (int)(zrl >> 16));
                    bits += (int)(zrl >> 16);
                    run -= 16;
                }
                size = size > 10 ? 10 : size;
                entry = ac_code[(run << 4) | size];
                run = 0;
            }
            const int len = (int)(entry >> 16) + size;
            if (EMIT) {
                const unsigned extra = (unsigned)(val < 0 ? val - 1 : val) & ((1u << size) - 1u);
                put_be(buf, pos + (unsigned)bits, ((entry & 0xffffu) << size) | extra, len);
            }
            bits += len;
        }
    }
    if (run > 0) {
        const unsigned eob = ac_code[0];
        if (EMIT) put_be(buf, pos + (unsigned)bits, eob & 0xffffu, (int)(eob >> 16));
        bits += (int)(eob >> 16);
    }
    return bits;
}

__global__ void __launch_bounds__(JPEG_LANES) k_jpeg_entropy(const short *__restrict__ coef, JpegGeom g, unsigned char *slots, IntervalMeta *meta)
{
    __shared__ unsigned buf[JPEG_BUF_WORDS];
    __shared__ unsigned dc_code[2][16], ac_code[2][256];
    __shared__ long long wsum[JPEG_LANES / 64];
    const int t = (int)threadIdx.x, interval = (int)blockIdx.x;
    for (int k = t; k < JPEG_BUF_WORDS; k += JPEG_LANES) buf[k] = 0u;
    for (int k = t; k < 512; k += JPEG_LANES) ac_code[k >> 8][k & 255] = 0u;
    if (t < 32) dc_code[t >> 4][t & 15] = 0u;
    __syncthreads();
    if (t < 4) {
        // Annex C: the codes of a table in the order of its symbols
        const int tbl = t >> 1, is_ac = t & 1;
        const unsigned char *counts = is_ac ? jpeg_ac_bits[tbl] : jpeg_dc_bits[tbl];
        unsigned *into = is_ac ? ac_code[tbl] : dc_code[tbl];
        unsigned code = 0u;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            const int count = counts[len - 1];
            for (int j = 0; j < count; ++j) {
                const int sym = is_ac ? jpeg_ac_vals[tbl][k] : k;
                into[sym] = code | ((unsigned)len << 16);
                ++code;
                ++k;
            }
            code <<= 1;
        }
    }
    __syncthreads();

    const int nb = g.blocks_per_mcu, n_blocks = g.mcu_w * nb;
    const short *blocks = coef + (long long)interval * n_blocks * 64;
    unsigned char *slot = slots + (long long)interval * g.slot_bytes;
    int done = 0, passes = 0;
    unsigned carry_bits = 0u;           // bits of an unfinished byte, at the top of buf[0]
    long long out_pos = 0, stuffed = 0;
    for (int pass = 0; pass < n_blocks && done < n_blocks; ++pass) {
        // a slab: the next JPEG_LANES blocks, or as many of them as the buffer holds (at least one: a block is 1660 bits at most)
        const int b = done + t;
        const bool have = b < n_blocks;
        int bits = 0, pred = 0, table = 0;
        if (have) {
            // the block of the same component before this one in the interval; none: the predictor is 0
            const int k = b % nb, m = b / nb;
            int prev;
            if (nb == 6) prev = k == 0 ? b - 3 : k < 4 ? b - 1 : b - 6;
            else prev = b - 3;
            if (m == 0 && !(nb == 6 && k > 0 && k < 4)) prev = -1;
            pred = prev >= 0 ? (int)blocks[(long long)prev * 64] : 0;
            table = k < nb - 2 ? 0 : 1;
            bits = code_block<false>(blocks + (long long)b * 64, pred, dc_code[table], ac_code[table], buf, 0u);
        }
        const long long before = jpeg_scan_excl((long long)bits, 0ll, JOpAdd(), wsum, nullptr);
        const bool fits = have && (long long)carry_bits + before + bits <= (long long)JPEG_BUF_BITS;
        long long taken = 0;
        (void)jpeg_scan_excl(fits ? ((long long)bits | (1ll << 32)) : 0ll, 0ll, JOpAdd(), wsum, &taken);
        const int take = (int)(taken >> 32);
        if (take == 0) break;
        if (fits) (void)code_block<true>(blocks + (long long)b * 64, pred, dc_code[table], ac_code[table], buf, carry_bits + (unsigned)before);
        unsigned n_bits = carry_bits + (unsigned)(taken & 0xffffffffll);
        __syncthreads();
        if (done + take == n_blocks && (n_bits & 7u)) {
            // the interval ends: 1-bits up to the byte
            const int pad = 8 - (int)(n_bits & 7u);
            if (t == 0) put_be(buf, n_bits, (1u << pad) - 1u, pad);
            n_bits += (unsigned)pad;
            __syncthreads();
        }
        // the whole bytes, a run of them a lane, with 0x00 behind every 0xFF
        const unsigned n_bytes = n_bits >> 3, per = (n_bytes + JPEG_LANES - 1) / JPEG_LANES;
        const unsigned lo = (unsigned)t * per < n_bytes ? (unsigned)t * per : n_bytes, hi = lo + per < n_bytes ? lo + per : n_bytes;
        int ff = 0;
        for (unsigned i = lo; i < hi; ++i) ff += buf_byte(buf, i) == 255u ? 1 : 0;
        long long ff_all = 0;
        const long long ff_before = jpeg_scan_excl((long long)ff, 0ll, JOpAdd(), wsum, &ff_all);
        unsigned char *dst = slot + out_pos + lo + ff_before;
        for (unsigned i = lo; i < hi; ++i) {
            const unsigned v = buf_byte(buf, i);
            *dst++ = (unsigned char)v;
            if (v == 255u) *dst++ = 0;
        }
        out_pos += (long long)n_bytes + ff_all;
        stuffed += ff_all;
        const unsigned left = n_bits & 7u, left_byte = left ? buf_byte(buf, n_bytes) : 0u;
        __syncthreads();
        const int used = (int)((n_bits + 31u) >> 5) + 1;
        for (int k = t; k < used && k < JPEG_BUF_WORDS; k += JPEG_LANES) buf[k] = k == 0 ? left_byte << 24 : 0u;
        __syncthreads();
        carry_bits = left;
        done += take;
        ++passes;
    }
    if (t == 0) {
        IntervalMeta m;
        m.bytes = (unsigned)out_pos;
        m.stuffed = (unsigned)stuffed;
        m.passes = (unsigned)passes;
        m.pad = 0u;
        meta[interval] = m;
    }
}

// ------------------------------------------------------------------ the file around the intervals

__global__ void __launch_bounds__(1024) k_jpeg_assemble(const IntervalMeta *__restrict__ meta, JpegGeom g, unsigned char *file, long long *offsets,
                                                        JpegInfo *info)
{
    __shared__ long long wsum[16];
    const int t = (int)threadIdx.x, n = g.mcu_h;
    const int per = (n + 1023) / 1024, c0 = t * per < n ? t * per : n, c1 = c0 + per < n ? c0 + per : n;
    long long bytes = 0, stuffed = 0, passes = 0;
    for (int c = c0; c < c1; ++c) {
        const IntervalMeta m = meta[c];
        bytes += (long long)m.bytes + 2;            // RSTm behind it, EOI behind the last
        stuffed += m.stuffed;
        passes = passes > (long long)m.passes ? passes : (long long)m.passes;
    }
    long long all_bytes = 0, all_stuffed = 0, max_passes = 0;
    long long off = jpeg_scan_excl(bytes, 0ll, JOpAdd(), wsum, &all_bytes);
    (void)jpeg_scan_excl(stuffed, 0ll, JOpAdd(), wsum, &all_stuffed);
    (void)jpeg_scan_excl(passes, 0ll, JOpMax(), wsum, &max_passes);
    for (int c = c0; c < c1; ++c) {
        offsets[c] = off;
        off += (long long)meta[c].bytes + 2;
    }
    // the tables: DQT 0 at 20, DQT 1 at 89, DHT DC 0 at 177, AC 0 at 210, DC 1 at 393, AC 1 at 426 -- 4 or 5 bytes of segment head each
    if (t < 128) file[25 + 69 * (t >> 6) + (t & 63)] = (unsigned char)quant_step(jpeg_base_q[t >> 6][jpeg_zigzag[t & 63]], g.scale);
    if (t < 16) {
        file[182 + t] = jpeg_dc_bits[0][t];
        file[215 + t] = jpeg_ac_bits[0][t];
        file[398 + t] = jpeg_dc_bits[1][t];
        file[431 + t] = jpeg_ac_bits[1][t];
    }
    if (t < 12) {
        file[198 + t] = (unsigned char)t;
        file[414 + t] = (unsigned char)t;
    }
    if (t < 162) {
        file[231 + t] = jpeg_ac_vals[0][t];
        file[447 + t] = jpeg_ac_vals[1][t];
    }
    if (t == 0) {
        const unsigned char hv = g.blocks_per_mcu == 6 ? 0x22 : 0x11;
        const unsigned char app0[20] = { 0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 };
        for (int k = 0; k < 20; ++k) file[k] = app0[k];
        for (int q = 0; q < 2; ++q) {
            unsigned char *d = file + 20 + 69 * q;
            d[0] = 0xFF; d[1] = 0xDB; d[2] = 0; d[3] = 67; d[4] = (unsigned char)q;
        }
        const unsigned char sof[19] = { 0xFF, 0xC0, 0, 17, 8, (unsigned char)(g.rows >> 8), (unsigned char)g.rows, (unsigned char)(g.width >> 8),
                                        (unsigned char)g.width, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1 };
        for (int k = 0; k < 19; ++k) file[158 + k] = sof[k];
        const int dht_at[4] = { 177, 210, 393, 426 };
        for (int q = 0; q < 4; ++q) {
            unsigned char *d = file + dht_at[q];
            const int len = (q & 1) ? 2 + 1 + 16 + 162 : 2 + 1 + 16 + 12;
            d[0] = 0xFF; d[1] = 0xC4; d[2] = (unsigned char)(len >> 8); d[3] = (unsigned char)len;
            d[4] = (unsigned char)(((q & 1) << 4) | (q >> 1));
        }
        const unsigned char tail[20] = { 0xFF, 0xDD, 0, 4, (unsigned char)(g.mcu_w >> 8), (unsigned char)g.mcu_w,
                                         0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 };
        for (int k = 0; k < 20; ++k) file[609 + k] = tail[k];
        info->jpeg_bytes = JPEG_HEAD + all_bytes;
        info->scan_bytes = all_bytes - 2;
        info->stuffed_bytes = all_stuffed;
        info->passes_max = (int)max_passes;
    }
}

__global__ void __launch_bounds__(256) k_jpeg_place(const unsigned char *__restrict__ slots, const IntervalMeta *__restrict__ meta,
                                                    const long long *__restrict__ offsets, JpegGeom g, unsigned char *file)
{
    const int interval = (int)blockIdx.x;
    const unsigned char *src = slots + (long long)interval * g.slot_bytes;
    unsigned char *dst = file + JPEG_HEAD + offsets[interval];
    const long long bytes = (long long)meta[interval].bytes;        // at most slot_bytes
    for (long long k = threadIdx.x; k < bytes; k += 256) dst[k] = src[k];
    if (threadIdx.x == 0) {
        dst[bytes] = 0xFF;
        dst[bytes + 1] = interval + 1 < g.mcu_h ? (unsigned char)(0xD0 + (interval & 7)) : (unsigned char)0xD9;
    }
}

// ------------------------------------------------------------------ host

// Checks size and parameters (who: the entry point's name, for the error text; null: no text) and fills the geometry.
int geometry(const char *who, int32_t width, int32_t rows, const ndt_jpeg_params *jp, JpegGeom *g)
{
#define JPEG_REFUSE(...) return who ? fail(NDT_E_INVALID, __VA_ARGS__) : NDT_E_INVALID
    if (width < 1 || rows < 1) JPEG_REFUSE("%s: a %d x %d image", who, width, rows);
    if (width > 65535 || rows > 65535) JPEG_REFUSE("%s: a %d x %d image: SOF0 holds dimensions up to 65535", who, width, rows);
    const int quality = jp && jp->quality ? jp->quality : 95, sampling = jp ? jp->sampling : 0;
    if (quality < 1 || quality > 100) JPEG_REFUSE("%s: quality %d is outside 1 .. 100", who, quality);
    if (sampling < 0 || sampling > 1) JPEG_REFUSE("%s: sampling %d is neither 0 (4:2:0) nor 1 (4:4:4)", who, sampling);
    if (jp && (jp->reserved[0] || jp->reserved[1])) JPEG_REFUSE("%s: the reserved words of ndt_jpeg_params must be 0", who);
#undef JPEG_REFUSE
    g->width = width;
    g->rows = rows;
    g->scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    g->side = sampling == 0 ? 16 : 8;
    g->blocks_per_mcu = sampling == 0 ? 6 : 3;
    g->mcu_w = (width + g->side - 1) / g->side;
    g->mcu_h = (rows + g->side - 1) / g->side;
    g->aligned = 0;
    // an interval with its padding, every byte stuffed (the file's bound: the head of this file)
    g->slot_bytes = 2 * (((long long)g->mcu_w * g->blocks_per_mcu * JPEG_BLOCK_BITS + 7 + 7) / 8);
    return NDT_OK;
}

long long file_bound(const JpegGeom &g) { return JPEG_HEAD + (long long)g.mcu_h * (g.slot_bytes + 2) + 2; }

} // namespace

extern "C" int64_t ndt_hip_jpeg_bound(int32_t width, int32_t rows, const ndt_jpeg_params *jp)
{
    JpegGeom g;
    if (geometry(nullptr, width, rows, jp, &g) != NDT_OK) return NDT_E_INVALID;
    return file_bound(g);
}

void ndt_impl::free_jpeg(ndt_hip_ctx *ctx)
{
    JpegState &js = ctx->jpeg;
    js.d_rgba8.release();
    js.d_coef.release();
    js.d_slots.release();
    js.d_meta.release();
    js.d_offsets.release();
    js.d_file.release();
    js.d_info.release();
    if (js.h_info) (void)hipHostFree(js.h_info);
    js = JpegState();
}

extern "C" int ndt_hip_encode_jpeg_device(ndt_hip_ctx *ctx, const void *d_rgba8, int32_t width, int32_t rows, const ndt_jpeg_params *jp,
                                          uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats)
{
    if (!ctx || !d_rgba8 || !jpg) return fail(NDT_E_INVALID, "ndt_hip_encode_jpeg: NULL argument");
    JpegGeom g;
    int rc;
    if ((rc = geometry("ndt_hip_encode_jpeg", width, rows, jp, &g))) return rc;
    if (cap < 0) return fail(NDT_E_INVALID, "ndt_hip_encode_jpeg: cap %lld", (long long)cap);
    if (((uintptr_t)d_rgba8 & 3u) != 0) return fail(NDT_E_INVALID, "ndt_hip_encode_jpeg: the image is not aligned to its 4-byte pixels");
    g.aligned = ((uintptr_t)d_rgba8 & 15u) == 0 && width % 4 == 0;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(ctx->device));
    JpegState &js = ctx->jpeg;
    const int n_mcus = g.mcu_w * g.mcu_h;           // at most 8192 x 8192
    const long long bound = file_bound(g);
    if ((rc = js.d_coef.reserve((size_t)n_mcus * g.blocks_per_mcu * 64 * sizeof(short), ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    if ((rc = js.d_slots.reserve((size_t)g.mcu_h * (size_t)g.slot_bytes, ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    if ((rc = js.d_meta.reserve((size_t)g.mcu_h * sizeof(IntervalMeta), ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    if ((rc = js.d_offsets.reserve((size_t)g.mcu_h * sizeof(long long), ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    if ((rc = js.d_file.reserve((size_t)bound, ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    if ((rc = js.d_info.reserve(sizeof(JpegInfo), ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    if (!js.h_info) HIP_TRY(hipHostMalloc(&js.h_info, sizeof(JpegInfo), hipHostMallocDefault));
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_jpeg_blocks, dim3((unsigned)((n_mcus + 3) / 4)), dim3(256), 0, s, (const unsigned *)d_rgba8, g, js.d_coef.as<short>());
    hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)g.mcu_h), dim3(JPEG_LANES), 0, s, js.d_coef.as<const short>(), g, js.d_slots.as<unsigned char>(),
                       js.d_meta.as<IntervalMeta>());
    hipLaunchKernelGGL(k_jpeg_assemble, dim3(1), dim3(1024), 0, s, js.d_meta.as<const IntervalMeta>(), g, js.d_file.as<unsigned char>(),
                       js.d_offsets.as<long long>(), js.d_info.as<JpegInfo>());
    hipLaunchKernelGGL(k_jpeg_place, dim3((unsigned)g.mcu_h), dim3(256), 0, s, js.d_slots.as<const unsigned char>(), js.d_meta.as<const IntervalMeta>(),
                       js.d_offsets.as<const long long>(), g, js.d_file.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(js.h_info, js.d_info.p, sizeof(JpegInfo), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const JpegInfo info = *(const JpegInfo *)js.h_info;
    if (stats) {
        *stats = ndt_jpeg_stats{};
        stats->jpeg_bytes = info.jpeg_bytes;
        stats->scan_bytes = info.scan_bytes;
        stats->stuffed_bytes = info.stuffed_bytes;
        stats->mcus = n_mcus;
        stats->intervals = g.mcu_h;
        stats->launches = 4;
        stats->passes_max = info.passes_max;
    }
    if (info.jpeg_bytes < JPEG_HEAD + 2 || info.jpeg_bytes > bound)
        return fail(NDT_E_DEVICE, "ndt_hip_encode_jpeg: the device reports a file of %lld bytes (bound %lld)", info.jpeg_bytes, bound);
    if (info.jpeg_bytes > cap)
        return fail(NDT_E_NOMEM, "ndt_hip_encode_jpeg: the file is %lld bytes, the buffer %lld", info.jpeg_bytes, (long long)cap);
    HIP_TRY(hipMemcpyAsync(jpg, js.d_file.p, (size_t)info.jpeg_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (stats) stats->encode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return NDT_OK;
}

extern "C" int ndt_hip_encode_jpeg(ndt_hip_ctx *ctx, const uint8_t *rgba8, int32_t width, int32_t rows, const ndt_jpeg_params *jp, uint8_t *jpg,
                                   int64_t cap, ndt_jpeg_stats *stats)
{
    if (!ctx || !rgba8 || !jpg) return fail(NDT_E_INVALID, "ndt_hip_encode_jpeg: NULL argument");
    JpegGeom g;
    int rc;
    if ((rc = geometry("ndt_hip_encode_jpeg", width, rows, jp, &g))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)width * (size_t)rows * 4;
    if ((rc = ctx->jpeg.d_rgba8.reserve(bytes, ctx->stream, "ndt_hip_encode_jpeg"))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->jpeg.d_rgba8.p, rgba8, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ndt_hip_encode_jpeg_device(ctx, ctx->jpeg.d_rgba8.p, width, rows, jp, jpg, cap, stats);
}

extern "C" int ndt_hip_render_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_jpeg_params *jp, uint8_t *jpg, int64_t cap,
                                   ndt_jpeg_stats *stats, ndt_render_stats *render_stats)
{
    if (!ctx || !p || !jpg) return fail(NDT_E_INVALID, "ndt_hip_render_jpeg: NULL argument");
    if (p->width < 1 || p->height < 1 || p->row_step < 1 || p->row_begin < 0) return fail(NDT_E_INVALID, "bad geometry");
    const int rows = ndt_hip_shard_rows(p->height, p->row_begin, p->row_step);
    JpegGeom g;
    int rc;
    if ((rc = refuse_empty_shard("ndt_hip_render_jpeg", rows)) || (rc = geometry("ndt_hip_render_jpeg", p->width, rows, jp, &g))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ctx->jpeg.d_rgba8.reserve((size_t)p->width * (size_t)rows * 4, ctx->stream, "ndt_hip_render_jpeg"))) return rc;
    ndt_hip_ctx *one[1] = { ctx };
    if ((rc = ndt_hip_render_multi_device(one, 1, p, NDT_IMAGE_RGBA8, ctx->jpeg.d_rgba8.p, render_stats))) return rc;
    return ndt_hip_encode_jpeg_device(ctx, ctx->jpeg.d_rgba8.p, p->width, rows, jp, jpg, cap, stats);
}
