// ndt_deflate.hpp -- the deflate the file sinks share (ndt_png.hip: the PNG's one stream; ndt_exr.hip: a stream per block of
// scanlines): one workgroup compresses an independent 32 KiB chunk of a byte stream with matches at one distance (1 for the PNG, 2
// for the OpenEXR blocks) and a dynamic Huffman code of its own, the bits packed into an LDS image with ds_or; a chunk the code
// does not shrink is stored; every chunk but the
// last of its stream ends on a byte boundary (an empty stored block: 00 00 FF FF).  With it the workgroup scans it is built on and
// the chunk's Adler-32 pair, from which the stream's checksum is folded.  Device code; each translation unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int PNG_CHUNK = 32768;                // bytes of the stream a workgroup compresses
constexpr int PNG_SLOT = PNG_CHUNK + 64;        // a chunk's output slot: the stored form is 5 + 32768 bytes
constexpr int PNG_SPAN = 32;                    // bytes of the chunk a lane holds in registers
constexpr int PNG_DEFLATE_LANES = PNG_CHUNK / PNG_SPAN;
constexpr int PNG_LITLEN = 286;                 // literal / length alphabet
constexpr unsigned ADLER_MOD = 65521u;

struct ChunkMeta { unsigned bytes, stored, s1, s2; };   // s1, s2: the chunk's Adler pair from (0, 0), mod 65521

// the order the header lists the code-length code's own lengths in
__constant__ int cl_order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

// ------------------------------------------------------------------ workgroup scans

// exclusive scan over the workgroup's lanes, from the lower lanes (DIR > 0) or the higher ones (DIR < 0); `op` commutes.
// Every lane calls it; *total (may be null) gets the fold over all lanes.
template <int DIR, typename Op>
__device__ __forceinline__ long long block_scan_excl(long long v, long long identity, Op op, long long *wsum, long long *total)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = DIR > 0 ? __shfl_up(x, d, 64) : __shfl_down(x, d, 64);
        if (DIR > 0 ? lane >= d : lane + d < 64) x = op(x, o);
    }
    if (lane == (DIR > 0 ? 63 : 0)) wsum[wave] = x;
    long long prev = DIR > 0 ? __shfl_up(x, 1, 64) : __shfl_down(x, 1, 64);
    if (DIR > 0 ? lane == 0 : lane == 63) prev = identity;
    __syncthreads();
    long long carry = identity, all = identity;
    for (int w = 0; w < n_waves; ++w) {
        const long long s = wsum[w];
        all = op(all, s);
        if (DIR > 0 ? w < wave : w > wave) carry = op(carry, s);
    }
    __syncthreads();
    if (total) *total = all;
    return op(carry, prev);
}

struct OpAdd { __device__ long long operator()(long long a, long long b) const { return a + b; } };
struct OpMax { __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; } };
struct OpMin { __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; } };

// ------------------------------------------------------------------ Huffman codes of a chunk

struct HuffScratch {
    unsigned weight[2 * 288];       // leaves in ascending order [0, n), the nodes the merge makes [n, 2n - 1)
    short parent[2 * 288];
    short sorted_sym[288];
    int num[16], next[16];          // codes per length, first code per length
    int n_used;
};

// A length-limited Huffman code for freq[0 .. n_sym): code[s] = bit-reversed code | length << 16, 0 for an unused symbol.
// Called by every lane of the workgroup (n_sym <= 288 <= lanes).  Lengths come from the two-queue merge over the symbols in
// ascending order (one lane), overlong codes are pulled in the way every Kraft-sum repair does, and the lengths are dealt
// shortest-to-most-frequent.  An alphabet with one used symbol gets a second code, so that the set is complete.
__device__ void huff_build(const unsigned *freq, int n_sym, int max_bits, unsigned *code, HuffScratch &hs)
{
    const int t = (int)threadIdx.x;
    if (t < 16) hs.num[t] = 0;
    if (t == 0) hs.n_used = 0;
    __syncthreads();
    const unsigned f = t < n_sym ? freq[t] : 0u;
    int rank = 0;
    if (f) {
        for (int j = 0; j < n_sym; ++j) {
            const unsigned fj = freq[j];
            rank += (fj && (fj < f || (fj == f && j < t))) ? 1 : 0;
        }
        atomicAdd(&hs.n_used, 1);
    }
    __syncthreads();
    const int n = hs.n_used;
    if (f) {
        hs.sorted_sym[rank] = (short)t;
        hs.weight[rank] = f;
    }
    if (t < n_sym) code[t] = 0u;
    __syncthreads();
    if (n < 2) {
        if (t == 0 && n == 1) {
            const int s = hs.sorted_sym[0], other = s == 0 ? 1 : 0;
            code[s < other ? s : other] = 0u | (1u << 16);
            code[s < other ? other : s] = 1u | (1u << 16);
        }
        __syncthreads();
        return;
    }
    if (t == 0) {
        int leaf = 0, node = n, made = n;
        for (int step = 0; step < n - 1; ++step) {
            int pick[2];
            for (int k = 0; k < 2; ++k) {
                if (leaf < n && (node >= made || hs.weight[leaf] <= hs.weight[node])) pick[k] = leaf++;
                else pick[k] = node++;
            }
            hs.weight[made] = hs.weight[pick[0]] + hs.weight[pick[1]];
            hs.parent[pick[0]] = (short)made;
            hs.parent[pick[1]] = (short)made;
            ++made;
        }
    }
    __syncthreads();
    if (t < n) {
        int at = t, depth = 0;
        for (int it = 0; it < n && at != 2 * n - 2; ++it) {
            at = hs.parent[at];
            ++depth;
        }
        atomicAdd(&hs.num[depth < max_bits ? depth : max_bits], 1);
    }
    __syncthreads();
    if (t == 0) {
        int total = 0;
        for (int l = 1; l <= max_bits; ++l) total += hs.num[l] << (max_bits - l);
        for (int it = 0; it < 288 && total > (1 << max_bits); ++it) {
            hs.num[max_bits] -= 1;
            for (int l = max_bits - 1; l >= 1; --l)
                if (hs.num[l]) {
                    hs.num[l] -= 1;
                    hs.num[l + 1] += 2;
                    break;
                }
            --total;
        }
        int c = 0;
        hs.next[0] = 0;
        for (int l = 1; l <= max_bits; ++l) {
            c = (c + (l > 1 ? hs.num[l - 1] : 0)) << 1;
            hs.next[l] = c;
        }
    }
    __syncthreads();
    int len = 0;
    if (f) {
        const int place = n - 1 - rank;         // 0: the most frequent symbol
        int cum = 0;
        for (int l = 1; l <= max_bits; ++l) {
            cum += hs.num[l];
            if (place < cum) { len = l; break; }
        }
        code[t] = (unsigned)len << 16;
    }
    __syncthreads();
    unsigned mine = 0u;
    if (len) {
        int before = 0;
        for (int j = 0; j < t; ++j) before += ((int)(code[j] >> 16) == len) ? 1 : 0;
        const unsigned c = (unsigned)(hs.next[len] + before);
        mine = (__brev(c) >> (32 - len)) | ((unsigned)len << 16);
    }
    __syncthreads();
    if (t < n_sym) code[t] = mine;
    __syncthreads();
}

// ------------------------------------------------------------------ a chunk's tokens

// length 3 .. 258 -> symbol 257 .. 285, number of extra bits and their value
__device__ __forceinline__ int length_symbol(int len, int &extra_bits, int &extra)
{
    if (len == 258) { extra_bits = 0; extra = 0; return 285; }
    const int l = len - 3;
    if (l < 8) { extra_bits = 0; extra = 0; return 257 + l; }
    const int eb = (31 - __clz(l)) - 2;
    extra_bits = eb;
    extra = l & ((1 << eb) - 1);
    return 257 + 4 * eb + 4 + ((l >> eb) & 3);
}

// What byte j of this lane's span becomes: 0 nothing (inside a match), 1 a literal, 2 a match of `len` bytes at the chunk's one
// match distance D (1: the PNG's stream; 2: the OpenEXR blocks', whose two byte planes give float samples a period of 2).
// A run -- a byte that differs from the byte D before it, then k - 1 that equal theirs -- is one literal and matches over the other
// k - 1 bytes in pieces of 258; a last piece under 3 bytes is literals.
// heads: bit j = byte j differs from the byte D before it; run_start / run_end: where the runs open at the span's ends begin and end.
__device__ __forceinline__ int token_at(int j, unsigned heads, int span0, int run_start, int run_end, int &len)
{
    const unsigned below = heads & ((2u << j) - 1u);
    const unsigned above = j < 31 ? heads >> (j + 1) : 0u;
    const int i = span0 + j;
    const int s = below ? span0 + 31 - __clz(below) : run_start;
    const int e = above ? i + 1 + (__ffs(above) - 1) : run_end;
    const int o = i - s, m = e - s - 1;
    if (o == 0 || m < 3) return 1;
    const int q = o - 1, piece = q / 258, r = q - piece * 258;
    const int left = m - piece * 258;
    len = left < 258 ? left : 258;
    if (len < 3) return 1;
    return r == 0 ? 2 : 0;
}

__device__ __forceinline__ void put_bits(unsigned *image, unsigned pos, unsigned val, int n_bits)
{
    const unsigned w = pos >> 5, sh = pos & 31u;
    atomicOr(&image[w], val << sh);
    if ((int)sh + n_bits > 32) atomicOr(&image[w + 1], val >> (32u - sh));
}

// MODE 0: histogram of the span's tokens; 1: their bits; 2: the bits themselves at bit position `pos`.  Returns the bits.
template <int MODE>
__device__ __forceinline__ int walk_span(const unsigned (&w)[8], int valid, unsigned heads, int span0, int run_start, int run_end,
                                         unsigned *ll_freq, const unsigned *ll_code, unsigned *image, unsigned pos, int *any_match)
{
    int bits = 0;
    bool matched = false;
#pragma unroll
    for (int j = 0; j < PNG_SPAN; ++j) {
        if (j < valid) {
            const unsigned b = (w[j >> 2] >> (8 * (j & 3))) & 255u;
            int len = 0;
            const int kind = token_at(j, heads, span0, run_start, run_end, len);
            if (kind == 1) {
                if (MODE == 0) atomicAdd(&ll_freq[b], 1u);
                else {
                    const unsigned c = ll_code[b];
                    if (MODE == 2) put_bits(image, pos + (unsigned)bits, c & 0xffffu, (int)(c >> 16));
                    bits += (int)(c >> 16);
                }
            } else if (kind == 2) {
                int eb, ev;
                const int sym = length_symbol(len, eb, ev);
                if (MODE == 0) {
                    atomicAdd(&ll_freq[sym], 1u);
                    matched = true;
                } else {
                    const unsigned c = ll_code[sym];
                    const int cl = (int)(c >> 16), nb = cl + eb + 1;        // + the one distance code: '0'
                    if (MODE == 2) put_bits(image, pos + (unsigned)bits, (c & 0xffffu) | ((unsigned)ev << cl), nb);
                    bits += nb;
                }
            }
        }
    }
    if (MODE == 0 && matched) atomicOr(any_match, 1);
    return bits;
}

// The workgroup's chunk: the n <= PNG_CHUNK bytes at `chunk` (aligned to 16 bytes; PNG_CHUNK bytes of the buffer can be read
// there, and bytes from n on are never looked at) compressed into `slot_bytes` (PNG_SLOT bytes, aligned to 4), its record into
// *meta.  `last`: the chunk ends its stream.  DIST: the match distance, 1 or 2 -- the block's distance code is its only one, one bit
// long (a single distance code of length one is what the format allows an incomplete code for).  Called by all PNG_DEFLATE_LANES
// lanes of the workgroup.
template <int DIST>
__device__ __forceinline__ void deflate_chunk(const unsigned char *__restrict__ chunk, int n, bool last, unsigned char *slot_bytes, ChunkMeta *meta)
{
    __shared__ unsigned image[PNG_SLOT / 4];
    __shared__ unsigned ll_freq[288], ll_code[288];
    __shared__ unsigned cl_freq[20], cl_code[20];
    __shared__ unsigned short cl_tok[296];          // code-length symbol | extra << 5
    __shared__ HuffScratch hs;
    __shared__ long long wsum[16];
    __shared__ int any_match, n_cl, n_hclen, n_hlit;
    __shared__ unsigned long long adler_sum[2];

    const int t = (int)threadIdx.x;
    const int span0 = t * PNG_SPAN;
    const int valid = n - span0 < 0 ? 0 : n - span0 > PNG_SPAN ? PNG_SPAN : n - span0;

    // the lane's 32 bytes (the buffer is whole chunks long: the loads stay inside it; bytes from n on are never looked at)
    unsigned w[8];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(chunk) + 2 * t;
        const uint4 a = src[0], b = src[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    }
    static_assert(DIST == 1 || DIST == 2, "the match distance");
    unsigned before[DIST];                                              // the DIST bytes in front of byte j, the oldest first
#pragma unroll
    for (int d = 0; d < DIST; ++d) before[d] = t > 0 ? (unsigned)chunk[span0 - DIST + d] : 0x100u;     // the chunk's first DIST bytes head runs

    for (int k = t; k < PNG_SLOT / 4; k += PNG_DEFLATE_LANES) image[k] = 0u;
    if (t < 288) ll_freq[t] = t == 256 ? 1u : 0u;                                  // one end-of-block
    if (t < 20) cl_freq[t] = 0u;
    if (t == 0) { any_match = 0; adler_sum[0] = 0ull; adler_sum[1] = 0ull; }

    unsigned heads = 0u, sum = 0u, wsum_bytes = 0u;
#pragma unroll
    for (int j = 0; j < PNG_SPAN; ++j) {
        const unsigned b = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        if (j < valid) {
            if (b != before[0]) heads |= 1u << j;
            sum += b;
            wsum_bytes += (unsigned)(valid - j) * b;
        }
#pragma unroll
        for (int d = 0; d + 1 < DIST; ++d) before[d] = before[d + 1];
        before[DIST - 1] = b;
    }
    __syncthreads();

    // Adler-32 of the chunk from (0, 0): s1 = sum of bytes, s2 = sum of (n - i) * byte i
    {
        unsigned long long a = sum, b2 = (unsigned long long)wsum_bytes + (unsigned long long)(n - span0 - valid) * sum;
        if (valid == 0) { a = 0ull; b2 = 0ull; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            a += __shfl_down(a, d, 64);
            b2 += __shfl_down(b2, d, 64);
        }
        if ((t & 63) == 0) {
            atomicAdd(&adler_sum[0], a);
            atomicAdd(&adler_sum[1], b2);
        }
    }

    // where the run open at the span's first byte began, and where the one open at its last byte ends
    const long long my_last = heads ? (long long)(span0 + 31 - __clz(heads)) : -1ll;
    const long long my_first = heads ? (long long)(span0 + __ffs(heads) - 1) : (long long)n;
    const int run_start = (int)block_scan_excl<1>(my_last, -1ll, OpMax(), wsum, nullptr);
    const int run_end = (int)block_scan_excl<-1>(my_first, (long long)n, OpMin(), wsum, nullptr);

    walk_span<0>(w, valid, heads, span0, run_start, run_end, ll_freq, ll_code, image, 0u, &any_match);
    __syncthreads();
    huff_build(ll_freq, PNG_LITLEN, 15, ll_code, hs);

    // the code lengths of the header, run-length coded with symbols 16 / 17 / 18 (one lane; at most 287 lengths)
    if (t == 0) {
        int hl = PNG_LITLEN;
        for (int k = 0; k < 29 && (ll_code[hl - 1] >> 16) == 0u; ++k) --hl;       // symbol 256 is used: hl >= 257
        n_hlit = hl;
        // the lengths the header lists: hl literal / length codes, then DIST distance codes of which the last is the one in use
        const int total = hl + DIST, dist_len = any_match ? 1 : 0;
        auto len_at = [&](int k) { return k < hl ? (int)(ll_code[k] >> 16) : k == total - 1 ? dist_len : 0; };
        int i = 0, count = 0;
        for (int it = 0; it < 288 && i < total; ++it) {
            const int v = len_at(i);
            int run = 1;
            for (int k = 1; k < 138 && i + k < total; ++k) {
                const int u = len_at(i + k);
                if (u != v) break;
                ++run;
            }
            int sym, extra = 0, used = 1;
            if (v == 0 && run >= 11) { sym = 18; extra = run - 11; used = run; }
            else if (v == 0 && run >= 3) { sym = 17; extra = run - 3; used = run; }
            else if (v != 0 && it > 0 && run >= 3 && i > 0 && len_at(i - 1) == v) {
                used = run < 6 ? run : 6;
                sym = 16;
                extra = used - 3;
            } else sym = v;
            cl_tok[count++] = (unsigned short)(sym | (extra << 5));
            cl_freq[sym] += 1u;
            i += used;
        }
        n_cl = count;
    }
    __syncthreads();
    huff_build(cl_freq, 19, 7, cl_code, hs);
    if (t == 0) {
        int h = 19;
        for (int k = 0; k < 15 && (cl_code[cl_order[h - 1]] >> 16) == 0u; ++k) --h;
        n_hclen = h;
    }
    __syncthreads();
    const int hclen = n_hclen, hlit = n_hlit, n_tok = n_cl;

    // bit positions: header tokens, then the data tokens, then end-of-block
    int cl_bits = 0;
    unsigned cl_val = 0u;
    if (t < n_tok) {
        const int tok = cl_tok[t], sym = tok & 31, extra = tok >> 5;
        const unsigned c = cl_code[sym];
        const int eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        cl_bits = (int)(c >> 16) + eb;
        cl_val = (c & 0xffffu) | ((unsigned)extra << (c >> 16));
    }
    long long cl_total = 0, tok_total = 0;
    const int cl_pos = (int)block_scan_excl<1>((long long)cl_bits, 0ll, OpAdd(), wsum, &cl_total);
    const int header_bits = 3 + 5 + 5 + 4 + 3 * hclen + (int)cl_total;
    const int my_bits = walk_span<1>(w, valid, heads, span0, run_start, run_end, ll_freq, ll_code, image, 0u, &any_match);
    const int my_pos = (int)block_scan_excl<1>((long long)my_bits, 0ll, OpAdd(), wsum, &tok_total);
    const long long block_bits = (long long)header_bits + tok_total + (long long)(ll_code[256] >> 16);
    // the block, then -- but for the last chunk -- an empty stored block: 3 bits, padding to a byte, 00 00 FF FF
    const long long packed_bytes = last ? (block_bits + 7) >> 3 : ((block_bits + 3 + 7) >> 3) + 4;
    const int stored_bytes = 5 + n;
    const bool stored = packed_bytes >= (long long)stored_bytes;
    int out_bytes;
    if (!stored) {
        out_bytes = (int)packed_bytes;
        if (t == 0) put_bits(image, 0u, (last ? 1u : 0u) | (2u << 1) | ((unsigned)(hlit - 257) << 3) | ((unsigned)(DIST - 1) << 8) | ((unsigned)(hclen - 4) << 13), 17);
        if (t < hclen) put_bits(image, 17u + 3u * (unsigned)t, cl_code[cl_order[t]] >> 16, 3);
        if (t < n_tok) put_bits(image, 17u + 3u * (unsigned)hclen + (unsigned)cl_pos, cl_val, cl_bits);
        walk_span<2>(w, valid, heads, span0, run_start, run_end, ll_freq, ll_code, image, (unsigned)header_bits + (unsigned)my_pos, &any_match);
        if (t == 0) {
            const unsigned eob = ll_code[256];
            put_bits(image, (unsigned)(block_bits - (long long)(eob >> 16)), eob & 0xffffu, (int)(eob >> 16));
            if (!last) put_bits(image, 8u * (unsigned)(out_bytes - 2), 0xffffu, 16);
        }
    } else {
        // one stored block: BFINAL, LEN, NLEN, the bytes as they are
        out_bytes = stored_bytes;
        if (t == 0) {
            const unsigned len = (unsigned)n & 0xffffu, nlen = ~len & 0xffffu;          // n = 32768 fits LEN
            put_bits(image, 0u, (last ? 1u : 0u) | (len << 8) | ((nlen & 0xffu) << 24), 32);
            put_bits(image, 32u, nlen >> 8, 8);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int have = valid - 4 * k;             // bytes of this word inside the chunk
            if (have > 0) {
                const unsigned x = have >= 4 ? w[k] : w[k] & ((1u << (8 * have)) - 1u);
                put_bits(image, 8u * (unsigned)(5 + span0 + 4 * k), x, 32);
            }
        }
    }
    __syncthreads();
    unsigned *slot = reinterpret_cast<unsigned *>(slot_bytes);
    const int words = (out_bytes + 3) >> 2;
    for (int k = t; k < words; k += PNG_DEFLATE_LANES) slot[k] = image[k];
    if (t == 0) {
        ChunkMeta m;
        m.bytes = (unsigned)out_bytes;
        m.stored = stored ? 1u : 0u;
        m.s1 = (unsigned)(adler_sum[0] % ADLER_MOD);
        m.s2 = (unsigned)(adler_sum[1] % ADLER_MOD);
        *meta = m;
    }
}

} // namespace
