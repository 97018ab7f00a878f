// ofd_deflate.hip -- MI355X (gfx950) DEFLATE encoder for the npz product.
//
// preprocess.py writes its product with np.savez_compressed (:446, :471-476):
// a zip of .npy members, each deflated by zlib on the host.  Per image that
// is 121 files and ~6.3 GB of float64 planes at 768x1024, and host zlib (one
// core per file) bounds the whole pipeline.  This file deflates the arrays on
// the GPU, where they already are, into streams any inflater (zlib, Python's
// zipfile, np.load) reads:
//
//   * every array is cut into 1 MiB SEGMENTS; each segment is one dynamic-
//     Huffman deflate block, closed by an empty stored block (zlib's
//     Z_SYNC_FLUSH marker 00 00 FF FF), so every segment ends on a byte
//     boundary and the segments concatenate;
//   * the array's stream ends with an empty final fixed block (03 00);
//   * CRC-32 (zlib's polynomial) of every array, for the zip headers.
//
// Two modes share every kernel; they differ in how a thread's 64-byte span
// becomes tokens and in the width of the symbol tables:
//   literal (ofd_deflate_batch)  every byte is a literal: 256 byte symbols +
//          end of block.  f64 planes of f32 / integer values are dominated
//          by zero bytes, which a per-segment code prices at about one bit.
//   match (ofd_deflate_lz_batch, opt-in)  every thread parses its span
//          greedily for runs equal to the bytes 1, E or 2E back (E = the
//          element size): 286 literal / length and 30 distance symbols.
//
// Kernels (all on the caller's stream, no host synchronisation):
//   HIST   one workgroup per 16 KiB chunk: the histogram of the chunk's
//          symbols (kept per chunk and added into its segment's), its
//          matches' extra bits, and the chunk's CRC-32 (a table CRC per
//          thread over 64 bytes, folded by x^(8n) mod P).
//   CODE   one workgroup per segment: the Huffman code lengths (max 15; the
//          frequencies are flattened and the tree rebuilt until it fits) of
//          the literal / length tree and, if the segment has a match, the
//          distance tree, the canonical codes, the block header (code-length
//          code, HLIT literal / length lengths, HDIST distance lengths: 257
//          and one zero length without a match), the segment's size in
//          bytes, every chunk's bit offset, the segment CRC.
//   SCAN   one thread per array: segment offsets, the array's size, its CRC,
//          the final block.
//   ENCODE one workgroup per chunk: the same tokens again, per-thread bit
//          counts, a block scan, then every thread packs its codes into
//          32-bit words of the (zeroed) output; the chunk holding a segment's
//          start writes the header, the one holding its end the end-of-block
//          code and FF FF.
//
// Plain HIP for gfx950.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <utility>

#include "ofd_deflate.h"
#include "ofd_fw.h"

namespace {

constexpr int kThr = 256;
constexpr int64_t kChunk = 16384;               // bytes per HIST / ENCODE workgroup
constexpr int kPerThr = int(kChunk / kThr);     // 64 bytes per thread
constexpr int64_t kSeg = int64_t(1) << 20;      // bytes per deflate block
constexpr int kChunksPerSeg = int(kSeg / kChunk);
constexpr int kSym = 257;                       // literals 0..255 + end of block
constexpr int kLSym = 286;                      // ... + 29 length symbols
constexpr int kDSym = 30;                       // distance symbols
constexpr int kDOff = kLSym;                    // the distance symbols follow in the joint tables ...
constexpr int kAll = 320;                       // ... of 316 entries, padded
constexpr int kMaxLen = 15;
constexpr int kMinMatch = 3;
constexpr int kCandDefault = 3;                 // bit 0: distance 1, bit 1: distance 2E (E itself always)
constexpr int kHdrWords = 80;                   // block header words
constexpr uint32_t kPoly = 0xEDB88320u;         // CRC-32, reflected
static_assert(kPerThr == 64, "a span's equality masks are 64-bit");
// BFINAL BTYPE HLIT HDIST HCLEN, 19 code-length-code lengths, 316 lengths of <= 7 bits: 2283 bits (match mode)
static_assert(14 + 19 * 3 + (kLSym + kDSym) * 7 <= kHdrWords * 32, "the block header must fit kHdrWords");

// Table widths of a mode: symbol counts per chunk and per segment, codes per
// segment.  The literal mode keeps no count for the end of block (one per
// segment) and none for the match symbols it never codes.
constexpr int hist_width(bool match) { return match ? kAll : 256; }
constexpr int code_width(bool match) { return match ? kAll : kSym; }

int g_lz_cand = kCandDefault;

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// ---------------------------------------------------------------- CRC-32 algebra (zlib's multmodp / x2nmodp)
__host__ __device__ inline uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P: the operator that shifts a CRC past n more bytes
__host__ __device__ inline uint32_t x8nmodp(uint64_t n) {
    uint32_t p = 1u << 31;     // x^0
    uint32_t sq = 1u << 23;    // x^8
    while (n) {
        if (n & 1) p = multmodp(sq, p);
        sq = multmodp(sq, sq);
        n >>= 1;
    }
    return p;
}

// crc(A || B) from crc(A), crc(B) and |B|
__host__ __device__ inline uint32_t crc_combine(uint32_t ca, uint32_t cb, uint64_t lenb) {
    return multmodp(x8nmodp(lenb), ca) ^ cb;
}

struct Geo {        // one batch of `count` arrays of `each` bytes
    int64_t each;   // bytes per array
    int cpa;        // chunks per array
    int spa;        // segments per array
    int64_t bound;  // output slot per array
};

struct DWs {
    uint16_t *chist;   // [chunks][hist_width]
    uint32_t *ccrc;    // [chunks]
    uint32_t *cxb;     // [chunks] extra bits of the chunk's matches (match mode only)
    uint64_t *cbit;    // [chunks] bit offset of the chunk's first code from the segment start
    uint32_t *shist;   // [segs][hist_width]  (zeroed per call)
    uint32_t *scode;   // [segs][code_width]  bit-reversed code | len << 24
    uint32_t *shdr;    // [segs][kHdrWords]
    uint32_t *shbits;  // [segs] header bits
    uint32_t *sbytes;  // [segs] segment bytes (header .. FF FF)
    uint32_t *scrc;    // [segs]
    uint64_t *soff;    // [segs] byte offset of the segment in its array's slot
};

// The workspace of a call on nc chunks and ns segments: its arrays carved from
// ws into w (ws == nullptr: none) and its size in bytes.
size_t ws_layout(void *ws, size_t nc, size_t ns, bool match, DWs *w) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void *p = ws ? static_cast<char *>(ws) + off : nullptr;
        off += align256(bytes);
        return p;
    };
    const size_t hw = size_t(hist_width(match)), cw = size_t(code_width(match));
    DWs d{};
    d.chist = static_cast<uint16_t *>(take(nc * 2 * hw));
    d.ccrc = static_cast<uint32_t *>(take(nc * 4));
    if (match) d.cxb = static_cast<uint32_t *>(take(nc * 4));
    d.cbit = static_cast<uint64_t *>(take(nc * 8));
    d.shist = static_cast<uint32_t *>(take(ns * 4 * hw));
    d.scode = static_cast<uint32_t *>(take(ns * 4 * cw));
    d.shdr = static_cast<uint32_t *>(take(ns * 4 * kHdrWords));
    d.shbits = static_cast<uint32_t *>(take(ns * 4));
    d.sbytes = static_cast<uint32_t *>(take(ns * 4));
    d.scrc = static_cast<uint32_t *>(take(ns * 4));
    // one more per-segment word, unused: ofd_deflate_workspace_bytes has always counted it, and callers hold that size
    if (!match) take(ns * 4);
    d.soff = static_cast<uint64_t *>(take(ns * 8));
    if (w) *w = d;
    return off;
}

size_t ws_bytes(int64_t count, int64_t each, bool match) {
    const int64_t cpa = (each + kChunk - 1) / kChunk, spa = (each + kSeg - 1) / kSeg;
    return ws_layout(nullptr, size_t(count * cpa), size_t(count * spa), match, nullptr);
}

__device__ __forceinline__ void make_crc_table(uint32_t *T) {
    for (int k = threadIdx.x; k < 256; k += kThr) {
        uint32_t c = uint32_t(k);
        for (int b = 0; b < 8; ++b) c = (c & 1) ? (c >> 1) ^ kPoly : c >> 1;
        T[k] = c;
    }
}

// A thread's n <= 64 bytes at src + t0 as 16 little-endian words (bytes past
// n read as 0): four 16-byte loads when aligned and whole, else byte loads.
__device__ __forceinline__ void load64(const uint8_t *__restrict__ src, int t0, int n, uint32_t wd[16]) {
    const uint8_t *p = src + t0;
    if (n == kPerThr && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
            wd[4 * q] = v.x;
            wd[4 * q + 1] = v.y;
            wd[4 * q + 2] = v.z;
            wd[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            uint32_t x = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * q + r < n) x |= uint32_t(p[4 * q + r]) << (8 * r);
            wd[q] = x;
        }
    }
}

// ---------------------------------------------------------------- tokens
// A thread turns its 64-byte span into tokens, in HIST and again in ENCODE (no
// token is ever stored).  Template parameter E is the mode.  E = 0, the literal
// mode: every byte is a literal.  E = 1, 2, 4, 8, the match mode at that
// element size: at byte p the thread takes the longest run b[p+i] == b[p+i-D]
// over the candidate distances D in {1, E, 2E} (the smaller D on ties) that
// stays inside the span, and codes it as a match when it is kMinMatch bytes or
// more, else b[p] as a literal.  A match may read the 2E <= 16 bytes before
// the span (they are input too), never bytes before its own array.  The parse
// is a pure function of the span and those 16 bytes.

// The 16 bytes before a span (zeros when there are none to read)
__device__ __forceinline__ void load_hist16(const uint8_t *p, bool have, uint32_t hs[4]) {
    hs[0] = hs[1] = hs[2] = hs[3] = 0u;
    if (!have) return;
    const uint8_t *h = p - 16;
    if ((reinterpret_cast<uintptr_t>(h) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(h);
        hs[0] = v.x, hs[1] = v.y, hs[2] = v.z, hs[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) hs[q] |= uint32_t(h[4 * q + r]) << (8 * r);
    }
}

// ext = 16 history bytes then the span's 64, as 20 little-endian words.
// Bit i of the result: span byte i equals the byte D before it.
template <int D, int q>
__device__ __forceinline__ uint64_t eq_nibble(const uint32_t ext[20]) {  // the mask's bits 4q .. 4q + 3
    uint32_t prev;
    if constexpr (D % 4 == 0)
        prev = ext[4 + q - D / 4];
    else
        prev = uint32_t(((uint64_t(ext[4 + q]) << 32) | ext[3 + q]) >> (8 * (4 - D)));
    const uint32_t x = ext[4 + q] ^ prev;
    uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 in every zero byte of x
    t >>= 7;
    return uint64_t((t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xFu) << (4 * q);
}

template <int D, int... Q>
__device__ __forceinline__ uint64_t eq_mask_seq(const uint32_t ext[20], std::integer_sequence<int, Q...>) {
    return (eq_nibble<D, Q>(ext) | ...);
}

template <int D>
__device__ __forceinline__ uint64_t eq_mask(const uint32_t ext[20]) {
    static_assert(D == 1 || D == 2 || D == 4 || D == 8 || D == 16, "distance");
    return eq_mask_seq<D>(ext, std::make_integer_sequence<int, 16>{});
}

// RFC 1951 3.2.5 for the distances in use (powers of two up to 16)
__device__ __forceinline__ constexpr int dist_sym(int D) { return D == 1 ? 0 : D == 2 ? 1 : D == 4 ? 3 : D == 8 ? 5 : 7; }
__device__ __forceinline__ constexpr int dist_xbits(int D) { return D == 8 ? 1 : D == 16 ? 2 : 0; }
__device__ __forceinline__ constexpr uint32_t dist_xval(int D) { return D == 8 ? 1u : D == 16 ? 3u : 0u; }

// length 3..257 -> symbol, extra bit count and value (258 is never emitted: a span has 64 bytes)
__device__ __forceinline__ void len_sym(int len, int &sym, int &xb, uint32_t &xv) {
    const int x = len - 3;
    if (x < 8) {
        sym = 257 + x, xb = 0, xv = 0u;
    } else {
        const int k = 29 - __clz(x);  // 8..15: 1 extra bit, 16..31: 2, 32..63: 3, ...
        sym = 257 + 4 * (k + 1) + ((x >> k) & 3), xb = k, xv = uint32_t(x) & ((1u << k) - 1u);
    }
}

template <int E>
struct SpanMasks {
    uint64_t m1, me, m2;  // distance 1 (E > 1 only), E, 2E; unused in the literal mode
};

// n = the span's bytes, first = the span starts its array (no history to match)
template <int E>
__device__ __forceinline__ SpanMasks<E> span_masks(const uint32_t ext[20], int n, bool first, int cand) {
    SpanMasks<E> m{0, 0, 0};
    if constexpr (E != 0) {
        const uint64_t live = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        if (E > 1 && (cand & 1)) m.m1 = eq_mask<1>(ext) & live & (first ? ~0ull << 1 : ~0ull);
        m.me = eq_mask<E>(ext) & live & (first ? ~0ull << E : ~0ull);
        if (cand & 2) m.m2 = eq_mask<2 * E>(ext) & live & (first ? ~0ull << (2 * E) : ~0ull);
    }
    return m;
}

template <int e, int E, class F>
__device__ __forceinline__ void parse_step(const SpanMasks<E> &m, int n, int &next, F &tok) {
    if constexpr (E == 0) {
        if (e < n) tok(std::integral_constant<int, e>{}, false, 0, 0);
    } else if (e == next && e < n) {
        auto run = [](uint64_t x) -> int {
            const uint64_t y = ~(x >> e);
            return y ? __builtin_ctzll(y) : 64;
        };
        int best = E > 1 ? run(m.m1) : 0, D = 1;
        const int re = run(m.me), r2 = run(m.m2);
        if (re > best) best = re, D = E;
        if (r2 > best) best = r2, D = 2 * E;
        const bool match = best >= kMinMatch;
        tok(std::integral_constant<int, e>{}, match, best, D);
        next = e + (match ? best : 1);
    }
}

template <int E, class F, int... I>
__device__ __forceinline__ void parse_steps(const SpanMasks<E> &m, int n, F &tok, std::integer_sequence<int, I...>) {
    int next = 0;
    (parse_step<I, E>(m, n, next, tok), ...);
}

// tok(e, is_match, length, D) for every token of the span, in order; e is the
// token's first byte as a std::integral_constant, so that every index into the
// span's registers is a constant.
template <int E, class F>
__device__ __forceinline__ void parse_span(const SpanMasks<E> &m, int n, F &&tok) {
    parse_steps<E>(m, n, tok, std::make_integer_sequence<int, kPerThr>{});
}

// byte e of the span in ext (e a constant)
template <int e>
__device__ __forceinline__ uint32_t span_byte(const uint32_t ext[20]) {
    return (ext[4 + (e >> 2)] >> (8 * (e & 3))) & 0xFFu;
}

// A thread's span of chunk bytes [t0, t0 + n) at src (chunk-relative; the chunk
// starts at byte beg of its array) with its history, as parse_span wants them
template <int E>
__device__ __forceinline__ void load_span(const uint8_t *__restrict__ src, int64_t beg, int t0, int n, uint32_t ext[20]) {
    if constexpr (E != 0) load_hist16(src + t0, n > 0 && beg + t0 > 0, ext);
    load64(src, t0, n, ext + 4);
}

// ---------------------------------------------------------------- HIST
// chunk c = (array a, chunk k of the array); thread t owns bytes [64 t, 64 t + 64)
template <int E>
__global__ __launch_bounds__(kThr) void dfl_hist_kernel(const uint8_t *__restrict__ in, Geo g, DWs w, int cand) {
    constexpr int kHist = hist_width(E != 0);
    __shared__ uint32_t T[256];
    __shared__ uint32_t H[kHist];
    __shared__ uint32_t C[kThr];
    __shared__ uint32_t X;
    const int c = blockIdx.x, a = c / g.cpa, k = c - a * g.cpa;
    const int64_t beg = int64_t(k) * kChunk, len = min(kChunk, g.each - beg);
    const uint8_t *src = in + int64_t(a) * g.each + beg;
    make_crc_table(T);
    for (int i = threadIdx.x; i < kHist; i += kThr) H[i] = 0u;
    if (threadIdx.x == 0) X = 0u;
    __syncthreads();
    const int t0 = threadIdx.x * kPerThr;
    const int n = int(min<int64_t>(kPerThr, max<int64_t>(len - t0, 0)));
    uint32_t ext[20];
    load_span<E>(src, beg, t0, n, ext);
    uint32_t crc = 0xFFFFFFFFu;
    auto crc_byte = [&](uint32_t b) { crc = T[(crc ^ b) & 0xFFu] ^ (crc >> 8); };
    // A match skips bytes, so the match mode's CRC takes a pass of its own; in
    // the literal mode every byte is a token and its CRC step rides along (a
    // second pass there costs 46 spilled SGPRs and a wave per SIMD).
    if constexpr (E != 0) {
#pragma unroll
        for (int e = 0; e < kPerThr; ++e)
            if (e < n) crc_byte(ext[4 + (e >> 2)] >> (8 * (e & 3)));
    }
    uint32_t zeros = 0, xbits = 0;
    const SpanMasks<E> sm = span_masks<E>(ext, n, beg + t0 == 0, cand);
    parse_span<E>(sm, n, [&](auto e, bool match, int mlen, int D) {
        if (!match) {
            const uint32_t b = span_byte<decltype(e)::value>(ext);
            if constexpr (E == 0) crc_byte(b);
            if (b == 0u)
                ++zeros;
            else
                atomicAdd(&H[b], 1u);
        } else {
            int sym, xb;
            uint32_t xv;
            len_sym(mlen, sym, xb, xv);
            atomicAdd(&H[sym], 1u);
            atomicAdd(&H[kDOff + dist_sym(D)], 1u);
            xbits += uint32_t(xb + dist_xbits(D));
        }
    });
    // zero literals dominate: one wave sum instead of 64 colliding LDS atomics per lane-step
    for (int d = 32; d > 0; d >>= 1) {
        zeros += __shfl_xor(zeros, d);
        if constexpr (E != 0) xbits += __shfl_xor(xbits, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (zeros) atomicAdd(&H[0], zeros);
        if (xbits) atomicAdd(&X, xbits);
    }
    C[threadIdx.x] = ~crc;
    __syncthreads();
    // fold the per-thread CRCs (thread t covers n_t bytes, all 64 but a ragged tail)
    for (int s = 1; s < kThr; s <<= 1) {
        if ((threadIdx.x & (2 * s - 1)) == 0 && threadIdx.x + s < kThr) {
            const int64_t lb = min<int64_t>(int64_t(s) * kPerThr, max<int64_t>(len - int64_t(threadIdx.x + s) * kPerThr, 0));
            if (lb > 0) C[threadIdx.x] = crc_combine(C[threadIdx.x], C[threadIdx.x + s], uint64_t(lb));
        }
        __syncthreads();
    }
    const int seg = a * g.spa + int(beg / kSeg);
    for (int i = threadIdx.x; i < kHist; i += kThr) {
        const uint32_t h = H[i];
        w.chist[int64_t(c) * kHist + i] = uint16_t(h);
        if (h) atomicAdd(&w.shist[int64_t(seg) * kHist + i], h);
    }
    if (threadIdx.x == 0) {
        w.ccrc[c] = len > 0 ? C[0] : 0u;
        if constexpr (E != 0) w.cxb[c] = X;
    }
}

// ---------------------------------------------------------------- CODE
// Huffman code lengths (<= maxlen) of n <= 512 symbols with frequencies f[]
// (0 = absent), by thread 0 after a block-wide sort; the frequencies are
// flattened and the tree rebuilt until the deepest leaf fits.
struct HuffLds {
    uint64_t key[512];    // sorted (freq << 16 | symbol)
    uint32_t node[1024];  // internal node frequencies / parents
    uint32_t par[1024];
    uint8_t len[512];
};

__device__ void sort_keys(uint64_t *key) {  // 512 keys ascending, 256 threads
    for (int k = 2; k <= 512; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < 512; i += kThr) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const uint64_t x = key[i], y = key[l];
                    if ((x > y) == up) {
                        key[i] = y;
                        key[l] = x;
                    }
                }
            }
            __syncthreads();
        }
}

// lengths for symbols 0..n-1 into L.len; f[] in LDS, may be modified (flattening)
__device__ void huff_lengths(uint32_t *f, int n, int maxlen, HuffLds &L) {
    __shared__ int s_ok;
    for (;;) {
        for (int i = threadIdx.x; i < 512; i += kThr) {
            L.key[i] = (i < n && f[i]) ? (uint64_t(f[i]) << 16) | uint64_t(i) : ~0ull;
            if (i < n) L.len[i] = 0;
        }
        __syncthreads();
        sort_keys(L.key);
        if (threadIdx.x == 0) {
            int m = 0;
            while (m < 512 && L.key[m] != ~0ull) ++m;  // leaves, ascending
            // two-queue Huffman: leaves 0..m-1, internal nodes m..2m-2
            int i = 0, j = 0;
            for (int k = 0; k < m - 1; ++k) {
                uint32_t fx[2];
                int id[2];
                for (int r = 0; r < 2; ++r) {
                    const bool leaf = i < m && (j >= k || uint32_t(L.key[i] >> 16) <= L.node[j]);
                    if (leaf) {
                        fx[r] = uint32_t(L.key[i] >> 16);
                        id[r] = i++;
                    } else {
                        fx[r] = L.node[j];
                        id[r] = m + j++;
                    }
                }
                L.node[k] = fx[0] + fx[1];
                L.par[id[0]] = uint32_t(m + k);
                L.par[id[1]] = uint32_t(m + k);
            }
            // depths: root = node m + m - 2 at depth 0 (a lone leaf gets length 1)
            int deepest = 0;
            if (m == 1) {
                L.len[uint32_t(L.key[0]) & 0xFFFFu] = 1;
                deepest = 1;
            } else {
                L.node[m - 2] = 0;  // reuse: depth of internal node k
                for (int k = m - 3; k >= 0; --k) L.node[k] = L.node[L.par[m + k] - m] + 1;
                for (int q = 0; q < m; ++q) {
                    const int d = int(L.node[L.par[q] - m]) + 1;
                    L.len[uint32_t(L.key[q]) & 0xFFFFu] = uint8_t(d);
                    deepest = d > deepest ? d : deepest;
                }
            }
            s_ok = deepest <= maxlen;
        }
        __syncthreads();
        if (s_ok) return;
        for (int i = threadIdx.x; i < n; i += kThr)
            if (f[i]) f[i] = (f[i] + 1u) >> 1;  // flatten (stays >= 1) and rebuild
        __syncthreads();
    }
}

// canonical code of every symbol (RFC 1951 3.2.2), bit-reversed for LSB-first
// emission, as code | len << 24; by thread 0
__device__ void canonical(const uint8_t *len, int n, uint32_t *out) {
    uint32_t count[16] = {}, next[16];
    for (int s = 0; s < n; ++s) ++count[len[s]];
    count[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b < 16; ++b) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        uint32_t c = 0;
        if (l) {
            const uint32_t v = next[l]++;
            for (int b = 0; b < l; ++b) c |= ((v >> b) & 1u) << (l - 1 - b);
        }
        out[s] = c | (uint32_t(l) << 24);
    }
}

__device__ __forceinline__ void put_bits(uint32_t *buf, uint32_t &pos, uint32_t v, int n) {  // LSB first, n <= 16
    for (int b = 0; b < n; ++b, ++pos)
        if ((v >> b) & 1u) buf[pos >> 5] |= 1u << (pos & 31);
}

// Two trees per segment: literal / length (<= 286 symbols) and distance (<= 30).
// zlib's inflater accepts exactly these distance codes: no match in the
// segment (always so in the literal mode) -> one distance length 0; one
// distance symbol -> that symbol with length 1 (incomplete, allowed); two or
// more -> a complete (Huffman) code.
template <bool kMatch>
__global__ __launch_bounds__(kThr) void dfl_code_kernel(Geo g, DWs w) {
    constexpr int kHist = hist_width(kMatch), kCode = code_width(kMatch);
    __shared__ HuffLds L;
    __shared__ uint32_t f[512];
    __shared__ uint32_t code[kAll];  // [0, 286) literal / length, [286, 316) distance
    __shared__ uint32_t hdr[kHdrWords];
    __shared__ uint32_t clf[19];
    __shared__ uint32_t clcode[19];
    __shared__ uint64_t cb[kChunksPerSeg];
    __shared__ int s_hlit, s_hdist, s_nd;
    const int s = blockIdx.x, a = s / g.spa, k = s - a * g.spa;
    const int64_t sbeg = int64_t(k) * kSeg, slen = min(kSeg, g.each - sbeg);
    const int c0 = a * g.cpa + int(sbeg / kChunk), nch = int((slen + kChunk - 1) / kChunk);
    const uint32_t *sh = w.shist + int64_t(s) * kHist;
    // the end of block occurs once; symbols past the mode's counts never
    for (int i = threadIdx.x; i < 512; i += kThr) f[i] = i == 256 ? 1u : (i < kLSym && i < kHist ? sh[i] : 0u);
    for (int i = threadIdx.x; i < kHdrWords; i += kThr) hdr[i] = 0u;
    for (int i = threadIdx.x; i < kAll; i += kThr) code[i] = 0u;
    if (threadIdx.x == 0) {
        int hlit = 257, hdist = 1, nd = 0;
        if constexpr (kMatch) {
            for (int i = 257; i < kLSym; ++i)
                if (sh[i]) hlit = i + 1;
            for (int i = 0; i < kDSym; ++i)
                if (sh[kDOff + i]) hdist = i + 1, ++nd;
        }
        s_hlit = hlit, s_hdist = hdist, s_nd = nd;
    }
    __syncthreads();
    huff_lengths(f, kLSym, kMaxLen, L);
    if (threadIdx.x == 0) canonical(L.len, kLSym, code);
    __syncthreads();
    if (kMatch && s_nd > 0) {  // the same in every thread
        for (int i = threadIdx.x; i < 512; i += kThr) f[i] = i < kDSym ? sh[kDOff + i] : 0u;
        __syncthreads();
        huff_lengths(f, kDSym, kMaxLen, L);
        if (threadIdx.x == 0) canonical(L.len, kDSym, code + kDOff);
        __syncthreads();
    }
    const int hlit = s_hlit, hdist = s_hdist;
    // code-length code over the hlit + hdist lengths sent
    if (threadIdx.x < 19) clf[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < hlit; i += kThr) atomicAdd(&clf[code[i] >> 24], 1u);
    for (int i = threadIdx.x; i < hdist; i += kThr) atomicAdd(&clf[code[kDOff + i] >> 24], 1u);
    __syncthreads();
    huff_lengths(clf, 19, 7, L);
    if (threadIdx.x == 0) {
        canonical(L.len, 19, clcode);
        static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && L.len[order[hclen - 1]] == 0) --hclen;
        uint32_t pos = 0;
        put_bits(hdr, pos, 0u, 1);  // BFINAL 0
        put_bits(hdr, pos, 2u, 2);  // BTYPE 2 (dynamic)
        put_bits(hdr, pos, uint32_t(hlit - 257), 5);
        put_bits(hdr, pos, uint32_t(hdist - 1), 5);
        put_bits(hdr, pos, uint32_t(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) put_bits(hdr, pos, L.len[order[i]], 3);
        for (int i = 0; i < hlit + hdist; ++i) {
            const uint32_t l = code[i < hlit ? i : kDOff + i - hlit] >> 24;
            put_bits(hdr, pos, clcode[l] & 0xFFFFFFu, int(clcode[l] >> 24));
        }
        w.shbits[s] = pos;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHdrWords; i += kThr) w.shdr[int64_t(s) * kHdrWords + i] = hdr[i];
    for (int i = threadIdx.x; i < kCode; i += kThr) w.scode[int64_t(s) * kCode + i] = code[i];
    // chunk bit counts: its symbols' code lengths plus its matches' extra bits; one wave per chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < nch; q += kThr / 64) {
        uint32_t bits = 0;
        for (int i = lane; i < kHist; i += 64) bits += uint32_t(w.chist[int64_t(c0 + q) * kHist + i]) * (code[i] >> 24);
        for (int d = 32; d > 0; d >>= 1) bits += __shfl_xor(bits, d);
        if (lane == 0) cb[q] = uint64_t(bits) + (kMatch ? w.cxb[c0 + q] : 0u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // in order: each chunk's first code sits after the header and the chunks before it
        uint64_t acc = w.shbits[s];
        for (int q = 0; q < nch; ++q) {
            w.cbit[c0 + q] = acc;
            acc += cb[q];
        }
        acc += code[256] >> 24;                    // end of block
        acc += 3;                                  // sync flush: an empty stored block's header ...
        const uint64_t bytes = (acc + 7) / 8 + 4;  // ... padded to a byte, LEN 0000, NLEN FFFF
        w.sbytes[s] = uint32_t(bytes);
        // segment CRC from its chunks' CRCs
        uint32_t crc = w.ccrc[c0];
        for (int q = 1; q < nch; ++q) {
            const int64_t lq = min(kChunk, slen - int64_t(q) * kChunk);
            crc = crc_combine(crc, w.ccrc[c0 + q], uint64_t(lq));
        }
        w.scrc[s] = crc;
    }
}

// ---------------------------------------------------------------- SCAN
__global__ void dfl_scan_kernel(Geo g, DWs w, uint8_t *__restrict__ out, uint64_t *__restrict__ sizes,
                                uint32_t *__restrict__ crcs, int64_t count) {
    const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= count) return;
    uint64_t off = 0;
    uint32_t crc = 0;
    for (int k = 0; k < g.spa; ++k) {
        const int64_t s = a * g.spa + k;
        w.soff[s] = off;
        off += w.sbytes[s];
        const int64_t lk = min(kSeg, g.each - int64_t(k) * kSeg);
        crc = k == 0 ? w.scrc[s] : crc_combine(crc, w.scrc[s], uint64_t(lk));
    }
    uint8_t *o = out + a * g.bound;
    o[off] = 0x03;  // final empty fixed block: BFINAL 1, BTYPE 1, end of block
    o[off + 1] = 0x00;
    sizes[a] = off + 2;
    crcs[a] = g.spa ? crc : 0u;
}

// ---------------------------------------------------------------- ENCODE
__device__ __forceinline__ void or_bits(uint32_t *o, uint64_t pos, uint64_t v, int n) {  // n <= 32, into zeroed memory
    const uint64_t wd = pos >> 5;
    const int sh = int(pos & 31);
    const uint64_t x = (v & ((n == 32) ? 0xFFFFFFFFull : ((1ull << n) - 1))) << sh;
    if (uint32_t(x)) atomicOr(o + wd, uint32_t(x));
    if (uint32_t(x >> 32)) atomicOr(o + wd + 1, uint32_t(x >> 32));
}

template <int E>
__global__ __launch_bounds__(kThr) void dfl_encode_kernel(const uint8_t *__restrict__ in, Geo g, DWs w,
                                                          uint8_t *__restrict__ out, int cand) {
    constexpr int kCode = code_width(E != 0);
    __shared__ uint32_t code[kCode];
    __shared__ uint32_t wsum[kThr / 64];
    const int c = blockIdx.x, a = c / g.cpa, k = c - a * g.cpa;
    const int64_t beg = int64_t(k) * kChunk, len = min(kChunk, g.each - beg);
    const int s = a * g.spa + int(beg / kSeg);
    for (int i = threadIdx.x; i < kCode; i += kThr) code[i] = w.scode[int64_t(s) * kCode + i];
    __syncthreads();
    const uint8_t *src = in + int64_t(a) * g.each + beg;
    const int t0 = threadIdx.x * kPerThr;
    const int n = int(min<int64_t>(kPerThr, max<int64_t>(len - t0, 0)));
    uint32_t ext[20];
    load_span<E>(src, beg, t0, n, ext);
    const SpanMasks<E> sm = span_masks<E>(ext, n, beg + t0 == 0, cand);
    // A token's code pieces, in stream order, each <= 20 bits LSB first, to
    // put(value, bit count): a literal's code; a match's length code with its
    // extra bits, then its distance code with its extra bits.
    auto pieces = [&](auto e, bool match, int mlen, int D, auto &put) {
        if (!match) {
            const uint32_t ce = code[span_byte<decltype(e)::value>(ext)];
            put(ce & 0xFFFFFFu, int(ce >> 24));
        } else {
            int sym, xb;
            uint32_t xv;
            len_sym(mlen, sym, xb, xv);
            const uint32_t cl = code[sym], cd = code[kDOff + dist_sym(D)];
            put((cl & 0xFFFFFFu) | (xv << (cl >> 24)), int(cl >> 24) + xb);
            put((cd & 0xFFFFFFu) | (dist_xval(D) << (cd >> 24)), int(cd >> 24) + dist_xbits(D));
        }
    };
    uint32_t bits = 0;
    auto count = [&](uint32_t, int nb) { bits += uint32_t(nb); };
    parse_span<E>(sm, n, [&](auto e, bool match, int mlen, int D) { pieces(e, match, mlen, D, count); });
    // exclusive scan of the bit counts over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = bits;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int q = 0; q < wave; ++q) before += wsum[q];
    const uint64_t seg_bit0 = w.soff[s] * 8;
    const uint64_t pos = seg_bit0 + w.cbit[c] + before + incl - bits;
    uint32_t *o = reinterpret_cast<uint32_t *>(out + a * g.bound);  // slots are 256-byte aligned
    // The thread's codes, packed into 32-bit words: its first and last words
    // may hold its neighbours' bits too (atomic OR into the zeroed slot), the
    // words in between are its own (plain stores).
    if (bits) {
        const uint64_t w0 = pos >> 5, wl = (pos + bits - 1) >> 5;
        uint64_t acc = 0;
        int nacc = int(pos & 31);  // the first word's bits below the thread's start stay 0
        uint64_t wi = w0;
        auto emit = [&](uint32_t v) {
            if (wi == w0 || wi == wl)
                atomicOr(o + wi, v);
            else
                o[wi] = v;
            ++wi;
        };
        auto add = [&](uint32_t v, int nb) {
            acc |= uint64_t(v) << nacc;
            nacc += nb;
            if (nacc >= 32) {
                emit(uint32_t(acc));
                acc >>= 32;
                nacc -= 32;
            }
        };
        parse_span<E>(sm, n, [&](auto e, bool match, int mlen, int D) { pieces(e, match, mlen, D, add); });
        if (nacc > 0) emit(uint32_t(acc));
    }
    const int64_t sbeg = int64_t(beg / kSeg) * kSeg;
    if (threadIdx.x == 0 && beg == sbeg) {
        // the segment's first chunk: its block header
        const uint32_t hb = w.shbits[s];
        const uint32_t *h = w.shdr + int64_t(s) * kHdrWords;
        for (uint32_t q = 0; q * 32 < hb; ++q) {
            const int nb = int(min(32u, hb - q * 32));
            or_bits(o, seg_bit0 + uint64_t(q) * 32, h[q], nb);
        }
    }
    const int64_t slen = min(kSeg, g.each - sbeg);
    if (threadIdx.x == kThr - 1 && beg + len == sbeg + slen) {
        // the segment's last chunk: end of block, then the sync marker's FF FF
        const uint32_t ce = code[256];
        const uint64_t epos = seg_bit0 + w.cbit[c] + before + incl;
        or_bits(o, epos, ce & 0xFFFFFFu, int(ce >> 24));
        const uint64_t end = w.soff[s] + w.sbytes[s];  // byte after FF FF
        or_bits(o, (end - 2) * 8, 0xFFFFu, 16);
    }
}

// ---------------------------------------------------------------- host
// The kernels of one call in mode E (0: literal); an empty array is its final block alone
using Launch = void (*)(const uint8_t *, uint8_t *, const Geo &, const DWs &, int64_t, uint64_t *, uint32_t *, int,
                        hipStream_t);

template <int E>
void launch(const uint8_t *src, uint8_t *dst, const Geo &g, const DWs &w, int64_t count, uint64_t *sizes, uint32_t *crcs,
            int cand, hipStream_t st) {
    const unsigned nc = unsigned(count * g.cpa), ns = unsigned(count * g.spa);
    if (nc) {
        hipLaunchKernelGGL(dfl_hist_kernel<E>, dim3(nc), dim3(kThr), 0, st, src, g, w, cand);
        hipLaunchKernelGGL(dfl_code_kernel<E != 0>, dim3(ns), dim3(kThr), 0, st, g, w);
    }
    hipLaunchKernelGGL(dfl_scan_kernel, dim3(unsigned((count + 255) / 256)), dim3(256), 0, st, g, w, dst, sizes, crcs,
                       count);
    if (nc) hipLaunchKernelGGL(dfl_encode_kernel<E>, dim3(nc), dim3(kThr), 0, st, src, g, w, dst, cand);
}

// Both entry points.  They report a bad workspace at different places: the
// match mode before anything is enqueued, the literal mode after the slots'
// memset (and so after that memset's own error).
int deflate_batch(Launch launch, bool match, const void *in, int64_t count, int64_t bytes_each, void *out,
                  uint64_t *sizes, uint32_t *crcs, void *workspace, size_t workspace_bytes, void *stream) {
    if (count < 0 || bytes_each < 0) return OFD_FW_EINVAL;
    if (count == 0) return OFD_FW_OK;
    if (!out || !sizes || !crcs || (bytes_each > 0 && !in)) return OFD_FW_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 255u) return OFD_FW_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Geo g;
    g.each = bytes_each;
    g.cpa = int((bytes_each + kChunk - 1) / kChunk);
    g.spa = int((bytes_each + kSeg - 1) / kSeg);
    g.bound = int64_t(ofd_deflate_bound(bytes_each));
    if (int64_t(count) * g.cpa >= (int64_t(1) << 31)) return OFD_FW_ETOOBIG;
    const bool ws_bad = bytes_each > 0 && (!workspace || workspace_bytes < ws_bytes(count, bytes_each, match) ||
                                           (reinterpret_cast<uintptr_t>(workspace) & 255u));
    if (match && ws_bad) return OFD_FW_EWORKSPACE;
    hipError_t e = hipMemsetAsync(out, 0, size_t(count) * size_t(g.bound), st);
    if (e != hipSuccess) return int(e);
    if (ws_bad) return OFD_FW_EWORKSPACE;
    DWs w{};
    if (bytes_each > 0) {
        const size_t ns = size_t(count) * g.spa;
        ws_layout(workspace, size_t(count) * g.cpa, ns, match, &w);
        e = hipMemsetAsync(w.shist, 0, ns * 4 * hist_width(match), st);
        if (e != hipSuccess) return int(e);
    }
    launch(static_cast<const uint8_t *>(in), static_cast<uint8_t *>(out), g, w, count, sizes, crcs, g_lz_cand, st);
    e = hipGetLastError();
    return e == hipSuccess ? OFD_FW_OK : int(e);
}

}  // namespace

extern "C" {

size_t ofd_deflate_bound(int64_t bytes_each) {
    if (bytes_each < 0) return 0;
    const int64_t spa = (bytes_each + kSeg - 1) / kSeg;
    // <= 15 bits per byte, a header and the sync marker per segment, the final block
    return align256(size_t(bytes_each) * 2 + size_t(spa) * (kHdrWords * 4 + 16) + 64);
}

size_t ofd_deflate_workspace_bytes(int64_t count, int64_t bytes_each) {
    if (count <= 0 || bytes_each <= 0) return 0;
    return ws_bytes(count, bytes_each, false);
}

int ofd_deflate_batch(const void *in, int64_t count, int64_t bytes_each, void *out, uint64_t *sizes, uint32_t *crcs,
                      void *workspace, size_t workspace_bytes, void *stream) {
    return deflate_batch(launch<0>, false, in, count, bytes_each, out, sizes, crcs, workspace, workspace_bytes, stream);
}

size_t ofd_deflate_lz_bound(int64_t bytes_each) {
    // The worst token decides.  A literal costs <= 15 bits for 1 byte.  A match
    // costs <= 15 (length code) + 5 (length extra bits) + 15 (distance code) +
    // 2 (extra bits of distance 16, the largest candidate) = 37 bits for
    // >= kMinMatch = 3 bytes, i.e. <= 12.4 bits per byte.  So 15 bits per byte
    // bounds the codes as in the literal mode, the header (<= 2283 bits) fits
    // the same kHdrWords, and the slot is the literal mode's.
    return ofd_deflate_bound(bytes_each);
}

size_t ofd_deflate_lz_workspace_bytes(int64_t count, int64_t bytes_each) {
    if (count <= 0 || bytes_each <= 0) return 0;
    return ws_bytes(count, bytes_each, true);
}

int ofd_deflate_lz_set_candidates(int mask) {
    if (mask < 0 || mask > 3) return OFD_FW_EINVAL;
    g_lz_cand = mask;
    return OFD_FW_OK;
}

int ofd_deflate_lz_batch(const void *in, int64_t count, int64_t bytes_each, int elem_bytes, void *out, uint64_t *sizes,
                         uint32_t *crcs, void *workspace, size_t workspace_bytes, void *stream) {
    Launch l;
    switch (elem_bytes) {
        case 1: l = launch<1>; break;
        case 2: l = launch<2>; break;
        case 4: l = launch<4>; break;
        case 8: l = launch<8>; break;
        default: return OFD_FW_EINVAL;
    }
    return deflate_batch(l, true, in, count, bytes_each, out, sizes, crcs, workspace, workspace_bytes, stream);
}

}  // extern "C"
