// PNG encoder on the device: uint8 [n, h, w, c] images (c = 1 grey, c = 3 RGB) -> one complete PNG file per
// image in device memory.  The host computes sizes and launches; every byte of the files is produced by the kernels below.
//
// File layout:  signature | IHDR | one IDAT per row | one closing IDAT | IEND.  The IDAT payloads form one zlib stream:
//   78 01 | per row: [fixed-Huffman block (BFINAL 0), empty stored block (pads to a byte: .. 00 00 FF FF)] | 03 00 (final
//   empty fixed block) | Adler-32.
// At level 2 a row's block is the smallest of three codings of the same tokens: fixed Huffman, dynamic Huffman (a code built
// from the row's own histogram, png_huffman.h) or stored.
// Every row therefore encodes independently of every other one and ends on a byte boundary (the way pigz joins the output of
// its threads), and every row's chunk carries its own CRC-32.
//
//   png_rows_kernel    one workgroup per (row, image): filter choice, deflate, CRC, the row's Adler-32 part -> staging slot
//   png_finish_kernel  one workgroup per image: signature, IHDR, row offsets (exclusive scan of the chunk sizes), the
//                      combined Adler-32, closing IDAT, IEND, the file's length
//   png_gather_kernel  one workgroup per (row, image): the row's chunk from its staging slot to its place in the file
// The assembly of a file from its rows (workgroup scan, row offsets, row copy, workspace tables) is row_files.h, shared with
// jpeg.hip.
//
// No atomics on global memory and fixed-order reductions: the bytes of an image do not depend on the batch it is in or on
// the run.
#include "cgan_common.h"
#include "png_huffman.h"
#include "row_files.h"

#include <vector>

namespace {

using row_files::T;                         // threads per workgroup, all three kernels
constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t PNG_FIXED_BYTES = 8 + 25 + 2 + 18 + 12;   // signature, IHDR, zlib header, closing IDAT, IEND

__host__ __device__ inline uint32_t png_round_up(uint32_t v, uint32_t a) { return (v + a - 1u) / a * a; }

// bytes of one row's deflate data, m = 1 + w * c filtered bytes: 3 header bits, at most 9 bits per byte, the 7-bit end of
// block, the 3-bit stored-block header, padding, then LEN / NLEN
__host__ __device__ inline uint32_t png_row_data_max(uint32_t m) { return (9u * m + 13u + 7u) / 8u + 4u; }

// a row's staging slot: [0, 16) the chunk header (length, "IDAT", the zlib header in row 0) right-aligned, so that the
// deflate data starts 16-byte aligned at 16; then the data and the chunk's CRC
__host__ __device__ inline uint32_t png_slot_bytes(uint32_t m) { return 16u + png_round_up(png_row_data_max(m) + 8u, 16u); }

// LDS of png_rows_kernel (byte offsets).  r0 holds the row and the row above it while the filter is chosen, then one of the
// two pointer-jumping buffers, then the bit buffer.
struct PngLds {
  uint32_t prev, j1, d, len, flags, scratch, total;
};
// What level 2 adds behind that (byte offsets from PngLds::total, 3488 bytes).  The sorted counts are dead once the lengths
// exist and give their place to the header tokens; the sort's symbol order gives its place to the codes.
constexpr uint32_t PNG_SYMS = 288;          // 286 literal / length symbols, padded
constexpr uint32_t PNG_H_HIST = 0;                              // uint32 [288]  token counts per symbol
constexpr uint32_t PNG_H_SORTED = PNG_H_HIST + 4u * PNG_SYMS;   // uint32 [288]  sorted counts; then uint16 header tokens
constexpr uint32_t PNG_H_CODES = PNG_H_SORTED + 4u * PNG_SYMS;  // uint16 [288]  symbols in sorted order; then the codes
constexpr uint32_t PNG_H_LENS = PNG_H_CODES + 2u * PNG_SYMS;    // uint8 [320]   code lengths, the distance code's behind
constexpr uint32_t PNG_H_CL = PNG_H_LENS + 320u;                // the code-length code: PngClCode
constexpr uint32_t PNG_H_BYTES = PNG_H_CL + 288u;
struct PngClCode {
  uint32_t counts[png_huff::NUM_CL], sorted[png_huff::NUM_CL];
  uint16_t order[png_huff::NUM_CL], codes[png_huff::NUM_CL];
  uint8_t lens[png_huff::NUM_CL + 1];
  uint32_t nlit, ndist, ntok, hclen, header_bits;   // of the dynamic block's header, 3-bit block header not counted
};
static_assert(sizeof(PngClCode) <= PNG_H_BYTES - PNG_H_CL, "PngClCode outgrew its place");
// the level-2 arrays by name, declared only inside the level-2 branches: level 1 has none of them
#define PNG_HUFFMAN_LDS(base)                                                                      \
  [[maybe_unused]] unsigned char* const hs = (base);                                                \
  [[maybe_unused]] uint32_t* const hist = reinterpret_cast<uint32_t*>(hs + PNG_H_HIST);             \
  [[maybe_unused]] uint16_t* const codes = reinterpret_cast<uint16_t*>(hs + PNG_H_CODES);           \
  [[maybe_unused]] uint16_t* const hdr_tokens = reinterpret_cast<uint16_t*>(hs + PNG_H_SORTED);     \
  [[maybe_unused]] uint8_t* const lens = hs + PNG_H_LENS;                                           \
  [[maybe_unused]] PngClCode* const cl = reinterpret_cast<PngClCode*>(hs + PNG_H_CL)
__host__ __device__ inline PngLds png_lds(uint32_t m) {
  PngLds o;
  const uint32_t rowb = png_round_up(m - 1u, 16u);
  const uint32_t jb = png_round_up(2u * (m + 1u), 16u);
  const uint32_t bb = png_round_up(png_row_data_max(m) + 8u, 16u);
  uint32_t r0 = 2u * rowb;
  r0 = r0 > jb ? r0 : jb;
  r0 = r0 > bb ? r0 : bb;
  const uint32_t mb = png_round_up(m + 1u, 16u);
  o.prev = rowb;
  o.j1 = r0;
  o.d = o.j1 + jb;
  o.len = o.d + mb;
  o.flags = o.len + mb;
  o.scratch = o.flags + mb;
  o.total = o.scratch + 5u * T * 4u;
  return o;
}

// ---- CRC-32 (reflected, bit 31 of a polynomial word = x^0) -------------------------------------------------------------
__device__ inline uint32_t crc_byte(uint32_t crc, uint32_t b) {
  crc ^= b;
#pragma unroll
  for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (CRC_POLY & (0u - (crc & 1u)));
  return crc;
}
// a * b mod P
__device__ inline uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 n) mod P: what n zero bytes do to a CRC register
__device__ inline uint32_t gf_pow_x8(uint32_t n) {
  uint32_t r = 0x80000000u, base = 0x00800000u;
  while (n) {
    if (n & 1u) r = gf_mul(r, base);
    base = gf_mul(base, base);
    n >>= 1;
  }
  return r;
}
__device__ inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// ---- fixed-Huffman codes ---------------------------------------------------------------------------------------------
// Huffman codes enter the stream most-significant bit first, everything else least-significant bit first: a token is
// returned as the value whose bit 0 is the first bit of the stream, and its bit count.
__device__ inline uint32_t bit_rev(uint32_t v, uint32_t n) { return __brev(v) >> (32u - n); }

__device__ inline uint32_t literal_token(uint32_t b, uint32_t& nbits) {
  if (b < 144u) {
    nbits = 8;
    return bit_rev(0x30u + b, 8);
  }
  nbits = 9;
  return bit_rev(0x190u + (b - 144u), 9);
}
// length symbol 257..285 of l = length - 3, its extra bits and their value
__device__ inline uint32_t length_symbol(uint32_t l, uint32_t& eb, uint32_t& ev) {
  eb = 0, ev = 0;
  if (l < 8u) return 257u + l;
  if (l == 255u) return 285u;
  eb = (31u - (uint32_t)__clz(l)) - 2u;
  ev = l & ((1u << eb) - 1u);
  return 261u + 4u * eb + ((l >> eb) & 3u);
}
// l = length - 3 (0..255), dist_c: distance 3 instead of 1
__device__ inline uint32_t match_token(uint32_t l, bool dist3, uint32_t& nbits) {
  uint32_t eb, ev;
  const uint32_t code = length_symbol(l, eb, ev);
  const uint32_t hb = code < 280u ? 7u : 8u;
  const uint32_t huff = code < 280u ? code - 256u : 0xC0u + (code - 280u);
  // distance codes 0 (distance 1) and 2 (distance 3): 5 bits, no extra bits; 00010 reversed = 01000
  const uint32_t dist = dist3 ? 8u : 0u;
  nbits = hb + eb + 5u;
  return bit_rev(huff, hb) | (ev << hb) | (dist << (hb + eb));
}
// ---- level 2: the same tokens under another code ------------------------------------------------------------------------
__device__ inline uint32_t symbol_extra_bits(uint32_t s) { return (s < 265u || s == 285u) ? 0u : (s - 261u) >> 2; }
__device__ inline uint32_t fixed_code_bits(uint32_t s) { return s < 144u ? 8u : (s < 256u ? 9u : (s < 280u ? 7u : 8u)); }
// The distance code is declared complete and never built: lengths {1, 1} (c = 1) or {1, 0, 1} (c = 3), so distance 1 (code
// 0) is the bit 0 and distance 3 (code 2) the bit 1.
__device__ inline uint32_t dynamic_match_token(uint32_t l, bool dist3, const uint16_t* codes, const uint8_t* lens,
                                               uint32_t& nbits) {
  uint32_t eb, ev;
  const uint32_t s = length_symbol(l, eb, ev);
  const uint32_t hb = lens[s];
  nbits = hb + eb + 1u;
  return codes[s] | (ev << hb) | ((dist3 ? 1u : 0u) << (hb + eb));
}

__device__ inline void emit_bits(uint32_t* bb, uint32_t pos, uint32_t v, uint32_t nbits) {
  const uint32_t wi = pos >> 5, sh = pos & 31u;
  atomicOr(&bb[wi], v << sh);
  if (sh + nbits > 32u) atomicOr(&bb[wi + 1u], v >> (32u - sh));
}

// sum over the workgroup, returned to every thread; s: T words of LDS
__device__ inline uint32_t block_sum(uint32_t* s, uint32_t v) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int k = T / 2; k > 0; k >>= 1) {
    if (t < k) s[t] += s[t + k];
    __syncthreads();
  }
  const uint32_t r = s[0];
  __syncthreads();
  return r;
}

__device__ inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ inline uint32_t png_filter(int f, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  switch (f) {
    case 0: return x;
    case 1: return (x - a) & 255u;
    case 2: return (x - b) & 255u;
    case 3: return (x - ((a + b) >> 1)) & 255u;
    default: return (x - paeth(a, b, c)) & 255u;
  }
}

// one workgroup per (row, image).  row_len = w * c bytes.  LEVEL 1: fixed-Huffman blocks; LEVEL 2: per row the smallest of
// the fixed, dynamic and stored coding (first on ties), PNG_H_BYTES more LDS behind PngLds::total.
enum : uint32_t { PNG_FIXED = 1, PNG_DYNAMIC = 2, PNG_STORED = 0 };         // = BTYPE
template <int LEVEL>
__global__ __launch_bounds__(T) void png_rows_kernel(const uint8_t* __restrict__ in, int h, int row_len, int c,
                                                         uint32_t* __restrict__ row_size, uint32_t* __restrict__ row_s1,
                                                         uint32_t* __restrict__ row_s2, uint8_t* __restrict__ staging,
                                                         uint32_t slot_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int r = blockIdx.x;
  const size_t idx = (size_t)blockIdx.y * h + r;
  const uint32_t L = (uint32_t)row_len, m = L + 1u;
  const PngLds o = png_lds(m);
  uint8_t* cur = smem;
  uint8_t* prev = smem + o.prev;
  uint16_t* j0 = reinterpret_cast<uint16_t*>(smem);
  uint16_t* j1 = reinterpret_cast<uint16_t*>(smem + o.j1);
  uint32_t* bb = reinterpret_cast<uint32_t*>(smem);
  uint8_t* d = smem + o.d;
  uint8_t* lenm3 = smem + o.len;
  uint8_t* flags = smem + o.flags;          // bit 0: a token starts here; bit 1: it is a match; bit 2: at distance c
  uint32_t* scratch = reinterpret_cast<uint32_t*>(smem + o.scratch);

  // ---- the row and the row above it (zeros above the first row) -------------------------------------------------------
  const uint8_t* src = in + idx * L;
  if ((L & 15u) == 0 && (reinterpret_cast<uintptr_t>(in) & 15u) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    const uint4* p4 = reinterpret_cast<const uint4*>(src - L);
    for (uint32_t k = t; k < L / 16u; k += T) {
      reinterpret_cast<uint4*>(cur)[k] = s4[k];
      reinterpret_cast<uint4*>(prev)[k] = r > 0 ? p4[k] : make_uint4(0, 0, 0, 0);
    }
  } else {
    for (uint32_t k = t; k < L; k += T) {
      cur[k] = src[k];
      prev[k] = r > 0 ? src[(ptrdiff_t)k - (ptrdiff_t)L] : (uint8_t)0;
    }
  }
  __syncthreads();

  // ---- filter choice: the smallest sum of |filtered byte as int8| over None, Sub, Up, Average, Paeth ---------------------
  uint32_t cost[5] = {0, 0, 0, 0, 0};
  for (uint32_t i = t; i < L; i += T) {
    const uint32_t x = cur[i], b = prev[i];
    const uint32_t a = i >= (uint32_t)c ? cur[i - c] : 0u, cc = i >= (uint32_t)c ? prev[i - c] : 0u;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const uint32_t v = png_filter(f, x, a, b, cc);
      cost[f] += v < 128u ? v : 256u - v;
    }
  }
  uint32_t total[5];
#pragma unroll
  for (int f = 0; f < 5; ++f) total[f] = block_sum(scratch, cost[f]);
  int best = 0;
#pragma unroll
  for (int f = 1; f < 5; ++f)
    if (total[f] < total[best]) best = f;

  // ---- filtered bytes d[0 .. m) (d[0] = the filter type) and the row's Adler-32 part:
  //      s1 = sum d[k], s2 = sum (m - k) d[k]  (what the row adds to A, and to B beyond m * A) ------------------------------
  uint32_t s1 = 0, s2 = 0;                 // per thread at most 49 terms of at most 255 * 12 289: no overflow
  for (uint32_t i = t; i < L; i += T) {
    const uint32_t x = cur[i], b = prev[i];
    const uint32_t a = i >= (uint32_t)c ? cur[i - c] : 0u, cc = i >= (uint32_t)c ? prev[i - c] : 0u;
    const uint32_t v = png_filter(best, x, a, b, cc);
    d[1u + i] = (uint8_t)v;
    s1 += v;
    s2 += (m - 1u - i) * v;
  }
  if (t == 0) {
    d[0] = (uint8_t)best;
    s1 += (uint32_t)best;
    s2 += m * (uint32_t)best;
  }
  s1 = block_sum(scratch, s1 % ADLER_MOD);
  s2 = block_sum(scratch, s2 % ADLER_MOD);   // the barriers inside also order d[] and free cur / prev
  if (t == 0) {
    row_s1[idx] = s1 % ADLER_MOD;
    row_s2[idx] = s2 % ADLER_MOD;
  }

  // ---- greedy parse: at i take the longer of the runs d[i..] == d[i-1..] and d[i..] == d[i-c..] (3..258 bytes, inside the
  //      row), else a literal.  Each thread owns a contiguous piece; the run lengths come from a backward walk that starts
  //      from the first mismatch in the pieces to the right. ------------------------------------------------------------
  const uint32_t piece = (m + T - 1u) / T;
  const uint32_t lo = (uint32_t)t * piece < m ? (uint32_t)t * piece : m;
  const uint32_t hi = lo + piece < m ? lo + piece : m;
  uint32_t* ff1 = scratch;                  // first position of the piece where the distance-1 / distance-c run breaks
  uint32_t* ffc = scratch + T;
  {
    uint32_t f1 = m, fc = m;
    for (uint32_t i = lo; i < hi; ++i) {
      const bool e1 = i >= 1u && d[i] == d[i - 1u];
      const bool ec = i >= (uint32_t)c && d[i] == d[i - c];
      if (!e1 && f1 == m) f1 = i;
      if (!ec && fc == m) fc = i;
    }
    ff1[t] = f1;
    ffc[t] = fc;
  }
  __syncthreads();
  {
    uint32_t end1 = m, endc = m;            // first break at or after hi (m: the end of the row)
    for (int u = t + 1; u < T && end1 == m; ++u) end1 = ff1[u];
    for (int u = t + 1; u < T && endc == m; ++u) endc = ffc[u];
    for (uint32_t i = hi; i-- > lo;) {
      if (!(i >= 1u && d[i] == d[i - 1u])) end1 = i;
      if (!(i >= (uint32_t)c && d[i] == d[i - c])) endc = i;
      const uint32_t r1 = end1 > i ? end1 - i : 0u, rc = endc > i ? endc - i : 0u;
      uint32_t n = r1 > rc ? r1 : rc;
      n = n < 258u ? n : 258u;
      if (n >= 3u) {
        j0[i] = (uint16_t)(i + n);
        lenm3[i] = (uint8_t)(n - 3u);
        flags[i] = (uint8_t)(2u | (rc > r1 ? 4u : 0u));
      } else {
        j0[i] = (uint16_t)(i + 1u);
        flags[i] = 0;
      }
    }
    if (t == 0) {
      j0[m] = (uint16_t)m;                  // the end of the row points at itself
      flags[m] = 0;
    }
  }
  __syncthreads();
  if (t == 0) flags[0] |= 1u;
  __syncthreads();
  // the token starts are the positions on the chain 0 -> j[0] -> j[j[0]] ...: pointer jumping, after round k every position
  // within 2^k hops of 0 is marked and jump[] spans 2^k hops.  A mark seen early only marks further chain positions, so the
  // result does not depend on the order of the threads.
  {
    uint16_t* a = j0;
    uint16_t* b = j1;
    for (uint32_t span = 1; span < m; span <<= 1) {
      for (uint32_t i = t; i <= m; i += T) {
        const uint32_t j = a[i];
        if (flags[i] & 1u) flags[j] |= 1u;
        b[i] = a[j];
      }
      __syncthreads();
      uint16_t* x = a;
      a = b;
      b = x;
    }
  }

  // ---- level 2: the tokens' histogram, a code built from it, the sizes of the three codings, the choice ------------------
  [[maybe_unused]] uint32_t mode = PNG_FIXED, n_mode = 0, dyn_bits = 0;
  if constexpr (LEVEL == 2) {
    PNG_HUFFMAN_LDS(smem + o.total);
    uint32_t* sorted = reinterpret_cast<uint32_t*>(hs + PNG_H_SORTED);
    uint16_t* order = codes;
    for (uint32_t k = t; k < PNG_SYMS; k += T) hist[k] = 0;
    for (uint32_t k = t; k < 320u; k += T) lens[k] = 0;
    __syncthreads();
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t f = flags[i];
      if (!(f & 1u)) continue;
      uint32_t eb, ev;
      atomicAdd(&hist[(f & 2u) ? length_symbol(lenm3[i], eb, ev) : (uint32_t)d[i]], 1u);
    }
    if (t == 0) atomicAdd(&hist[256], 1u);                 // the end of block
    __syncthreads();
    // used symbols in ascending order of (count, symbol): every symbol counts the ones before it
    uint32_t used = 0;
    for (uint32_t s = t; s < (uint32_t)png_huff::NUM_LITLEN; s += T) {
      const uint32_t cnt = hist[s];
      uint32_t rank = 0;
      used = 0;
      for (uint32_t u = 0; u < (uint32_t)png_huff::NUM_LITLEN; ++u) {
        const uint32_t cu = hist[u];
        used += cu != 0u ? 1u : 0u;
        rank += (cu != 0u && (cu < cnt || (cu == cnt && u < s))) ? 1u : 0u;
      }
      if (cnt) {
        sorted[rank] = cnt;
        order[rank] = (uint16_t)s;
      }
    }
    __syncthreads();
    if (t == 0) {                                          // the serial part (png_huffman.h), one lane
      png_huff::lengths_from_sorted(sorted, order, (int)used, png_huff::MAX_BITS, lens);
      uint32_t nlit = png_huff::NUM_LITLEN;
      while (nlit > 257u && lens[nlit - 1u] == 0) --nlit;
      png_huff::codes_from_lengths(lens, (int)nlit, codes);
      lens[nlit] = 1;                                      // the distance code's lengths follow in the header's sequence
      lens[nlit + 1u] = c == 1 ? 1 : 0;
      lens[nlit + 2u] = 1;
      const uint32_t ndist = c == 1 ? 2u : 3u;
      const uint32_t ntok = (uint32_t)png_huff::header_tokens(lens, (int)(nlit + ndist), hdr_tokens, cl->counts);
      const int cl_used = png_huff::sort_counts(cl->counts, png_huff::NUM_CL, cl->sorted, cl->order);
      for (int k = 0; k < png_huff::NUM_CL; ++k) cl->lens[k] = 0;
      png_huff::lengths_from_sorted(cl->sorted, cl->order, cl_used, png_huff::CL_MAX_BITS, cl->lens);
      png_huff::codes_from_lengths(cl->lens, png_huff::NUM_CL, cl->codes);
      uint32_t hclen = png_huff::NUM_CL;
      while (hclen > 4u && cl->lens[png_huff::cl_order((int)hclen - 1)] == 0) --hclen;
      uint32_t hb = 5u + 5u + 4u + 3u * hclen;
      for (uint32_t k = 0; k < (uint32_t)png_huff::NUM_CL; ++k) hb += cl->counts[k] * (cl->lens[k] + png_huff::cl_extra_bits(k));
      cl->nlit = nlit, cl->ndist = ndist, cl->ntok = ntok, cl->hclen = hclen, cl->header_bits = hb;
    }
    __syncthreads();
    uint32_t fb = 0, db = 0;                               // bits of all tokens and the end of block under either code
    for (uint32_t s = t; s < (uint32_t)png_huff::NUM_LITLEN; s += T) {
      const uint32_t cnt = hist[s], x = symbol_extra_bits(s);
      fb += cnt * (fixed_code_bits(s) + x + (s > 256u ? 5u : 0u));
      db += cnt * (lens[s] + x + (s > 256u ? 1u : 0u));
    }
    fb = block_sum(scratch, fb);
    db = block_sum(scratch, db);
    // block header | tokens, end of block | stored block: 3 bits, padding, 00 00 FF FF
    const uint32_t n_fixed = (3u + fb + 3u + 7u) / 8u + 4u;
    const uint32_t n_dynamic = (3u + cl->header_bits + db + 3u + 7u) / 8u + 4u;
    const uint32_t n_stored = 1u + 4u + m + 1u + 4u;       // header and padding, LEN / NLEN, the bytes, the empty block
    n_mode = n_fixed;
    if (n_dynamic < n_mode) mode = PNG_DYNAMIC, n_mode = n_dynamic;
    if (n_stored < n_mode) mode = PNG_STORED, n_mode = n_stored;
    dyn_bits = db;
  }

  // the token that starts at i (f = flags[i]) under the row's code, fixed or dynamic -> its value, nb: its bits
  auto token = [&](uint32_t i, uint32_t f, uint32_t& nb) -> uint32_t {
    if constexpr (LEVEL == 2) {
      if (mode == PNG_DYNAMIC) {
        PNG_HUFFMAN_LDS(smem + o.total);
        if (f & 2u) return dynamic_match_token(lenm3[i], (f & 4u) != 0, codes, lens, nb);
        nb = lens[d[i]];
        return codes[d[i]];
      }
    }
    return (f & 2u) ? match_token(lenm3[i], (f & 4u) != 0, nb) : literal_token(d[i], nb);
  };

  // ---- bit offsets of the tokens: sum per piece, exclusive scan over the pieces ------------------------------------------
  uint32_t bits = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t f = flags[i];
    if (!(f & 1u)) continue;
    uint32_t nb;
    token(i, f, nb);
    bits += nb;
  }
  scratch[t] = bits;
  __syncthreads();
  row_files::scan(scratch);
  const uint32_t token_bits = scratch[T - 1];
  uint32_t pos = 3u + scratch[t] - bits;
  // block: BFINAL 0, BTYPE 01 | tokens | end of block (7 zero bits) | stored block: BFINAL 0, BTYPE 00, padding, 00 00 FF FF
  uint32_t n = (3u + token_bits + 7u + 3u + 7u) / 8u + 4u;             // bytes of this row's deflate data
  if constexpr (LEVEL == 2) {
    PNG_HUFFMAN_LDS(smem + o.total);
    n = n_mode;
    if (mode == PNG_DYNAMIC) pos += cl->header_bits;
  }
  const uint32_t bb_words = png_round_up(png_row_data_max(m) + 8u, 16u) / 4u;
  for (uint32_t k = t; k < bb_words; k += T) bb[k] = 0;            // j0 / j1 are dead: the bit buffer takes their place
  __syncthreads();
  if constexpr (LEVEL == 2) {
    PNG_HUFFMAN_LDS(smem + o.total);
    if (mode == PNG_STORED) {                // 00 | LEN, NLEN | the filtered bytes | 00 | 00 00 FF FF, all with byte stores
      uint8_t* b8 = reinterpret_cast<uint8_t*>(bb);
      for (uint32_t k = t; k < m; k += T) b8[5u + k] = d[k];
      if (t == 0) {
        b8[1] = (uint8_t)m, b8[2] = (uint8_t)(m >> 8);
        b8[3] = (uint8_t)~m, b8[4] = (uint8_t)(~m >> 8);
        b8[n - 2u] = 0xFF, b8[n - 1u] = 0xFF;
      }
    } else if (t == 0) {
      emit_bits(bb, 0, mode << 1, 3);
      emit_bits(bb, (n - 2u) * 8u, 0xFFFFu, 16);
      if (mode == PNG_DYNAMIC) {             // HLIT, HDIST, HCLEN | the code-length code | the run-length coded lengths
        uint32_t p = 3u;
        emit_bits(bb, p, cl->nlit - 257u, 5), p += 5u;
        emit_bits(bb, p, cl->ndist - 1u, 5), p += 5u;
        emit_bits(bb, p, cl->hclen - 4u, 4), p += 4u;
        for (uint32_t k = 0; k < cl->hclen; ++k, p += 3u) emit_bits(bb, p, cl->lens[png_huff::cl_order((int)k)], 3);
        for (uint32_t k = 0; k < cl->ntok; ++k) {
          const uint32_t sym = hdr_tokens[k] & 31u, extra = hdr_tokens[k] >> 5, hb = cl->lens[sym];
          const uint32_t nb = hb + png_huff::cl_extra_bits(sym);
          emit_bits(bb, p, cl->codes[sym] | (extra << hb), nb);
          p += nb;
        }
        emit_bits(bb, p + dyn_bits - lens[256], codes[256], lens[256]);      // the end of block, behind the tokens
      }
    }
  } else if (t == 0) {
    emit_bits(bb, 0, 2u, 3);
    emit_bits(bb, (n - 2u) * 8u, 0xFFFFu, 16);
  }
  for (uint32_t i = lo; i < hi && mode != PNG_STORED; ++i) {
    const uint32_t f = flags[i];
    if (!(f & 1u)) continue;
    uint32_t nb;
    const uint32_t v = token(i, f, nb);
    emit_bits(bb, pos, v, nb);
    pos += nb;
  }
  __syncthreads();

  // ---- CRC-32 of "IDAT" [78 01] data: every thread takes k bytes of the data (right-aligned, so that all pieces but the
  //      leading ones are full; leading zeros do not change a register that starts at 0), then a tree in which the left
  //      half is multiplied by x^(8 * bytes of the right half) ---------------------------------------------------------------
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(bb);
  {
    const uint32_t k = (n + T - 1u) / T;
    const int end = (int)n - (T - 1 - t) * (int)k;
    const int begin = end - (int)k;
    uint32_t crc = 0;
    for (int i = begin > 0 ? begin : 0; i < end; ++i) crc = crc_byte(crc, bytes[i]);
    scratch[t] = crc;
    uint32_t xp = gf_pow_x8(k);
    for (int s = 1; s < T; s <<= 1) {
      __syncthreads();
      if ((t & (2 * s - 1)) == 0) scratch[t] = gf_mul(scratch[t], xp) ^ scratch[t + s];
      xp = gf_mul(xp, xp);
    }
    __syncthreads();
  }
  uint8_t* slot = staging + idx * slot_bytes;
  const uint32_t hdr = r == 0 ? 10u : 8u;
  if (t == 0) {
    uint8_t* hp = slot + 16u - hdr;
    put_be32(hp, n + hdr - 8u);
    hp[4] = 'I', hp[5] = 'D', hp[6] = 'A', hp[7] = 'T';
    if (r == 0) hp[8] = 0x78, hp[9] = 0x01;               // zlib header: deflate, 32 KiB window, fastest level, no dictionary
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t i = 4; i < hdr; ++i) reg = crc_byte(reg, hp[i]);
    reg = gf_mul(reg, gf_pow_x8(n)) ^ scratch[0];
    put_be32(reinterpret_cast<uint8_t*>(bb) + n, ~reg);    // the CRC follows the data in the bit buffer
    row_size[idx] = hdr + n + 4u;
  }
  __syncthreads();
  uint32_t* dst = reinterpret_cast<uint32_t*>(slot + 16u);
  for (uint32_t k = t; k < (n + 4u + 3u) / 4u; k += T) dst[k] = bb[k];
}

// one workgroup per image
__global__ __launch_bounds__(T) void png_finish_kernel(int h, int w, int c, const uint32_t* __restrict__ row_size,
                                                           const uint32_t* __restrict__ row_s1,
                                                           const uint32_t* __restrict__ row_s2, uint32_t* __restrict__ row_off,
                                                           uint8_t* __restrict__ out, size_t out_pitch,
                                                           long long* __restrict__ sizes) {
  __shared__ uint32_t scratch[T];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * h;
  const uint32_t m = (uint32_t)w * (uint32_t)c + 1u;
  // the rows' chunks follow the signature and IHDR, one behind the other
  const uint32_t running = row_files::row_offsets(scratch, row_size + base, row_off + base, h, 8u + 25u, 0u);
  // Adler-32 of all filtered rows from the rows' parts.  Row i turns (A, B) into (A + s1_i, B + m A + s2_i); from (1, 0):
  //   A = 1 + sum s1_i,   B = m h + m sum s1_i (h - 1 - i) + sum s2_i        (mod 65521)
  uint32_t a_part = 0, b1_part = 0, b2_part = 0;
  for (int r = t; r < h; r += T) {
    const uint32_t s1 = row_s1[base + r];
    a_part = (a_part + s1) % ADLER_MOD;
    b1_part = (b1_part + s1 * ((uint32_t)(h - 1 - r) % ADLER_MOD) % ADLER_MOD) % ADLER_MOD;
    b2_part = (b2_part + row_s2[base + r]) % ADLER_MOD;
  }
  const uint32_t a_sum = block_sum(scratch, a_part) % ADLER_MOD;       // 256 terms below 65521: no overflow
  const uint32_t b1_sum = block_sum(scratch, b1_part) % ADLER_MOD;
  const uint32_t b2_sum = block_sum(scratch, b2_part) % ADLER_MOD;
  if (t != 0) return;
  const uint32_t adler_a = (1u + a_sum) % ADLER_MOD;
  const uint32_t mh = (m % ADLER_MOD) * ((uint32_t)h % ADLER_MOD) % ADLER_MOD;
  const uint32_t adler_b = (mh + (m % ADLER_MOD) * b1_sum % ADLER_MOD + b2_sum) % ADLER_MOD;
  uint8_t* f = out + (size_t)blockIdx.x * out_pitch;
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  for (int i = 0; i < 8; ++i) f[i] = sig[i];
  uint8_t* p = f + 8;
  put_be32(p, 13u);
  p[4] = 'I', p[5] = 'H', p[6] = 'D', p[7] = 'R';
  put_be32(p + 8, (uint32_t)w);
  put_be32(p + 12, (uint32_t)h);
  p[16] = 8;                                // bit depth
  p[17] = c == 3 ? 2 : 0;                   // colour type: RGB / grey
  p[18] = 0, p[19] = 0, p[20] = 0;          // deflate, adaptive filtering, no interlace
  uint32_t reg = 0xFFFFFFFFu;
  for (int i = 4; i < 21; ++i) reg = crc_byte(reg, p[i]);
  put_be32(p + 21, ~reg);
  p = f + running;                          // behind the last row's chunk
  put_be32(p, 6u);
  p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
  p[8] = 0x03, p[9] = 0x00;                 // BFINAL 1, BTYPE 01, end of block
  put_be32(p + 10, (adler_b << 16) | adler_a);
  reg = 0xFFFFFFFFu;
  for (int i = 4; i < 14; ++i) reg = crc_byte(reg, p[i]);
  put_be32(p + 14, ~reg);
  p += 18;
  put_be32(p, 0u);
  p[4] = 'I', p[5] = 'E', p[6] = 'N', p[7] = 'D';
  put_be32(p + 8, 0xAE426082u);
  sizes[blockIdx.x] = (long long)running + 18 + 12;
}

// one workgroup per (row, image): the chunk, from its right-aligned header on
__global__ __launch_bounds__(T) void png_gather_kernel(int h, const uint32_t* __restrict__ row_size,
                                                           const uint32_t* __restrict__ row_off,
                                                           const uint8_t* __restrict__ staging, uint32_t slot_bytes,
                                                           uint8_t* __restrict__ out, size_t out_pitch) {
  const int r = blockIdx.x;
  const size_t idx = (size_t)blockIdx.y * h + r;
  row_files::copy_row(staging + idx * slot_bytes, r == 0 ? 6u : 8u, row_size[idx],
                      out + (size_t)blockIdx.y * out_pitch + row_off[idx]);
}

bool png_shape_ok(const char* what, int64_t n, int32_t h, int32_t w, int32_t c) {
  if (!row_files::channels_ok(what, c)) return false;
  if (w < 1 || w > row_files::MAX_W) {
    cgan_set_error("%s: w = %d: rows of 1 to %d pixels only", what, w, row_files::MAX_W);
    return false;
  }
  if (!row_files::grid_ok(n, h)) {
    cgan_set_error("%s: n = %lld, h = %d: 1 <= n <= 65535, h >= 1 and n * h < 2^31 expected", what, (long long)n, h);
    return false;
  }
  return row_files::file_fits(what, h, w, c, PNG_FIXED_BYTES + (uint64_t)h * (12u + png_row_data_max((uint32_t)w * c + 1u)));
}

}  // namespace

extern "C" size_t cgan_png_bound_bytes(int32_t h, int32_t w, int32_t c) {
  if (!png_shape_ok("cgan_png_bound_bytes", 1, h, w, c)) return 0;
  return PNG_FIXED_BYTES + (size_t)h * (12u + png_row_data_max((uint32_t)w * c + 1u));
}

extern "C" size_t cgan_png_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (!png_shape_ok("cgan_png_workspace_bytes", n, h, w, c)) return 0;
  const int64_t rows = (int64_t)n * h;
  return 4 * row_files::table_bytes(rows) + (size_t)rows * png_slot_bytes((uint32_t)w * c + 1u);
}

extern "C" int cgan_png_huffman_lengths(const uint32_t* counts, int32_t n, int32_t limit, uint8_t* lengths) {
  CGAN_REQUIRE(counts && lengths, "cgan_png_huffman_lengths: null pointer");
  CGAN_REQUIRE(n >= 1 && n <= 65535 && limit >= 1 && limit <= png_huff::MAX_BITS,
               "cgan_png_huffman_lengths: n = %d, limit = %d: 1 <= n <= 65535 and 1 <= limit <= %d expected", n, limit,
               png_huff::MAX_BITS);
  std::vector<uint32_t> sorted((size_t)n);
  std::vector<uint16_t> order((size_t)n);
  const int used = png_huff::sort_counts(counts, n, sorted.data(), order.data());
  CGAN_REQUIRE((int64_t)used <= (int64_t)1 << limit, "cgan_png_huffman_lengths: %d used symbols do not fit codes of %d bits",
               used, limit);
  uint64_t sum = 0;
  for (int k = 0; k < used; ++k) sum += sorted[(size_t)k];
  CGAN_REQUIRE(sum <= 0xffffffffull, "cgan_png_huffman_lengths: the counts sum to %llu, above 2^32 - 1",
               (unsigned long long)sum);
  for (int32_t s = 0; s < n; ++s) lengths[s] = 0;
  png_huff::lengths_from_sorted(sorted.data(), order.data(), used, limit, lengths);
  return CGAN_OK;
}

extern "C" int cgan_png_encode_u8_level(const uint8_t* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t level,
                                        uint8_t* out, size_t out_pitch, int64_t* sizes, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  CGAN_REQUIRE(in && out && sizes && workspace, "cgan_png_encode_u8: null pointer");
  CGAN_REQUIRE(level == 1 || level == 2, "cgan_png_encode_u8: level = %d: 1 (fixed Huffman) or 2 (per-row choice) only", level);
  if (!png_shape_ok("cgan_png_encode_u8", n, h, w, c)) return CGAN_ERR_BAD_ARG;
  if (const int rc = row_files::buffers_ok("cgan_png_encode_u8", out_pitch, cgan_png_bound_bytes(h, w, c), workspace,
                                          workspace_bytes, cgan_png_workspace_bytes(n, h, w, c)))
    return rc;
  const uint32_t m = (uint32_t)w * c + 1u;
  const int64_t all_rows = (int64_t)n * h;
  uint32_t* row_size = row_files::table(workspace, all_rows, 0);
  uint32_t* row_s1 = row_files::table(workspace, all_rows, 1);
  uint32_t* row_s2 = row_files::table(workspace, all_rows, 2);
  uint32_t* row_off = row_files::table(workspace, all_rows, 3);
  uint8_t* staging = reinterpret_cast<uint8_t*>(row_files::table(workspace, all_rows, 4));
  const uint32_t slot = png_slot_bytes(m);
  const PngLds lds = png_lds(m);
  auto* rows = level == 2 ? &png_rows_kernel<2> : &png_rows_kernel<1>;
  const uint32_t lds_bytes = lds.total + (level == 2 ? PNG_H_BYTES : 0u);
  static bool attr_set[2] = {false, false};
  if (!attr_set[level - 1]) {                // the widest rows need more than the 64 KiB a launch gets by default
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rows), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) {
      cgan_set_error("cgan_png_encode_u8: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return CGAN_ERR_HIP;
    }
    attr_set[level - 1] = true;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rows, dim3(h, n), dim3(T), lds_bytes, s, in, h, w * c, c, row_size, row_s1, row_s2, staging, slot);
  CGAN_CHECK_LAUNCH("cgan_png_encode_u8 (rows)");
  hipLaunchKernelGGL(png_finish_kernel, dim3(n), dim3(T), 0, s, h, w, c, row_size, row_s1, row_s2, row_off, out,
                     out_pitch, reinterpret_cast<long long*>(sizes));
  CGAN_CHECK_LAUNCH("cgan_png_encode_u8 (finish)");
  hipLaunchKernelGGL(png_gather_kernel, dim3(h, n), dim3(T), 0, s, h, row_size, row_off, staging, slot, out, out_pitch);
  CGAN_CHECK_LAUNCH("cgan_png_encode_u8 (gather)");
  return CGAN_OK;
}

extern "C" int cgan_png_encode_u8(const uint8_t* in, int32_t n, int32_t h, int32_t w, int32_t c, uint8_t* out,
                                  size_t out_pitch, int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
  return cgan_png_encode_u8_level(in, n, h, w, c, 1, out, out_pitch, sizes, workspace, workspace_bytes, stream);
}
