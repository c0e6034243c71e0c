// PNG encoder on the device: uint8 [n, h, w, c] images (c = 1 grey, c = 3 RGB) -> one complete PNG file per
// image in device memory.  The host computes sizes and launches; every byte of the files is produced by the kernels below.
//
// File layout:  signature | IHDR | one IDAT per row | one closing IDAT | IEND.  The IDAT payloads form one zlib stream:
//   78 01 | per row: [fixed-Huffman block (BFINAL 0), empty stored block (pads to a byte: .. 00 00 FF FF)] | 03 00 (final
//   empty fixed block) | Adler-32.
// Every row therefore encodes independently of every other one and ends on a byte boundary (the way pigz joins the output of
// its threads), and every row's chunk carries its own CRC-32.
//
//   png_rows_kernel    one workgroup per (row, image): filter choice, deflate, CRC, the row's Adler-32 part -> staging slot
//   png_finish_kernel  one workgroup per image: signature, IHDR, row offsets (exclusive scan of the chunk sizes), the
//                      combined Adler-32, closing IDAT, IEND, the file's length
//   png_gather_kernel  one workgroup per (row, image): the row's chunk from its staging slot to its place in the file
//
// No atomics on global memory and fixed-order reductions: the bytes of an image do not depend on the batch it is in or on
// the run.
#include "cgan_common.h"

namespace {

constexpr int PNG_T = 256;                  // threads per workgroup, all three kernels
constexpr int PNG_MAX_W = 4096;             // widest row: 4096 pixels (12 288 filtered bytes as RGB)
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
  o.total = o.scratch + 5u * PNG_T * 4u;
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
// l = length - 3 (0..255), dist_c: distance 3 instead of 1
__device__ inline uint32_t match_token(uint32_t l, bool dist3, uint32_t& nbits) {
  uint32_t code, eb = 0, ev = 0;
  if (l < 8u) {
    code = 257u + l;
  } else if (l == 255u) {
    code = 285u;
  } else {
    eb = (31u - (uint32_t)__clz(l)) - 2u;
    code = 261u + 4u * eb + ((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
  }
  const uint32_t hb = code < 280u ? 7u : 8u;
  const uint32_t huff = code < 280u ? code - 256u : 0xC0u + (code - 280u);
  // distance codes 0 (distance 1) and 2 (distance 3): 5 bits, no extra bits; 00010 reversed = 01000
  const uint32_t dist = dist3 ? 8u : 0u;
  nbits = hb + eb + 5u;
  return bit_rev(huff, hb) | (ev << hb) | (dist << (hb + eb));
}
__device__ inline void emit_bits(uint32_t* bb, uint32_t pos, uint32_t v, uint32_t nbits) {
  const uint32_t wi = pos >> 5, sh = pos & 31u;
  atomicOr(&bb[wi], v << sh);
  if (sh + nbits > 32u) atomicOr(&bb[wi + 1u], v >> (32u - sh));
}

// sum over the workgroup, returned to every thread; s: PNG_T words of LDS
__device__ inline uint32_t block_sum(uint32_t* s, uint32_t v) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int k = PNG_T / 2; k > 0; k >>= 1) {
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

// one workgroup per (row, image).  row_len = w * c bytes.
__global__ __launch_bounds__(PNG_T) void png_rows_kernel(const uint8_t* __restrict__ in, int h, int row_len, int c,
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
    for (uint32_t k = t; k < L / 16u; k += PNG_T) {
      reinterpret_cast<uint4*>(cur)[k] = s4[k];
      reinterpret_cast<uint4*>(prev)[k] = r > 0 ? p4[k] : make_uint4(0, 0, 0, 0);
    }
  } else {
    for (uint32_t k = t; k < L; k += PNG_T) {
      cur[k] = src[k];
      prev[k] = r > 0 ? src[(ptrdiff_t)k - (ptrdiff_t)L] : (uint8_t)0;
    }
  }
  __syncthreads();

  // ---- filter choice: the smallest sum of |filtered byte as int8| over None, Sub, Up, Average, Paeth ---------------------
  uint32_t cost[5] = {0, 0, 0, 0, 0};
  for (uint32_t i = t; i < L; i += PNG_T) {
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
  for (uint32_t i = t; i < L; i += PNG_T) {
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
  const uint32_t piece = (m + PNG_T - 1u) / PNG_T;
  const uint32_t lo = (uint32_t)t * piece < m ? (uint32_t)t * piece : m;
  const uint32_t hi = lo + piece < m ? lo + piece : m;
  uint32_t* ff1 = scratch;                  // first position of the piece where the distance-1 / distance-c run breaks
  uint32_t* ffc = scratch + PNG_T;
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
    for (int u = t + 1; u < PNG_T && end1 == m; ++u) end1 = ff1[u];
    for (int u = t + 1; u < PNG_T && endc == m; ++u) endc = ffc[u];
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
      for (uint32_t i = t; i <= m; i += PNG_T) {
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

  // ---- bit offsets of the tokens: sum per piece, exclusive scan over the pieces ------------------------------------------
  uint32_t bits = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t f = flags[i];
    if (!(f & 1u)) continue;
    uint32_t nb;
    if (f & 2u) match_token(lenm3[i], (f & 4u) != 0, nb);
    else literal_token(d[i], nb);
    bits += nb;
  }
  scratch[t] = bits;
  __syncthreads();
  for (int s = 1; s < PNG_T; s <<= 1) {
    const uint32_t x = t >= s ? scratch[t - s] : 0u;
    __syncthreads();
    scratch[t] += x;
    __syncthreads();
  }
  const uint32_t token_bits = scratch[PNG_T - 1];
  uint32_t pos = 3u + scratch[t] - bits;
  // block: BFINAL 0, BTYPE 01 | tokens | end of block (7 zero bits) | stored block: BFINAL 0, BTYPE 00, padding, 00 00 FF FF
  const uint32_t n = (3u + token_bits + 7u + 3u + 7u) / 8u + 4u;       // bytes of this row's deflate data
  const uint32_t bb_words = png_round_up(png_row_data_max(m) + 8u, 16u) / 4u;
  for (uint32_t k = t; k < bb_words; k += PNG_T) bb[k] = 0;            // j0 / j1 are dead: the bit buffer takes their place
  __syncthreads();
  if (t == 0) {
    emit_bits(bb, 0, 2u, 3);
    emit_bits(bb, (n - 2u) * 8u, 0xFFFFu, 16);
  }
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t f = flags[i];
    if (!(f & 1u)) continue;
    uint32_t nb;
    const uint32_t v = (f & 2u) ? match_token(lenm3[i], (f & 4u) != 0, nb) : literal_token(d[i], nb);
    emit_bits(bb, pos, v, nb);
    pos += nb;
  }
  __syncthreads();

  // ---- CRC-32 of "IDAT" [78 01] data: every thread takes k bytes of the data (right-aligned, so that all pieces but the
  //      leading ones are full; leading zeros do not change a register that starts at 0), then a tree in which the left
  //      half is multiplied by x^(8 * bytes of the right half) ---------------------------------------------------------------
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(bb);
  {
    const uint32_t k = (n + PNG_T - 1u) / PNG_T;
    const int end = (int)n - (PNG_T - 1 - t) * (int)k;
    const int begin = end - (int)k;
    uint32_t crc = 0;
    for (int i = begin > 0 ? begin : 0; i < end; ++i) crc = crc_byte(crc, bytes[i]);
    scratch[t] = crc;
    uint32_t xp = gf_pow_x8(k);
    for (int s = 1; s < PNG_T; s <<= 1) {
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
  for (uint32_t k = t; k < (n + 4u + 3u) / 4u; k += PNG_T) dst[k] = bb[k];
}

// one workgroup per image
__global__ __launch_bounds__(PNG_T) void png_finish_kernel(int h, int w, int c, const uint32_t* __restrict__ row_size,
                                                           const uint32_t* __restrict__ row_s1,
                                                           const uint32_t* __restrict__ row_s2, uint32_t* __restrict__ row_off,
                                                           uint8_t* __restrict__ out, size_t out_pitch,
                                                           long long* __restrict__ sizes) {
  __shared__ uint32_t scratch[PNG_T];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * h;
  const uint32_t m = (uint32_t)w * (uint32_t)c + 1u;
  // offsets of the rows' chunks: exclusive scan of their sizes, PNG_T rows at a time
  uint32_t running = 8u + 25u;
  for (int r0 = 0; r0 < h; r0 += PNG_T) {
    const int r = r0 + t;
    const uint32_t v = r < h ? row_size[base + r] : 0u;
    scratch[t] = v;
    __syncthreads();
    for (int s = 1; s < PNG_T; s <<= 1) {
      const uint32_t x = t >= s ? scratch[t - s] : 0u;
      __syncthreads();
      scratch[t] += x;
      __syncthreads();
    }
    if (r < h) row_off[base + r] = running + scratch[t] - v;
    running += scratch[PNG_T - 1];
    __syncthreads();
  }
  // Adler-32 of all filtered rows from the rows' parts.  Row i turns (A, B) into (A + s1_i, B + m A + s2_i); from (1, 0):
  //   A = 1 + sum s1_i,   B = m h + m sum s1_i (h - 1 - i) + sum s2_i        (mod 65521)
  uint32_t a_part = 0, b1_part = 0, b2_part = 0;
  for (int r = t; r < h; r += PNG_T) {
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

// one workgroup per (row, image): the chunk starts at any byte offset of the file, so it moves byte by byte
__global__ __launch_bounds__(PNG_T) void png_gather_kernel(int h, const uint32_t* __restrict__ row_size,
                                                           const uint32_t* __restrict__ row_off,
                                                           const uint8_t* __restrict__ staging, uint32_t slot_bytes,
                                                           uint8_t* __restrict__ out, size_t out_pitch) {
  const int r = blockIdx.x;
  const size_t idx = (size_t)blockIdx.y * h + r;
  const uint32_t size = row_size[idx];
  const uint8_t* src = staging + idx * slot_bytes + (r == 0 ? 6u : 8u);
  uint8_t* dst = out + (size_t)blockIdx.y * out_pitch + row_off[idx];
  for (uint32_t k = threadIdx.x; k < size; k += PNG_T) dst[k] = src[k];
}

bool png_shape_ok(const char* what, int64_t n, int32_t h, int32_t w, int32_t c) {
  if (c != 1 && c != 3) {
    cgan_set_error("%s: c = %d: 8-bit grey (1) or RGB (3) only", what, c);
    return false;
  }
  if (w < 1 || w > PNG_MAX_W) {
    cgan_set_error("%s: w = %d: rows of 1 to %d pixels only", what, w, PNG_MAX_W);
    return false;
  }
  if (h < 1 || n < 1 || n > 65535 || n * (int64_t)h > 0x7fffffffll) {
    cgan_set_error("%s: n = %lld, h = %d: 1 <= n <= 65535, h >= 1 and n * h < 2^31 expected", what, (long long)n, h);
    return false;
  }
  const uint64_t bound = PNG_FIXED_BYTES + (uint64_t)h * (12u + png_row_data_max((uint32_t)w * c + 1u));
  if (bound > 0x7fffffffull) {
    cgan_set_error("%s: a %d x %d x %d image may need %llu bytes, more than the 2^31 - 1 one file may have", what, h, w, c,
                   (unsigned long long)bound);
    return false;
  }
  return true;
}

size_t png_table_bytes(int64_t rows) { return (size_t)((rows * 4 + 15) / 16 * 16); }

}  // namespace

extern "C" size_t cgan_png_bound_bytes(int32_t h, int32_t w, int32_t c) {
  if (!png_shape_ok("cgan_png_bound_bytes", 1, h, w, c)) return 0;
  return PNG_FIXED_BYTES + (size_t)h * (12u + png_row_data_max((uint32_t)w * c + 1u));
}

extern "C" size_t cgan_png_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (!png_shape_ok("cgan_png_workspace_bytes", n, h, w, c)) return 0;
  const int64_t rows = (int64_t)n * h;
  return 4 * png_table_bytes(rows) + (size_t)rows * png_slot_bytes((uint32_t)w * c + 1u);
}

extern "C" int cgan_png_encode_u8(const uint8_t* in, int32_t n, int32_t h, int32_t w, int32_t c, uint8_t* out,
                                  size_t out_pitch, int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
  CGAN_REQUIRE(in && out && sizes && workspace, "cgan_png_encode_u8: null pointer");
  if (!png_shape_ok("cgan_png_encode_u8", n, h, w, c)) return CGAN_ERR_BAD_ARG;
  CGAN_REQUIRE(out_pitch >= cgan_png_bound_bytes(h, w, c), "cgan_png_encode_u8: out_pitch %zu is below the bound %zu",
               out_pitch, cgan_png_bound_bytes(h, w, c));
  if (workspace_bytes < cgan_png_workspace_bytes(n, h, w, c) || (reinterpret_cast<uintptr_t>(workspace) & 15u)) {
    cgan_set_error("cgan_png_encode_u8: workspace of %zu bytes (16-byte aligned) expected, got %zu at %p",
                   cgan_png_workspace_bytes(n, h, w, c), workspace_bytes, workspace);
    return CGAN_ERR_WORKSPACE;
  }
  const uint32_t m = (uint32_t)w * c + 1u;
  const size_t tb = png_table_bytes((int64_t)n * h);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* row_size = reinterpret_cast<uint32_t*>(ws);
  uint32_t* row_s1 = reinterpret_cast<uint32_t*>(ws + tb);
  uint32_t* row_s2 = reinterpret_cast<uint32_t*>(ws + 2 * tb);
  uint32_t* row_off = reinterpret_cast<uint32_t*>(ws + 3 * tb);
  uint8_t* staging = ws + 4 * tb;
  const uint32_t slot = png_slot_bytes(m);
  const PngLds lds = png_lds(m);
  static bool attr_set = false;
  if (!attr_set) {                           // the widest rows need more than the 64 KiB a launch gets by default
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&png_rows_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      cgan_set_error("cgan_png_encode_u8: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return CGAN_ERR_HIP;
    }
    attr_set = true;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(png_rows_kernel, dim3(h, n), dim3(PNG_T), lds.total, s, in, h, w * c, c, row_size, row_s1, row_s2,
                     staging, slot);
  CGAN_CHECK_LAUNCH("cgan_png_encode_u8 (rows)");
  hipLaunchKernelGGL(png_finish_kernel, dim3(n), dim3(PNG_T), 0, s, h, w, c, row_size, row_s1, row_s2, row_off, out,
                     out_pitch, reinterpret_cast<long long*>(sizes));
  CGAN_CHECK_LAUNCH("cgan_png_encode_u8 (finish)");
  hipLaunchKernelGGL(png_gather_kernel, dim3(h, n), dim3(PNG_T), 0, s, h, row_size, row_off, staging, slot, out, out_pitch);
  CGAN_CHECK_LAUNCH("cgan_png_encode_u8 (gather)");
  return CGAN_OK;
}
