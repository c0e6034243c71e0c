// JPEG encoder on the device: uint8 [n, h, w, c] images (c = 1 grey, c = 3 RGB) -> one complete baseline JPEG
// file per image in device memory.  The host computes sizes and launches; every byte of the files is produced by the
// kernels below (the tables and the serial logic they share with the host: jpeg_tables.h).
//
// File layout:  SOI | APP0 (JFIF) | DQT per table | SOF0 | DHT per table | DRI | SOS | per MCU row: entropy-coded data padded
// with ones to a byte [RSTm] | EOI.  The restart interval is one MCU row, so every row codes independently of every other
// one (its DC predictors start at 0) and ends on a byte boundary: the structure of the PNG encoder's rows (png.hip).
//
//   jpeg_rows_kernel    one workgroup per (MCU row, image), the row in segments of 256 pixels: colour conversion, chroma
//                       mean (4:2:0), DCT, quantisation, the blocks' code sizes, their scan, the codes into a bit buffer,
//                       FF stuffing -> the row's staging slot.  With a coefficient pointer it stops behind the quantisation
//                       and writes the coefficients instead (cgan_jpeg_coefficients_u8: the same device code).
//   jpeg_finish_kernel  one workgroup per image: the headers, the rows' offsets (exclusive scan of their sizes), EOI, the
//                       file's length
//   jpeg_gather_kernel  one workgroup per (MCU row, image): the row's data from its slot to its place, its RSTm behind it
// The assembly of a file from its rows (workgroup scan, row offsets, row copy, workspace tables) is row_files.h, shared with
// png.hip.
//
// No atomics on global memory and no order-dependent sums: the bytes of an image do not depend on the batch it is in or on
// the run.
#include "cgan_common.h"
#include "jpeg_tables.h"
#include "row_files.h"

namespace {

using jpeg_tab::Geometry;

using row_files::T;                         // threads per workgroup, all three kernels
constexpr int JPEG_MAX_H = 65535;           // SOF0 holds 16 bits
constexpr int SEG_PX = 256;                 // pixels of an MCU row per segment
constexpr int SEG_BLOCKS = 96;              // blocks of a segment at most: 32 MCUs x 3 (4:4:4), 16 x 6 (4:2:0)
constexpr int PLANE_FLOATS = 3 * 8 * SEG_PX;                    // 4:4:4: 3 planes of 8 x 256; 4:2:0: 16 x 256 + 2 x 8 x 128
constexpr int BB_WORDS = (SEG_BLOCKS * (int)jpeg_tab::BLOCK_MAX_BITS + 8 + 31) / 32 + 1;
static_assert(BB_WORDS <= PLANE_FLOATS, "the bit buffer takes the planes' place");
constexpr int RAW_STRIDE = SEG_PX * 3 + 16;                     // a staged pixel row: its bytes from the 16-byte boundary below
constexpr int COEF_STRIDE = 66;                                 // int16 per block in LDS: 33 words, no bank shared by blocks
constexpr int RAW_BYTES = 16 * RAW_STRIDE > SEG_BLOCKS * COEF_STRIDE * 2 ? 16 * RAW_STRIDE : SEG_BLOCKS * COEF_STRIDE * 2;

__host__ __device__ inline uint32_t jpeg_slot_bytes(const Geometry& g) { return (jpeg_tab::row_max_bytes(g) + 15u) / 16u * 16u; }

// 8-point orthonormal DCT-II: c[k] = cos(k pi / 16) / 2, v[u] = a(u) sum_x v[x] cos((2 x + 1) u pi / 16)
__device__ inline void dct8(float (&v)[8]) {
  constexpr float c1 = 0.49039264f, c2 = 0.46193977f, c3 = 0.41573481f, c4 = 0.35355339f, c5 = 0.27778512f, c6 = 0.19134172f,
                  c7 = 0.09754516f;
  const float s0 = v[0] + v[7], s1 = v[1] + v[6], s2 = v[2] + v[5], s3 = v[3] + v[4];
  const float d0 = v[0] - v[7], d1 = v[1] - v[6], d2 = v[2] - v[5], d3 = v[3] - v[4];
  const float e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
  v[0] = c4 * (e0 + e1);
  v[4] = c4 * (e0 - e1);
  v[2] = c2 * e2 + c6 * e3;
  v[6] = c6 * e2 - c2 * e3;
  v[1] = c1 * d0 + c3 * d1 + c5 * d2 + c7 * d3;
  v[3] = c3 * d0 - c7 * d1 - c1 * d2 - c5 * d3;
  v[5] = c5 * d0 - c1 * d1 + c7 * d2 + c3 * d3;
  v[7] = c7 * d0 - c5 * d1 + c3 * d2 - c1 * d3;
}

// The bit buffer: stream bit p is bit 31 - (p & 31) of word p >> 5.  `v`: nbits <= 27 bits, most significant first.
struct LdsBits {
  uint32_t* bb;
  uint32_t pos;
  __device__ void operator()(uint32_t v, uint32_t nbits) {
    const uint32_t wi = pos >> 5, end = (pos & 31u) + nbits;
    if (end <= 32u) {
      atomicOr(&bb[wi], v << (32u - end));
    } else {
      atomicOr(&bb[wi], v >> (end - 32u));
      atomicOr(&bb[wi + 1u], v << (64u - end));
    }
    pos += nbits;
  }
};
__device__ inline uint32_t bits_byte(const uint32_t* bb, uint32_t k) { return (bb[k >> 2] >> (24u - 8u * (k & 3u))) & 255u; }

// One workgroup per (MCU row, image).  coef_out != nullptr: the quantised coefficients, nothing else.
__global__ __launch_bounds__(T) void jpeg_rows_kernel(const uint8_t* __restrict__ in, size_t in_bytes, int h, int w, int c,
                                                           int sub420, int quality, uint32_t* __restrict__ row_size,
                                                           uint8_t* __restrict__ staging, uint32_t slot_bytes,
                                                           int16_t* __restrict__ coef_out) {
  __shared__ __attribute__((aligned(16))) uint32_t big[PLANE_FLOATS];          // the planes, then the bit buffer
  __shared__ __attribute__((aligned(16))) unsigned char rawc[RAW_BYTES];       // the staged pixel rows, then the coefficients
  __shared__ uint32_t codes[4][256];
  __shared__ float recip[2][64];
  __shared__ uint32_t scratch[T];
  __shared__ uint32_t wave_ff[T / 64];
  __shared__ int dc_carry[3];
  float* planes = reinterpret_cast<float*>(big);
  int16_t* coef = reinterpret_cast<int16_t*>(rawc);
  const int t = threadIdx.x;
  const int my = blockIdx.x, img = blockIdx.y;
  const Geometry g = jpeg_tab::geometry(h, w, c, sub420);
  const size_t idx = (size_t)img * g.mcus_y + my;

  if (t < 4) jpeg_tab::build_codes(t, codes[t]);
  if (t >= 64 && t < 64 + 128) {
    const int k = t - 64;
    recip[k >> 6][k & 63] = 1.0f / (float)jpeg_tab::scaled_quant(k >> 6, k & 63, quality);
  }
  if (t < 3) dc_carry[t] = 0;
  __syncthreads();

  const int y0 = my * g.mcu;
  const int padded_w = g.mcus_x * g.mcu;
  uint32_t carry_bits = 0, left = 0, out_bytes = 0;        // left: the carry_bits (< 8) bits a segment left over, in bits 31 ..
  uint8_t* slot = staging + idx * slot_bytes;
  for (int x0 = 0; x0 < padded_w; x0 += SEG_PX) {
    const int segw = padded_w - x0 < SEG_PX ? padded_w - x0 : SEG_PX;
    const int nm = segw / g.mcu, nb = nm * g.bpm;
    const int cw = segw / g.v;                                       // width of a chroma plane
    const bool last = x0 + SEG_PX >= padded_w;
    const int real_w = (x0 + segw < w ? x0 + segw : w) - x0;         // pixels the image has in this segment (>= 1)
    float* const pl_cb = planes + g.mcu * segw;
    float* const pl_cr = pl_cb + 8 * cw;

    // ---- the segment's pixel rows, 16 bytes at a time from the 16-byte boundary below each row's first byte; rows below
    //      the image repeat its last row ---------------------------------------------------------------------------------
    auto row_ptr = [&](int r) {
      const int ys = y0 + r < h ? y0 + r : h - 1;
      return in + (((size_t)img * h + ys) * w + x0) * c;
    };
    {
      const int per_row = (15 + real_w * c + 15) / 16;               // granules that can hold bytes of the row
      for (int k = t; k < g.mcu * per_row; k += T) {
        const int r = k / per_row, gi = k % per_row;
        const uint8_t* p = row_ptr(r);
        const uint8_t* a = p - (reinterpret_cast<uintptr_t>(p) & 15u) + 16 * gi;
        unsigned char* dst = rawc + r * RAW_STRIDE + 16 * gi;
        if (a >= in && a + 16 <= in + in_bytes) {
          *reinterpret_cast<u32x4*>(dst) = CGAN_LD_STREAM(reinterpret_cast<const u32x4*>(a));
        } else {
          for (int i = 0; i < 16; ++i) dst[i] = (a + i >= in && a + i < in + in_bytes) ? a[i] : (uint8_t)0;
        }
      }
    }
    __syncthreads();

    // ---- level shift / JFIF YCbCr (full range, BT.601); 4:2:0: the chroma of a 2 x 2 group is the mean of its pixels';
    //      columns right of the image repeat its last column ----------------------------------------------------------
    auto pixel = [&](int r, int x) { return rawc + r * RAW_STRIDE + (reinterpret_cast<uintptr_t>(row_ptr(r)) & 15u) + (x < real_w ? x : real_w - 1) * c; };
    if (c == 1) {
      for (int k = t; k < 8 * segw; k += T) {
        const int r = k / segw, x = k % segw;
        planes[k] = (float)pixel(r, x)[0] - 128.f;
      }
    } else if (g.v == 1) {
      for (int k = t; k < 8 * segw; k += T) {
        const int r = k / segw, x = k % segw;
        const unsigned char* p = pixel(r, x);
        const float R = p[0], G = p[1], B = p[2];
        planes[k] = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
        pl_cb[k] = -0.168736f * R - 0.331264f * G + 0.5f * B;
        pl_cr[k] = 0.5f * R - 0.418688f * G - 0.081312f * B;
      }
    } else {
      for (int k = t; k < 8 * cw; k += T) {
        const int r = k / cw, x = k % cw;
        float cb = 0.f, cr = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int rr = 2 * r + (d >> 1), xx = 2 * x + (d & 1);
          const unsigned char* p = pixel(rr, xx);
          const float R = p[0], G = p[1], B = p[2];
          planes[rr * segw + xx] = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
          cb += -0.168736f * R - 0.331264f * G + 0.5f * B;
          cr += 0.5f * R - 0.418688f * G - 0.081312f * B;
        }
        pl_cb[k] = 0.25f * cb;
        pl_cr[k] = 0.25f * cr;
      }
    }
    __syncthreads();

    // ---- DCT along the rows, in place: every plane's width is a multiple of 8, so the planes are one run of 8-value pieces -
    const int plane_floats = g.mcu * segw + (c == 3 ? 2 * 8 * cw : 0);
    for (int k = t; k < plane_floats / 8; k += T) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = planes[8 * k + i];
      dct8(v);
#pragma unroll
      for (int i = 0; i < 8; ++i) planes[8 * k + i] = v[i];
    }
    __syncthreads();

    // ---- DCT along the columns and quantisation: one thread per (block, column); the blocks in scan order --------------------
    for (int k = t; k < nb * 8; k += T) {
      const int b = k >> 3, j = k & 7;
      const int m = b / g.bpm, kb = b % g.bpm;
      const float* src;
      int stride, tbl;
      if (kb < g.ny) {
        src = planes + (kb / g.v) * 8 * segw + (m * g.v + kb % g.v) * 8 + j;
        stride = segw, tbl = 0;
      } else {
        src = (kb == g.ny ? pl_cb : pl_cr) + m * 8 + j;
        stride = cw, tbl = 1;
      }
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = src[i * stride];
      dct8(v);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float q = rintf(v[u] * recip[tbl][u * 8 + j]);
        if (u + j > 0) q = fminf(fmaxf(q, -1023.f), 1023.f);
        coef[b * COEF_STRIDE + u * 8 + j] = (int16_t)q;
      }
    }
    __syncthreads();

    if (coef_out) {
      for (int k = t; k < nb * 64; k += T) {
        const int b = k >> 6;
        int comp;
        const int64_t gb = jpeg_tab::coef_block(g, my, x0 / g.mcu + b / g.bpm, b % g.bpm, comp);
        coef_out[((int64_t)img * g.blocks + gb) * 64 + (k & 63)] = coef[b * COEF_STRIDE + (k & 63)];
      }
      __syncthreads();
      continue;
    }

    // ---- the blocks' code sizes (the DC before a block: the same component's block before it in scan order) and their scan --
    int prev_dc = 0;
    const uint32_t *dc_codes = codes[0], *ac_codes = codes[1];
    uint32_t bits = 0;
    if (t < nb) {
      const int kb = t % g.bpm;
      const int comp = kb < g.ny ? 0 : kb - g.ny + 1;
      const int pb = comp == 0 ? (kb > 0 ? t - 1 : t - g.bpm + g.ny - 1) : t - g.bpm;
      prev_dc = pb < 0 ? dc_carry[comp] : coef[pb * COEF_STRIDE];
      if (comp) dc_codes = codes[2], ac_codes = codes[3];
      bits = jpeg_tab::block_bits(coef + t * COEF_STRIDE, prev_dc, dc_codes, ac_codes);
    }
    scratch[t] = bits;
    for (int k = t; k < BB_WORDS; k += T)                       // the planes are dead: the bit buffer takes their place
      big[k] = k == 0 ? left : 0u;
    __syncthreads();
    row_files::scan(scratch);
    uint32_t total_bits = carry_bits + scratch[T - 1];
    if (t < nb) {
      LdsBits sink{big, carry_bits + scratch[t] - bits};
      jpeg_tab::code_block(coef + t * COEF_STRIDE, prev_dc, dc_codes, ac_codes, sink);
    }
    if (t == 0) {
      for (int comp = 0; comp < c; ++comp) dc_carry[comp] = coef[((nm - 1) * g.bpm + g.ny - 1 + comp) * COEF_STRIDE];
      if (last && (total_bits & 7u)) {                               // the interval ends: ones up to the byte boundary
        LdsBits pad{big, total_bits};
        pad((1u << (8u - (total_bits & 7u))) - 1u, 8u - (total_bits & 7u));
      }
    }
    if (last) total_bits = (total_bits + 7u) & ~7u;
    __syncthreads();

    // ---- the whole bytes to the slot, 00 behind every FF ------------------------------------------------------------------
    const uint32_t nbytes = total_bits >> 3;
    uint32_t ff_before = 0;
    for (uint32_t k0 = 0; k0 < nbytes; k0 += T) {
      const uint32_t k = k0 + t;
      const uint32_t byte = k < nbytes ? bits_byte(big, k) : 0u;
      const bool ff = byte == 0xFFu;
      const unsigned long long mask = __ballot(ff);
      const int lane = t & 63, wave = t >> 6;
      if (lane == 0) wave_ff[wave] = (uint32_t)__popcll(mask);
      __syncthreads();
      uint32_t pre = ff_before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), all = 0;
      for (int u = 0; u < T / 64; ++u) {
        if (u < wave) pre += wave_ff[u];
        all += wave_ff[u];
      }
      if (k < nbytes) {
        uint8_t* dst = slot + out_bytes + k + pre;
        dst[0] = (uint8_t)byte;
        if (ff) dst[1] = 0;
      }
      ff_before += all;
      __syncthreads();
    }
    out_bytes += nbytes + ff_before;
    carry_bits = total_bits & 7u;
    left = carry_bits ? bits_byte(big, nbytes) << 24 : 0u;
    __syncthreads();
  }
  if (t == 0 && !coef_out) row_size[idx] = out_bytes;
}

// one workgroup per image
__global__ __launch_bounds__(T) void jpeg_finish_kernel(int h, int w, int c, int sub420, int quality, int rows,
                                                             const uint32_t* __restrict__ row_size,
                                                             uint32_t* __restrict__ row_off, uint8_t* __restrict__ out,
                                                             size_t out_pitch, long long* __restrict__ sizes) {
  __shared__ uint32_t scratch[T];
  const size_t base = (size_t)blockIdx.x * rows;
  // the rows' data follows the headers, an RSTm (2 bytes) behind each row but the last
  const uint32_t running = row_files::row_offsets(scratch, row_size + base, row_off + base, rows, jpeg_tab::header_bytes(c), 2u);
  if (threadIdx.x != 0) return;
  uint8_t* f = out + (size_t)blockIdx.x * out_pitch;
  jpeg_tab::write_headers(f, h, w, c, sub420, quality);
  f[running] = 0xFF, f[running + 1u] = 0xD9;
  sizes[blockIdx.x] = (long long)running + 2;
}

// one workgroup per (MCU row, image): the row's data, its RSTm behind it
__global__ __launch_bounds__(T) void jpeg_gather_kernel(int rows, const uint32_t* __restrict__ row_size,
                                                             const uint32_t* __restrict__ row_off,
                                                             const uint8_t* __restrict__ staging, uint32_t slot_bytes,
                                                             uint8_t* __restrict__ out, size_t out_pitch) {
  const int r = blockIdx.x;
  const size_t idx = (size_t)blockIdx.y * rows + r;
  uint8_t* end = row_files::copy_row(staging + idx * slot_bytes, 0u, row_size[idx],
                                     out + (size_t)blockIdx.y * out_pitch + row_off[idx]);
  if (threadIdx.x == 0 && r + 1 < rows) end[0] = 0xFF, end[1] = (uint8_t)(0xD0 + (r & 7));
}

bool jpeg_args_ok(const char* what, int64_t n, int32_t h, int32_t w, int32_t c, int32_t quality, int32_t subsampling) {
  if (!row_files::channels_ok(what, c)) return false;
  if (subsampling != 444 && subsampling != 420) {
    cgan_set_error("%s: subsampling = %d: 444 or 420 only", what, subsampling);
    return false;
  }
  if (quality < 1 || quality > 100) {
    cgan_set_error("%s: quality = %d: 1 to 100 only", what, quality);
    return false;
  }
  if (w < 1 || w > row_files::MAX_W || h < 1 || h > JPEG_MAX_H) {
    cgan_set_error("%s: h = %d, w = %d: 1 to %d rows of 1 to %d pixels only", what, h, w, JPEG_MAX_H, row_files::MAX_W);
    return false;
  }
  const Geometry g = jpeg_tab::geometry(h, w, c, subsampling == 420);
  if (!row_files::grid_ok(n, g.mcus_y)) {
    cgan_set_error("%s: n = %lld: 1 <= n <= 65535 expected", what, (long long)n);
    return false;
  }
  return row_files::file_fits(what, h, w, c, jpeg_tab::file_max_bytes(g));
}

}  // namespace

// The bound of one file.  A block takes at most BLOCK_MAX_BITS = 22 + 63 * 26 bits: its DC difference a code of at most 11
// bits and 11 value bits, each of its 63 AC values at most the longest code, 16 bits, and 10 value bits (ZRL and EOB stand for
// at least one value each and are shorter).  An MCU row's blocks, padded to a whole byte, double when every byte is an FF that
// gets its 00: row_max_bytes.  Behind every row but the last stand the 2 bytes of an RSTm; SOI .. SOS take header_bytes(c)
// bytes (629 for RGB, 334 for grey) and EOI 2: file_max_bytes.
extern "C" size_t cgan_jpeg_bound_bytes(int32_t h, int32_t w, int32_t c, int32_t subsampling) {
  if (!jpeg_args_ok("cgan_jpeg_bound_bytes", 1, h, w, c, 50, subsampling)) return 0;
  return (size_t)jpeg_tab::file_max_bytes(jpeg_tab::geometry(h, w, c, subsampling == 420));
}

extern "C" size_t cgan_jpeg_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t subsampling) {
  if (!jpeg_args_ok("cgan_jpeg_workspace_bytes", n, h, w, c, 50, subsampling)) return 0;
  const Geometry g = jpeg_tab::geometry(h, w, c, subsampling == 420);
  const int64_t rows = (int64_t)n * g.mcus_y;
  return 2 * row_files::table_bytes(rows) + (size_t)rows * jpeg_slot_bytes(g);
}

extern "C" int cgan_jpeg_encode_u8(const uint8_t* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t quality,
                                   int32_t subsampling, uint8_t* out, size_t out_pitch, int64_t* sizes, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  CGAN_REQUIRE(in && out && sizes && workspace, "cgan_jpeg_encode_u8: null pointer");
  if (!jpeg_args_ok("cgan_jpeg_encode_u8", n, h, w, c, quality, subsampling)) return CGAN_ERR_BAD_ARG;
  if (const int rc = row_files::buffers_ok("cgan_jpeg_encode_u8", out_pitch, cgan_jpeg_bound_bytes(h, w, c, subsampling),
                                          workspace, workspace_bytes, cgan_jpeg_workspace_bytes(n, h, w, c, subsampling)))
    return rc;
  const int sub420 = subsampling == 420;
  const Geometry g = jpeg_tab::geometry(h, w, c, sub420);
  const int64_t all_rows = (int64_t)n * g.mcus_y;
  uint32_t* row_size = row_files::table(workspace, all_rows, 0);
  uint32_t* row_off = row_files::table(workspace, all_rows, 1);
  uint8_t* staging = reinterpret_cast<uint8_t*>(row_files::table(workspace, all_rows, 2));
  const uint32_t slot = jpeg_slot_bytes(g);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_rows_kernel, dim3(g.mcus_y, n), dim3(T), 0, s, in, (size_t)n * h * w * c, h, w, c, sub420,
                     quality, row_size, staging, slot, static_cast<int16_t*>(nullptr));
  CGAN_CHECK_LAUNCH("cgan_jpeg_encode_u8 (rows)");
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3(n), dim3(T), 0, s, h, w, c, sub420, quality, g.mcus_y, row_size, row_off,
                     out, out_pitch, reinterpret_cast<long long*>(sizes));
  CGAN_CHECK_LAUNCH("cgan_jpeg_encode_u8 (finish)");
  hipLaunchKernelGGL(jpeg_gather_kernel, dim3(g.mcus_y, n), dim3(T), 0, s, g.mcus_y, row_size, row_off, staging, slot,
                     out, out_pitch);
  CGAN_CHECK_LAUNCH("cgan_jpeg_encode_u8 (gather)");
  return CGAN_OK;
}

extern "C" int cgan_jpeg_coefficients_u8(const uint8_t* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t quality,
                                         int32_t subsampling, int16_t* coef, void* stream) {
  CGAN_REQUIRE(in && coef, "cgan_jpeg_coefficients_u8: null pointer");
  if (!jpeg_args_ok("cgan_jpeg_coefficients_u8", n, h, w, c, quality, subsampling)) return CGAN_ERR_BAD_ARG;
  const int sub420 = subsampling == 420;
  const Geometry g = jpeg_tab::geometry(h, w, c, sub420);
  hipLaunchKernelGGL(jpeg_rows_kernel, dim3(g.mcus_y, n), dim3(T), 0, static_cast<hipStream_t>(stream), in,
                     (size_t)n * h * w * c, h, w, c, sub420, quality, static_cast<uint32_t*>(nullptr),
                     static_cast<uint8_t*>(nullptr), 0u, coef);
  CGAN_CHECK_LAUNCH("cgan_jpeg_coefficients_u8");
  return CGAN_OK;
}

extern "C" int cgan_jpeg_tables(int32_t quality, uint8_t* luma, uint8_t* chroma) {
  CGAN_REQUIRE(luma && chroma, "cgan_jpeg_tables: null pointer");
  CGAN_REQUIRE(quality >= 1 && quality <= 100, "cgan_jpeg_tables: quality = %d: 1 to 100 only", quality);
  for (int i = 0; i < 64; ++i) {
    luma[i] = (uint8_t)jpeg_tab::scaled_quant(0, i, quality);
    chroma[i] = (uint8_t)jpeg_tab::scaled_quant(1, i, quality);
  }
  return CGAN_OK;
}

extern "C" int cgan_jpeg_scan_host(const int16_t* coef, int32_t h, int32_t w, int32_t c, int32_t quality, int32_t subsampling,
                                   uint8_t* out, size_t cap, size_t* size) {
  CGAN_REQUIRE(coef && out && size, "cgan_jpeg_scan_host: null pointer");
  if (!jpeg_args_ok("cgan_jpeg_scan_host", 1, h, w, c, quality, subsampling)) return CGAN_ERR_BAD_ARG;
  const Geometry g = jpeg_tab::geometry(h, w, c, subsampling == 420);
  for (int64_t b = 0; b < g.blocks; ++b) {
    const int16_t* v = coef + 64 * b;
    // the DC difference must fit category 11 whatever DC stands before it; an AC value category 10
    CGAN_REQUIRE(v[0] >= -1024 && v[0] <= 1023, "cgan_jpeg_scan_host: DC %d of block %lld is outside -1024 .. 1023", v[0],
                 (long long)b);
    for (int i = 1; i < 64; ++i)
      CGAN_REQUIRE(v[i] >= -1023 && v[i] <= 1023, "cgan_jpeg_scan_host: AC value %d of block %lld is outside +-1023", v[i],
                   (long long)b);
  }
  *size = (size_t)jpeg_tab::scan_host(coef, h, w, c, subsampling == 420, quality, out, cap);
  CGAN_REQUIRE(*size <= cap, "cgan_jpeg_scan_host: the file has %zu bytes, the buffer %zu", *size, cap);
  return CGAN_OK;
}
