// Masker evaluation (reference eval_masker.py + climategan/eval_metrics.py:133-542): the labelled test set's loader step,
// the classification sums of masker_classification_metrics and the edge coherence of edges_coherence_std_min, for a whole
// batch [n][h][w] per call.
//   cgan_mask_label_encode   crop_and_resize's nearest-neighbour label resize + centre crop + encode_mask_label's argmin
//   cgan_masker_eval         6 launches: counts + Sobel edges (tile partials) -> per-image finish of the counts -> column
//                            distances to the label edge -> exact squared distance per prediction-edge pixel (row pass)
//                            -> two-pass mean / population std of sqrt(d2) / h
// Integer sums are exact; fp64 sums are per-block partials reduced in a fixed order.  No atomics: every result is
// run-to-run identical and does not depend on the other images of the batch.
#include "cgan_common.h"

namespace {

constexpr int TW = 64, TH = 16;            // counts / edges tile: 64 columns x 16 rows, 256 threads, 4 rows per thread
constexpr int NONE = 0x3fffffff;           // "no label-edge pixel in this column"
constexpr int VR = 16;                     // rows per block of the variance pass
constexpr int ME_MAX_W = 16384;            // the row pass keeps one row of column distances in LDS
constexpr int ME_MAX_H = 16384;            // (h - 1)^2 + (w - 1)^2 < 2^32

// ---- label encoding ---------------------------------------------------------------------------------------------------
// classes_dict["flood"] (data.py:65-69): 0 cannot [255, 0, 0], 1 must [0, 0, 255], 2 may [0, 0, 0].  Integer squared
// distances; np.argmin keeps the first minimum (sqrt is strictly monotone on these integers, so the order is the same).
__device__ inline uint8_t flood_class(int r, int g, int b) {
  const int d0 = (r - 255) * (r - 255) + g * g + b * b;
  const int d1 = r * r + g * g + (b - 255) * (b - 255);
  const int d2 = r * r + g * g + b * b;
  int best = 0, bd = d0;
  if (d1 < bd) best = 1, bd = d1;
  if (d2 < bd) best = 2;
  return (uint8_t)best;
}

// skimage 0.18.3 resize(order=0): warp with the metric affine map src = f (dst + 0.5) - 0.5, f = in / out, and the
// nearest sample at round() (half away from zero); the coordinates stay inside [-0.5, in - 0.5), clamped for safety.
__device__ inline int nearest_src(int dst, double f, int in) {
  const double s = f * ((double)dst + 0.5) - 0.5;
  long r = (long)round(s);
  return (int)(r < 0 ? 0 : (r >= in ? in - 1 : r));
}

__global__ __launch_bounds__(256) void label_encode_kernel(const uint8_t* __restrict__ img, int h, int w, int c, int rows,
                                                           int cols, int top, int left, int oh, int ow,
                                                           uint8_t* __restrict__ out) {
  const int n = blockIdx.y;
  const long npix = (long)oh * ow;
  const double fr = (double)h / (double)rows, fc = (double)w / (double)cols;
  const uint8_t* src = img + (long)n * h * w * c;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int i = (int)(p / ow), j = (int)(p - (long)i * ow);
    const int si = nearest_src(i + top, fr, h), sj = nearest_src(j + left, fc, w);
    const uint8_t* px = src + ((long)si * w + sj) * c;
    out[(long)n * npix + p] = flood_class(px[0], px[1], px[2]);
  }
}

// ---- prediction loads -------------------------------------------------------------------------------------------------
// dtype: CGAN_F16 / CGAN_BF16 / CGAN_F32 / CGAN_MEVAL_U8 (bool or uint8) / CGAN_MEVAL_F64.  value(): the element as a
// double (exact for every type); one_minus(): (1.0 - pred) as numpy (fp16, fp32, fp64 arrays) or torch (bf16) computes it,
// in the element's own precision, then widened.
template <int D> struct Pred;
template <> struct Pred<CGAN_F16> {
  static constexpr bool integer = false;
  __device__ static double value(const void* p, long i) { return (double)(float)reinterpret_cast<const _Float16*>(p)[i]; }
  __device__ static double one_minus(const void* p, long i) {
    return (double)(float)(_Float16)(1.0f - (float)reinterpret_cast<const _Float16*>(p)[i]);
  }
};
template <> struct Pred<CGAN_BF16> {
  static constexpr bool integer = false;
  __device__ static double value(const void* p, long i) { return (double)(float)reinterpret_cast<const __bf16*>(p)[i]; }
  __device__ static double one_minus(const void* p, long i) {
    return (double)(float)(__bf16)(1.0f - (float)reinterpret_cast<const __bf16*>(p)[i]);
  }
};
template <> struct Pred<CGAN_F32> {
  static constexpr bool integer = false;
  __device__ static double value(const void* p, long i) { return (double)reinterpret_cast<const float*>(p)[i]; }
  __device__ static double one_minus(const void* p, long i) { return (double)(1.0f - reinterpret_cast<const float*>(p)[i]); }
};
template <> struct Pred<CGAN_MEVAL_F64> {
  static constexpr bool integer = false;
  __device__ static double value(const void* p, long i) { return reinterpret_cast<const double*>(p)[i]; }
  __device__ static double one_minus(const void* p, long i) { return 1.0 - reinterpret_cast<const double*>(p)[i]; }
};
template <> struct Pred<CGAN_MEVAL_U8> {
  static constexpr bool integer = true;
  __device__ static double value(const void* p, long i) { return (double)reinterpret_cast<const uint8_t*>(p)[i]; }
  __device__ static double one_minus(const void* p, long i) { return 1.0 - (double)reinterpret_cast<const uint8_t*>(p)[i]; }
};

// ---- fixed-order block reductions (256 threads = 4 waves) ------------------------------------------------------------
template <typename V>
__device__ inline V block_sum(V v, V* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return ((red[0] + red[1]) + (red[2] + red[3]));   // every thread gets the same value
}

// per-image quantities the counts kernel reduces per tile
enum { I_CANNOT, I_MUST, I_MAY, I_P_CANNOT, I_P_MUST, I_P_MAY, I_PE, I_LE, NI };
enum { F_TP, F_TN, F_FP, F_FN, F_MP, F_MN, NF };

// ---- pass 1: counts, metric maps, Sobel edges -------------------------------------------------------------------------
// One block per 64 x 16 tile of one image; the binarised prediction and the "must" indicator of the tile plus a one-pixel
// halo sit in LDS for the 3x3 Sobel stencil.  skimage 0.18.3 sobel: h = convolve(img, [[1,2,1],[0,0,0],[-1,-2,-1]] / 4),
// v = its transpose, the outer row / column of each zeroed, out = sqrt(h^2 + v^2) / sqrt(2).  On 0/1 input 4h and 4v
// are integers, so h^2 + v^2 = (16h^2 + 16v^2) / 16 exactly and the map equals the reference's bit for bit; an edge pixel
// is one with out > 0.  Interior pixels read only in-image neighbours, so the reflect mode never matters.
template <int D>
__global__ __launch_bounds__(256) void counts_edges_kernel(const void* __restrict__ pred, const uint8_t* __restrict__ labels,
                                                           int h, int w, int binarize, double th, double edge_th,
                                                           uint8_t* __restrict__ pred_edge, uint8_t* __restrict__ label_edge,
                                                           double* __restrict__ maps, double* __restrict__ sobel,
                                                           long long* __restrict__ part_i, double* __restrict__ part_f) {
  __shared__ uint8_t pb[TH + 2][TW + 2];
  __shared__ uint8_t lb[TH + 2][TW + 2];
  __shared__ long long red_i[4];
  __shared__ double red_f[4];
  const int n = blockIdx.y, tiles_x = (w + TW - 1) / TW;
  const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
  const long hw = (long)h * w, base = (long)n * hw;
  const bool integer = Pred<D>::integer || binarize;

  for (int k = threadIdx.x; k < (TH + 2) * (TW + 2); k += 256) {
    const int r = k / (TW + 2), c = k - r * (TW + 2);
    const int gy = y0 + r - 1, gx = x0 + c - 1;
    uint8_t pv = 0, lv = 0;
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
      const long i = base + (long)gy * w + gx;
      pv = Pred<D>::value(pred, i) > (binarize ? th : edge_th) ? 1 : 0;
      lv = labels[i] == 1 ? 1 : 0;
    }
    pb[r][c] = pv;
    lb[r][c] = lv;
  }
  __syncthreads();

  long long si[NI] = {0, 0, 0, 0, 0, 0, 0, 0};
  double sf[NF] = {0, 0, 0, 0, 0, 0};
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int x = x0 + tx;
  for (int k = 0; k < TH / 4; ++k) {
    const int ly = ty + 4 * k, y = y0 + ly;
    if (x >= w || y >= h) continue;
    const long i = base + (long)y * w + x;
    const int lab = labels[i];
    const long long c0 = lab == 0, c1 = lab == 1, c2 = lab == 2;
    si[I_CANNOT] += c0, si[I_MUST] += c1, si[I_MAY] += c2;
    double pv, qv;                                   // pred and (1.0 - pred) as the reference's maps hold them
    if (integer) {
      const long long v = binarize ? (long long)pb[ly + 1][tx + 1] : (long long)Pred<D>::value(pred, i);
      si[I_P_CANNOT] += v * c0, si[I_P_MUST] += v * c1, si[I_P_MAY] += v * c2;
      pv = (double)v, qv = 1.0 - (double)v;
    } else {
      pv = Pred<D>::value(pred, i), qv = Pred<D>::one_minus(pred, i);
      sf[F_TP] += pv * (double)c1, sf[F_TN] += qv * (double)c0, sf[F_FP] += pv * (double)c0;
      sf[F_FN] += qv * (double)c1, sf[F_MP] += pv * (double)c2, sf[F_MN] += qv * (double)c2;
    }
    if (maps) {                                      // tp tn fp fn may_pos may_neg (eval_metrics.py:211-224)
      const long plane = (long)gridDim.y * hw;
      maps[0 * plane + i] = pv * (double)c1;
      maps[1 * plane + i] = qv * (double)c0;
      maps[2 * plane + i] = pv * (double)c0;
      maps[3 * plane + i] = qv * (double)c1;
      maps[4 * plane + i] = pv * (double)c2;
      maps[5 * plane + i] = qv * (double)c2;
    }
    const bool interior = y > 0 && y < h - 1 && x > 0 && x < w - 1;
    int e[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
      uint8_t(*b)[TW + 2] = s == 0 ? pb : lb;
      const int r = ly + 1, c = tx + 1;
      const int gh = (b[r - 1][c - 1] + 2 * b[r - 1][c] + b[r - 1][c + 1]) - (b[r + 1][c - 1] + 2 * b[r + 1][c] + b[r + 1][c + 1]);
      const int gv = (b[r - 1][c - 1] + 2 * b[r][c - 1] + b[r + 1][c - 1]) - (b[r - 1][c + 1] + 2 * b[r][c + 1] + b[r + 1][c + 1]);
      const int m2 = interior ? gh * gh + gv * gv : 0;
      e[s] = m2 > 0;
      if (sobel) sobel[(long)s * gridDim.y * hw + i] = sqrt((double)m2 * 0.0625) / 1.4142135623730951;
    }
    pred_edge[i] = (uint8_t)e[0];
    label_edge[i] = (uint8_t)e[1];
    si[I_PE] += e[0], si[I_LE] += e[1];
  }

  const long tile = (long)n * gridDim.x + blockIdx.x;
  for (int q = 0; q < NI; ++q) {
    const long long v = block_sum(si[q], red_i);
    if (threadIdx.x == 0) part_i[tile * NI + q] = v;
  }
  if (!integer) {
    for (int q = 0; q < NF; ++q) {
      const double v = block_sum(sf[q], red_f);
      if (threadIdx.x == 0) part_f[tile * NF + q] = v;
    }
  }
}

// ---- pass 2: per-image finish of the tile partials --------------------------------------------------------------------
// res[n][16]: int64 slots 0..7 (enum I_*), fp64 slots 8..13 (enum F_*: the six masked sums, integer ones converted exactly),
// 14 = mean, 15 = std of the edge distances (pass 6).
__global__ __launch_bounds__(256) void finish_counts_kernel(const long long* __restrict__ part_i,
                                                            const double* __restrict__ part_f, int tiles, int integer,
                                                            long long* __restrict__ res) {
  __shared__ long long red_i[4];
  __shared__ double red_f[4];
  const int n = blockIdx.x;
  long long ti[NI];
  for (int q = 0; q < NI; ++q) {
    long long v = 0;
    for (int t = threadIdx.x; t < tiles; t += 256) v += part_i[((long)n * tiles + t) * NI + q];
    ti[q] = block_sum(v, red_i);
  }
  double tf[NF];
  if (integer) {
    tf[F_TP] = (double)ti[I_P_MUST], tf[F_TN] = (double)(ti[I_CANNOT] - ti[I_P_CANNOT]);
    tf[F_FP] = (double)ti[I_P_CANNOT], tf[F_FN] = (double)(ti[I_MUST] - ti[I_P_MUST]);
    tf[F_MP] = (double)ti[I_P_MAY], tf[F_MN] = (double)(ti[I_MAY] - ti[I_P_MAY]);
  } else {
    for (int q = 0; q < NF; ++q) {
      double v = 0;
      for (int t = threadIdx.x; t < tiles; t += 256) v += part_f[((long)n * tiles + t) * NF + q];
      tf[q] = block_sum(v, red_f);
    }
  }
  if (threadIdx.x == 0) {
    long long* r = res + (long)n * 16;
    for (int q = 0; q < NI; ++q) r[q] = ti[q];
    double* rf = reinterpret_cast<double*>(r + 8);
    for (int q = 0; q < NF; ++q) rf[q] = tf[q];
    rf[6] = 0.0, rf[7] = 0.0;
  }
}

// ---- pass 3: vertical distance to the nearest label-edge pixel of the same column ------------------------------------
// One thread per column: a downward and an upward sweep (coalesced across the wave's 64 neighbouring columns).
__global__ __launch_bounds__(256) void column_kernel(const uint8_t* __restrict__ label_edge, int h, int w,
                                                     const long long* __restrict__ res, int* __restrict__ g) {
  const int n = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
  if (x >= w) return;
  const long long* r = res + (long)n * 16;
  if (r[I_PE] == 0 || r[I_LE] == 0) return;             // nothing to measure (the row pass skips the image too)
  const long base = (long)n * h * w + x;
  int last = -1;
#pragma unroll 8
  for (int y = 0; y < h; ++y) {
    if (label_edge[base + (long)y * w]) last = y;
    g[base + (long)y * w] = last < 0 ? NONE : y - last;
  }
  int next = -1;
#pragma unroll 8
  for (int y = h - 1; y >= 0; --y) {
    if (label_edge[base + (long)y * w]) next = y;
    if (next >= 0) {
      const long o = base + (long)y * w;
      const int d = next - y;
      if (d < g[o]) g[o] = d;
    }
  }
}

// ---- pass 4: exact squared distance of every prediction-edge pixel to the label edge ---------------------------------
// d2(x, y) = min_x' (x - x')^2 + g(x', y)^2 over the row (one block per row, g in LDS), searched outwards from x and
// stopped as soon as (x - x')^2 alone reaches the best value: the exact brute-force minimum.  Writes d2 per edge pixel
// and the row's fixed-order partial sum of sqrt(d2) / h.
__global__ __launch_bounds__(256) void row_kernel(const uint8_t* __restrict__ pred_edge, const int* __restrict__ g, int h,
                                                  int w, const long long* __restrict__ res, unsigned* __restrict__ d2,
                                                  double* __restrict__ row_sum) {
  extern __shared__ int gs[];
  __shared__ double red[4];
  const int n = blockIdx.y, y = blockIdx.x;
  const long long* r = res + (long)n * 16;
  const bool live = r[I_PE] > 0 && r[I_LE] > 0;         // block-uniform
  double acc = 0.0;
  if (live) {
    const long row = ((long)n * h + y) * w;
    for (int x = threadIdx.x; x < w; x += 256) gs[x] = g[row + x];
    __syncthreads();
    const double hd = (double)h;
    for (int x = threadIdx.x; x < w; x += 256) {
      if (!pred_edge[row + x]) continue;
      unsigned long long best = ~0ull;
      for (int d = 0; d < w; ++d) {
        const unsigned long long dd = (unsigned long long)d * d;
        if (dd >= best) break;
        if (x - d >= 0 && gs[x - d] != NONE) {
          const unsigned long long v = dd + (unsigned long long)gs[x - d] * gs[x - d];
          if (v < best) best = v;
        }
        if (d > 0 && x + d < w && gs[x + d] != NONE) {
          const unsigned long long v = dd + (unsigned long long)gs[x + d] * gs[x + d];
          if (v < best) best = v;
        }
      }
      d2[row + x] = (unsigned)best;                      // a label edge exists: best is finite and < 2^32
      acc += sqrt((double)best) / hd;
    }
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) row_sum[(long)n * h + y] = s;
}

// mean of the distances from the row partials: the same fixed order in every block that needs it
__device__ inline double edge_mean(const double* row_sum, int h, long long count, double* red) {
  double v = 0.0;
  for (int y = threadIdx.x; y < h; y += 256) v += row_sum[y];
  return block_sum(v, red) / (double)count;
}

// ---- pass 5: sum of squared deviations, VR rows per block -------------------------------------------------------------
__global__ __launch_bounds__(256) void var_kernel(const uint8_t* __restrict__ pred_edge, const unsigned* __restrict__ d2,
                                                  int h, int w, const long long* __restrict__ res,
                                                  const double* __restrict__ row_sum, double* __restrict__ var_part) {
  __shared__ double red[4];
  const int n = blockIdx.y, parts = gridDim.x;
  const long long* r = res + (long)n * 16;
  double acc = 0.0;
  if (r[I_PE] > 0 && r[I_LE] > 0) {
    const double mean = edge_mean(row_sum + (long)n * h, h, r[I_PE], red);
    const long img = (long)n * h * w;
    const int y1 = min(h, (int)(blockIdx.x + 1) * VR);
    for (int y = blockIdx.x * VR; y < y1; ++y)
      for (int x = threadIdx.x; x < w; x += 256) {
        const long o = img + (long)y * w + x;
        if (!pred_edge[o]) continue;
        const double dv = sqrt((double)d2[o]) / (double)h - mean;
        acc += dv * dv;
      }
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) var_part[(long)n * parts + blockIdx.x] = s;
}

// ---- pass 6: per-image mean and population std (np.std, ddof 0) -------------------------------------------------------
// No prediction edge: 1.0 (eval_metrics.py:533-535).  Prediction edges but no label edge: nan (the reference's
// euclidean_distances raises ValueError; the caller reads the counts).
__global__ __launch_bounds__(256) void final_kernel(const double* __restrict__ row_sum, const double* __restrict__ var_part,
                                                    int h, int parts, long long* __restrict__ res) {
  __shared__ double red[4];
  const int n = blockIdx.x;
  long long* r = res + (long)n * 16;
  double* rf = reinterpret_cast<double*>(r + 8);
  const long long pe = r[I_PE], le = r[I_LE];
  if (pe == 0 || le == 0) {
    if (threadIdx.x == 0) rf[6] = pe == 0 ? 1.0 : __builtin_nan(""), rf[7] = pe == 0 ? 1.0 : __builtin_nan("");
    return;
  }
  const double mean = edge_mean(row_sum + (long)n * h, h, pe, red);
  double v = 0.0;
  for (int p = threadIdx.x; p < parts; p += 256) v += var_part[(long)n * parts + p];
  const double ss = block_sum(v, red);
  if (threadIdx.x == 0) rf[6] = mean, rf[7] = sqrt(ss / (double)pe);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
  size_t part_i, part_f, g, d2, row_sum, var_part, total;
};

Layout layout(int n, int h, int w) {
  const size_t tiles = (size_t)((w + TW - 1) / TW) * ((h + TH - 1) / TH), npix = (size_t)n * h * w;
  const size_t parts = (size_t)(h + VR - 1) / VR;
  Layout L;
  L.part_i = 0;
  L.part_f = L.part_i + align256((size_t)n * tiles * NI * 8);
  L.g = L.part_f + align256((size_t)n * tiles * NF * 8);
  L.d2 = L.g + align256(npix * 4);
  L.row_sum = L.d2 + align256(npix * 4);
  L.var_part = L.row_sum + align256((size_t)n * h * 8);
  L.total = L.var_part + align256((size_t)n * parts * 8);
  return L;
}

bool pred_dtype_ok(int d) {
  return d == CGAN_F16 || d == CGAN_BF16 || d == CGAN_F32 || d == CGAN_MEVAL_U8 || d == CGAN_MEVAL_F64;
}

}  // namespace

extern "C" int cgan_mask_label_encode(const void* img_hwc_u8, int32_t n, int32_t h, int32_t w, int32_t c, int32_t rows,
                                      int32_t cols, int32_t top, int32_t left, int32_t out_h, int32_t out_w, void* labels,
                                      void* stream) {
  CGAN_REQUIRE(img_hwc_u8 && labels, "mask_label_encode: null pointer");
  CGAN_REQUIRE(c == 3, "mask_label_encode: an RGB label image is expected (%d channels; encode_mask_label compares "
               "3-channel colours)", c);
  CGAN_REQUIRE(n > 0 && h > 0 && w > 0 && rows > 0 && cols > 0 && out_h > 0 && out_w > 0, "mask_label_encode: bad shape");
  CGAN_REQUIRE(top >= 0 && left >= 0 && top + out_h <= rows && left + out_w <= cols,
               "mask_label_encode: the %dx%d crop at (%d, %d) leaves the %dx%d resized image", out_h, out_w, top, left, rows,
               cols);
  CGAN_REQUIRE(n <= 65535, "mask_label_encode: at most 65535 images per call");
  const long npix = (long)out_h * out_w;
  long blocks = (npix + 256 * 4 - 1) / (256 * 4);
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(label_encode_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)img_hwc_u8, h, w, c, rows, cols, top, left, out_h, out_w, (uint8_t*)labels);
  CGAN_CHECK_LAUNCH("mask_label_encode");
  return CGAN_OK;
}

extern "C" size_t cgan_masker_eval_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return layout(n, h, w).total;
}

extern "C" int cgan_masker_eval(const void* pred, int32_t pred_dtype, const void* labels, int32_t n, int32_t h, int32_t w,
                                int32_t binarize, double threshold, double edge_threshold, void* pred_edge,
                                void* label_edge, double* maps, double* sobel, int64_t* res, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CGAN_REQUIRE(pred && labels && pred_edge && label_edge && res, "masker_eval: null pointer");
  CGAN_REQUIRE(pred_dtype_ok(pred_dtype), "masker_eval: bad prediction dtype %d", pred_dtype);
  CGAN_REQUIRE(n > 0 && h > 0 && w > 0, "masker_eval: bad shape %d x %d x %d", n, h, w);
  CGAN_REQUIRE(h <= ME_MAX_H && w <= ME_MAX_W && n <= 65535, "masker_eval: at most 65535 images of %d x %d pixels",
               ME_MAX_H, ME_MAX_W);
  CGAN_REQUIRE(binarize == 0 || binarize == 1, "masker_eval: binarize must be 0 or 1");
  const Layout L = layout(n, h, w);
  CGAN_REQUIRE(workspace && workspace_bytes >= L.total, "masker_eval: workspace of %zu bytes needed", L.total);
  char* ws = (char*)workspace;
  long long* part_i = (long long*)(ws + L.part_i);
  double* part_f = (double*)(ws + L.part_f);
  int* g = (int*)(ws + L.g);
  unsigned* d2 = (unsigned*)(ws + L.d2);
  double* row_sum = (double*)(ws + L.row_sum);
  double* var_part = (double*)(ws + L.var_part);
  const int tiles = ((w + TW - 1) / TW) * ((h + TH - 1) / TH), parts = (h + VR - 1) / VR;
  const int integer = pred_dtype == CGAN_MEVAL_U8 || binarize;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* lab = (const uint8_t*)labels;
  uint8_t *pe = (uint8_t*)pred_edge, *le = (uint8_t*)label_edge;
  long long* r = (long long*)res;

#define ME_COUNTS(D)                                                                                                     \
  hipLaunchKernelGGL(counts_edges_kernel<D>, dim3(tiles, n), dim3(256), 0, s, pred, lab, h, w, binarize, threshold,     \
                     edge_threshold, pe, le, maps, sobel, part_i, part_f)
  switch (pred_dtype) {
    case CGAN_F16: ME_COUNTS(CGAN_F16); break;
    case CGAN_BF16: ME_COUNTS(CGAN_BF16); break;
    case CGAN_F32: ME_COUNTS(CGAN_F32); break;
    case CGAN_MEVAL_F64: ME_COUNTS(CGAN_MEVAL_F64); break;
    default: ME_COUNTS(CGAN_MEVAL_U8); break;
  }
#undef ME_COUNTS
  CGAN_CHECK_LAUNCH("masker_eval (counts)");
  hipLaunchKernelGGL(finish_counts_kernel, dim3(n), dim3(256), 0, s, part_i, part_f, tiles, integer, r);
  CGAN_CHECK_LAUNCH("masker_eval (finish counts)");
  hipLaunchKernelGGL(column_kernel, dim3((w + 255) / 256, n), dim3(256), 0, s, le, h, w, r, g);
  CGAN_CHECK_LAUNCH("masker_eval (columns)");
  hipLaunchKernelGGL(row_kernel, dim3(h, n), dim3(256), (size_t)w * sizeof(int), s, pe, g, h, w, r, d2, row_sum);
  CGAN_CHECK_LAUNCH("masker_eval (rows)");
  hipLaunchKernelGGL(var_kernel, dim3(parts, n), dim3(256), 0, s, pe, d2, h, w, r, row_sum, var_part);
  CGAN_CHECK_LAUNCH("masker_eval (variance)");
  hipLaunchKernelGGL(final_kernel, dim3(n), dim3(256), 0, s, row_sum, var_part, h, parts, r);
  CGAN_CHECK_LAUNCH("masker_eval (final)");
  return CGAN_OK;
}
